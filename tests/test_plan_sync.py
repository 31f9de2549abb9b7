"""CPU check of what csrc/zs_plan.h decides for an inflate batch that finds its restart points
(zs_plan_sync over the candidates and the lanes' records, zs_sync_validate, the candidate cap, the
sync_pass range, the scan's tiles): tools/emu/emu_plan_sync.cpp, plain g++, no ROCm headers.  The
emulator itself refuses (exit 3) a plan whose points do not pass zs_restart_validate."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_sync.cpp")
LANDED, FINAL, ERROR, PASSED = 1, 2, 3, 4
OK, WBITS, D64, CAPS, ALIGN = range(5)  # zs_sync_err
SEG_MAX = 67108863


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_sync")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out = {}
        for line in r.stdout.splitlines():
            head, _, text = line.partition(" text=")
            kv = dict(f.split("=", 1) for f in head.split())
            kv["text"] = text
            out[kv.pop("case")] = kv
        return out

    return run


def ints(text):
    return [] if text in ("-", "") else [int(x) for x in text.split(",")]


def stream(in_len, first, cands, recs):
    """recs: the first point's lane, then one per candidate"""
    assert len(recs) == len(cands) + 1
    return "%d:%d:%s:%s" % (in_len, first, ",".join(map(str, cands)) or "-", ",".join(".".join(map(str, r)) for r in recs))


def plan(emu, streams, wbits=-15):
    p = emu(["plan x %d %s" % (wbits, "/".join(streams))])["x"]
    assert p["valid"] == "0"  # the emulator's own assertion: the points pass zs_restart_validate
    first, rin, rout = ints(p["first"]), ints(p["in"]), ints(p["out"])
    return [list(zip(rin[a:b], rout[a:b])) for a, b in zip(first, first[1:])]


X = (ERROR, 0, 0, 0)  # a lane that is on no chain


def test_the_chain_over_true_candidates(emu):
    s = stream(400, 0, [100, 200, 300], [(LANDED, 100, 1000, 0), (LANDED, 200, 500, 0), (LANDED, 300, 0, 0), (FINAL, 390, 7, 0)])
    assert plan(emu, [s]) == [[(0, 0), (100, 1000), (200, 1500), (300, 1500)]]  # out_pos: the lengths' prefix sums
    # two streams of one call: each follows its own candidates and records; a header in front of the first
    t = stream(90, 10, [50], [(LANDED, 50, 9, 0), (FINAL, 82, 1, 0)])
    assert plan(emu, [s, t, s], 31) == [[(0, 0), (100, 1000), (200, 1500), (300, 1500)], [(10, 0), (50, 9)],
                                        [(0, 0), (100, 1000), (200, 1500), (300, 1500)]]
    # no candidate: one point, whatever the lane found
    for how in (FINAL, ERROR, PASSED):
        assert plan(emu, [stream(50, 2, [], [(how, 40, 5, 0)])], 15) == [[(2, 0)]]


def test_false_candidates_are_skipped_and_those_behind_final_ignored(emu):
    s = stream(500, 0, [20, 100, 130, 200, 450, 470],
               [(LANDED, 100, 64, 0), X, (LANDED, 200, 10, 0), (PASSED, 470, 3, 0), (FINAL, 400, 5, 0), X, X])
    assert plan(emu, [s]) == [[(0, 0), (100, 64), (200, 74)]]


def test_an_error_or_a_passed_lane_mid_chain_gives_a_tail(emu):
    for how in (ERROR, PASSED):
        s = stream(500, 0, [100, 200, 300], [(LANDED, 100, 10, 0), (how, 250, 3, 0), (LANDED, 300, 10, 0), (FINAL, 490, 10, 0)])
        assert plan(emu, [s]) == [[(0, 0), (100, 10)]], how  # that lane's start is the last point
    # a landing that is no candidate, one under 5 bytes behind its start, one past the input: the chain stops there
    for end in (150, 104, 501):
        s = stream(500, 0, [100, 104, 200], [(LANDED, 100, 10, 0), (LANDED, end, 3, 0), X, X])
        assert plan(emu, [s]) == [[(0, 0), (100, 10)]], end
    # the output passes 2^32 - 1: the chain stops in front of it
    s = stream(500, 0, [100, 200], [(LANDED, 100, 0xffffff00, 0), (LANDED, 200, 0x100, 0), (FINAL, 490, 1, 0)])
    assert plan(emu, [s]) == [[(0, 0), (100, 0xffffff00)]]


def test_the_reach_stack(emu):
    def chain(reaches, lens=(1000, 1000, 1000, 1000)):
        cands = [100, 200, 300]
        recs = [(LANDED, c, n, r) for c, n, r in zip(cands, lens, reaches)] + [(FINAL, 390, lens[3], reaches[3])]
        return plan(emu, [stream(400, 0, cands, recs)])[0]

    all4 = [(0, 0), (100, 1000), (200, 2000), (300, 3000)]
    assert chain([0, 0, 0, 0]) == all4  # a reach of 0 keeps the point
    assert chain([0, 1, 0, 0]) == [all4[0], all4[2], all4[3]]  # a sync point dropped: its own
    assert chain([0, 0, 1000, 0]) == [all4[0], all4[1], all4[3]]  # up to the point before: that one stays
    assert chain([0, 0, 1001, 0]) == [all4[0], all4[3]]  # one byte before it: it goes too
    assert chain([0, 0, 0, 2500]) == [all4[0]]  # a later segment reaching past two earlier points drops both
    assert chain([0, 0, 0, 2000]) == [all4[0], all4[1]]
    assert chain([0, 1, 0, 1]) == [all4[0], all4[2]]
    assert chain([0, 0, 0, 5000]) == [all4[0]]  # past the first point: the stream's own error, the decode reports it
    assert chain([7, 0, 0, 0]) == all4  # the first point is never dropped
    assert chain([0, 1, 0, 0], lens=(0, 0, 0, 5)) == [(0, 0), (200, 0), (300, 0)]  # empty segments: equal out_pos
    # the tail's recorded reach counts like any segment's
    s = stream(400, 0, [100, 200], [(LANDED, 100, 50, 0), (LANDED, 200, 50, 0), (PASSED, 390, 9, 60)])
    assert plan(emu, [s]) == [[(0, 0)]]


def test_the_validators_fault_order_and_the_caps(emu):
    out = emu(["validate d64 -16 2 - 2,0", "validate d64_empty -16 0 - -", "validate wbits 14 2 - 2,0",
               "validate wbits0 0 2 16,16 0,16", "validate empty 31 0 - -", "validate caps 31 2 - 2,0",
               "validate align_off 15 2 16,16 2,16", "validate align_cap 15 2 18,16 0,20", "validate ok -15 2 16,16 0,16",
               "count at %d %d" % (1, SEG_MAX - 1), "count over %d %d" % (1, SEG_MAX), "count many 100 %d" % (SEG_MAX - 99),
               "count fits 100 %d" % (SEG_MAX - 100), "count none 5 0"] +
              ["pass p%d %d" % (v + 1, v) for v in (-1, 0, 1, 8, 64, 65)] +
              ["tiles t 0,20,4096,4097,67108864 3,15,0,0,1"])

    def v(name):
        return int(out[name]["device"]), int(out[name]["host"])

    # the format first, even of an empty batch and whatever else is wrong; then the capacities; alignment last
    assert v("d64") == v("d64_empty") == (D64, D64) and v("wbits") == v("wbits0") == (WBITS, WBITS)
    assert v("empty") == (OK, OK) and v("caps") == (CAPS, CAPS) and v("ok") == (OK, OK)
    assert v("align_off") == v("align_cap") == (ALIGN, OK)  # the host entries stage their own regions
    assert out["caps"]["text"] == "restart points are found with given capacities only"
    assert out["align_off"]["text"] == "output offsets/capacities must be multiples of 4"
    # candidates plus streams: the restart entries' segment cap
    assert [out[k]["ok"] for k in ("at", "over", "many", "fits", "none")] == ["1", "0", "0", "1", "1"]
    assert [out["p%d" % (x + 1)]["ok"] for x in (-1, 0, 1, 8, 64, 65)] == ["0", "0", "1", "1", "1", "0"]
    # an empty stream has no tile; 20 bytes one; a tile is 4,096 bytes of the aligned units the stream lies in
    assert ints(out["t"]["stile"]) == [0, 0, 1, 2, 4, 4 + 16385]
