"""CPU check of what csrc/zs_plan.h decides for an inflate batch that finds its gzip members
(zs_plan_members over the candidates and the lanes' records, zs_members_validate):
tools/emu/emu_plan_members.cpp, plain g++, no ROCm headers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_members.cpp")
FINAL, ERROR, PASSED = 2, 3, 4
OK, WBITS, CAPS, ALIGN = range(4)  # zs_members_err
X = (ERROR, 0, 0, 0)  # a lane that is on no chain


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_members")
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


def stream(in_len, out_cap, cands, recs):
    """recs: offset 0's lane, then one per candidate"""
    assert len(recs) == len(cands) + 1
    return "%d:%d:%s:%s" % (in_len, out_cap, ",".join(map(str, cands)) or "-", ",".join(".".join(map(str, r)) for r in recs))


def plan(emu, streams):
    p = emu(["plan x %s" % "/".join(streams)])["x"]
    first = ints(p["first"])
    mem = list(zip(ints(p["in"]), ints(p["len"]), ints(p["out"]), ints(p["cap"])))
    assert len(mem) == first[-1] and ints(p["stream"]) == [i for i, (a, b) in enumerate(zip(first, first[1:])) for _ in range(b - a)]
    return [mem[a:b] for a, b in zip(first, first[1:])], p


def test_the_chain_and_the_in_place_route(emu):
    s = stream(400, 100, [100, 150, 200, 300], [(FINAL, 100, 8, 0), (FINAL, 200, 12, 0), X, (FINAL, 300, 4, 0), (FINAL, 390, 7, 0)])
    t = stream(90, 16, [], [(FINAL, 82, 1, 0)])
    mem, p = plan(emu, [s, t])
    # (in_pos, in_len, out_pos, cap); the candidate at 150 lies inside a member and is on no chain; the bytes
    # from 390 on pass no test and are ignored
    assert mem == [[(0, 100, 0, 8), (100, 100, 8, 12), (200, 100, 20, 4), (300, 90, 24, 7)], [(0, 82, 0, 1)]]
    assert p["in_place"] == "1" and p["stage"] == "0" and p["tstream"] == "-"
    # the place's tiles count even so (they are not launched in place)
    assert ints(p["ptile"]) == [0, 1, 2, 3, 4, 5]


def test_the_staged_route(emu):
    """an out_pos that is no multiple of 4: 4-aligned staging regions, their prefix sums"""
    s = stream(400, 5000, [100, 200], [(FINAL, 100, 5, 0), (FINAL, 200, 4096, 0), (FINAL, 390, 2, 0)])
    mem, p = plan(emu, [stream(50, 8, [], [(FINAL, 50, 8, 0)]), s])
    assert mem[1] == [(0, 100, 0, 5), (100, 100, 5, 4096), (200, 190, 4101, 2)]
    assert p["in_place"] == "0" and ints(p["stoff"]) == [0, 8, 16, 4112] and p["stage"] == str(4116 + 16)
    assert ints(p["ptile"]) == [0, 1, 2, 4, 5]  # (4096 bytes and a leading partial word: two tiles)
    # a stream's FIRST member never decides the route: out_pos 0
    _, p = plan(emu, [stream(50, 8, [], [(FINAL, 50, 7, 0)]), stream(50, 8, [], [(FINAL, 50, 3, 0)])])
    assert p["in_place"] == "1"


def test_the_capacity_cut(emu):
    recs = [(FINAL, 100, 8, 0), (FINAL, 200, 12, 0), (FINAL, 300, 4, 0)]
    for cap, want in [(24, [8, 12, 4]), (23, [8, 12, 0]), (20, [8, 12, 0]), (19, [8, 0]), (8, [8, 0]), (7, [0]), (0, [0])]:
        mem, _ = plan(emu, [stream(300, cap, [100, 200], recs)])
        assert [c for _, _, _, c in mem[0]] == want, cap  # the first member that does not fit: no room, and the last
        assert [(a, n) for a, n, _, _ in mem[0]] == [(0, 100), (100, 100), (200, 100)][:len(want)]
    # an empty member fits a full region
    mem, _ = plan(emu, [stream(200, 8, [100], [(FINAL, 100, 8, 0), (FINAL, 200, 0, 0)])])
    assert mem == [[(0, 100, 0, 8), (100, 100, 8, 0)]]
    # a total above 2^32 - 1 never fits, whatever the capacity
    big = 0xffffffff
    mem, _ = plan(emu, [stream(200, big, [100], [(FINAL, 100, big - 1, 0), (FINAL, 200, 2, 0)])])
    assert mem == [[(0, 100, 0, big - 1), (100, 100, big - 1, 0)]]


def test_error_at_start_0_and_behind_members(emu):
    """ERROR: the stream's last member, with the input to the end and the room that is left"""
    mem, p = plan(emu, [stream(77, 40, [], [(ERROR, 0, 0, 0)]), stream(0, 8, [], [(ERROR, 0, 0, 0)])])
    assert mem == [[(0, 77, 0, 40)], [(0, 0, 0, 8)]] and p["in_place"] == "1"
    mem, _ = plan(emu, [stream(300, 40, [100, 200], [(FINAL, 100, 8, 0), (ERROR, 150, 3, 0), (FINAL, 300, 4, 0)])])
    assert mem == [[(0, 100, 0, 8), (100, 200, 8, 32)]]
    # a FINAL record that does not move, or ends past the input, is no member either
    mem, _ = plan(emu, [stream(300, 40, [], [(FINAL, 0, 8, 0)]), stream(300, 40, [], [(FINAL, 301, 8, 0)])])
    assert mem == [[(0, 300, 0, 40)], [(0, 300, 0, 40)]]


def test_more_than_64_members(emu):
    n = 150
    cands = [10 * k for k in range(1, n)]
    recs = [(FINAL, 10 * (k + 1), k % 3 + 1, 0) for k in range(n)]
    mem, p = plan(emu, [stream(10 * n + 5, 10000, cands, recs)])
    outs, o = [], 0
    for k in range(n):
        outs.append(o)
        o += k % 3 + 1
    assert mem == [[(10 * k, 10, outs[k], k % 3 + 1) for k in range(n)]]
    assert p["in_place"] == "0"


def test_a_passed_lane_goes_on_the_tail_list(emu):
    s = stream(400, 100, [100, 200], [(FINAL, 100, 8, 0), (PASSED, 150, 0, 0), X])
    t = stream(400, 100, [100], [(PASSED, 100, 0, 0), X])
    mem, p = plan(emu, [s, t])
    assert ints(p["tstream"]) == [0, 1] and ints(p["tstart"]) == [100, 0] and ints(p["trec"]) == [2, 1]
    assert mem == [[(0, 100, 0, 8)], []]  # the members in front of the open starts; complete once no start is listed


def test_the_validation_order(emu):
    lines = [
        "validate a -15 2 - -", "validate b 15 0 - -", "validate c 31 0 - -", "validate d 31 2 - 0,16",
        "validate e 31 2 16,16 2,16", "validate f 31 2 18,16 0,16", "validate g 31 2 16,16 0,16", "validate h 30 2 18,16 2,16",
    ]
    r = emu(lines)
    got = {k: (int(v["device"]), int(v["host"]), v["text"]) for k, v in r.items()}
    assert got["a"] == (WBITS, WBITS, "members are a gzip notion (use windowBits 31)")
    assert got["b"][:2] == (WBITS, WBITS) and got["h"][:2] == (WBITS, WBITS)  # the format first, even of an empty batch
    assert got["c"][:2] == (OK, OK)
    assert got["d"] == (CAPS, CAPS, "members are found with given capacities only")
    assert got["e"] == (ALIGN, OK, "output offsets/capacities must be multiples of 4")
    assert got["f"][:2] == (ALIGN, OK) and got["g"][:2] == (OK, OK)
