"""CPU check of what csrc/zs_plan.h decides for an inflate batch with restart points
(zs_restart_validate, zs_plan_restart, zs_section_put, zs_plan_inflate over the segments' copies,
which capi.cpp runs before it launches anything): tools/emu/emu_plan_restart.cpp, plain g++, no ROCm
headers."""
import os
import shutil
import subprocess

import pytest

from test_plan_params import fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_restart.cpp")
# zs_restart_err
OK, WBITS, D64, ARRAYS, NO_FIRST, MANY, FIRST_OUT, IN_POS, OUT_POS, PAST_END, ALIGN = range(11)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_restart")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        kv = fields(line)
        out[kv.pop("case")] = kv
    return out


def ints(text):
    return [] if text in ("-", "") else [int(x) for x in text.split(",")]


def seg(plans, name):
    p = plans["seg/" + name]
    assert (p["valid"], p["aligned"], p["apart"], p["staged"], p["meta_after"]) == ("0", "1", "1", "1", "1"), name
    return p


def test_one_point_is_one_segment_that_ends_by_itself(plans):
    p = seg(plans, "one")
    assert (p["M"], p["in_place"], ints(p["rfirst"]), ints(p["rstream"])) == ("1", "1", [0, 1], [0])
    assert (ints(p["soff"]), ints(p["slen"]), ints(p["glen"])) == ([2], [98], [98])  # no 03 00: its own final block
    assert (ints(p["opos"]), ints(p["olen"]), ints(p["ocap"])) == ([0], [400], [400])
    assert p["stage"] == "0" and int(p["gather"]) == 112 + 16


def test_points_at_0_and_at_the_end(plans):
    """a marker alone behind the header; a last segment that is 03 00 and the trailer"""
    p = seg(plans, "ends")
    assert ints(p["soff"]) == [2, 7, 17] and ints(p["slen"]) == [5, 10, 6] and ints(p["glen"]) == [7, 12, 6]
    assert ints(p["goff"]) == [0, 16, 32]
    assert ints(p["opos"]) == [0, 0, 3] and ints(p["olen"]) == [0, 3, 5] and ints(p["ocap"]) == [0, 3, 5]
    assert p["in_place"] == "0" and ints(p["stoff"]) == [0, 0, 4]  # 3 is no multiple of 4


def test_abc_with_every_subset_of_the_positions(plans):
    for m in range(16):
        ps = [b for b in range(4) if m >> b & 1]
        p = seg(plans, "abc/%d" % m)
        assert int(p["M"]) == len(ps) + 1 and ints(p["rfirst"]) == [0, len(ps) + 1]
        assert ints(p["opos"]) == [0] + ps
        assert ints(p["olen"]) == [b - a for a, b in zip([0] + ps, ps)] + [4 - ([0] + ps)[-1]]  # the last: its room
        slen, glen = ints(p["slen"]), ints(p["glen"])
        assert glen == [x + 2 for x in slen[:-1]] + slen[-1:]
        assert ints(p["goff"]) == [16 * k for k in range(len(ps) + 1)]  # (every copy under 16 bytes)
        assert p["in_place"] == ("1" if all(b % 4 == 0 for b in ps) else "0"), m
        assert (p["stage"] == "0") == (p["in_place"] == "1")


def test_in_place_until_one_point_of_the_call_is_no_multiple_of_4(plans):
    a, b = seg(plans, "in_place"), seg(plans, "staged")
    assert a["in_place"] == "1" and a["stage"] == "0" and b["in_place"] == "0"
    assert ints(a["rfirst"]) == [0, 3, 5] and ints(a["rstream"]) == [0, 0, 0, 1, 1]
    assert ints(a["olen"]) == [400, 400, 200, 4, 996] and ints(b["olen"]) == [400, 400, 200, 5, 995]
    assert ints(b["stoff"]) == [0, 400, 800, 1000, 1008] and int(b["stage"]) == 1008 + 996 + 16
    # gather offsets: multiples of 16, each copy and its padding in front of the next
    assert ints(a["goff"]) == [0, 96, 208, 320, 464] and ints(a["glen"]) == [92, 102, 100, 142, 50]


def test_capacities_are_cut_at_the_streams_capacity(plans):
    p = seg(plans, "over")
    assert ints(p["olen"]) == [400, 400, 0] and ints(p["ocap"]) == [400, 100, 0] and ints(p["over"]) == [1]
    assert ints(seg(plans, "in_place")["over"]) == [0, 0]


def test_tiles_of_a_small_and_a_large_segment(plans):
    p = seg(plans, "tiles")
    assert ints(p["gtile"]) == [0, 1, 257] and ints(p["ptile"]) == [0, 1, 1025]


def test_only_first_points_plan_the_segment_batch_as_the_plain_batch(plans):
    a, b = plans["first_only/segments"], plans["first_only/direct"]
    assert a == b and ints(a["seg"]) == [3, 4, 5] and a["refw"] == "0"
    p = plans["first_only/plan"]
    assert p["in_place"] == "1" and ints(p["glen"]) == [0, 1, 100, 5000, 40000, 300000]


def test_every_refusal_in_validation_order(plans):
    def r(name):
        p = plans["refuse/" + name]
        return int(p["device"]), int(p["host"])

    assert r("ok") == (OK, OK) and r("empty_batch") == (OK, OK)
    # the format first, whatever else is wrong (here: every array null)
    assert r("d64") == (D64, D64) and r("wbits") == (WBITS, WBITS) and r("wbits0") == (WBITS, WBITS)
    for name in ("null_first", "null_in", "null_out"):
        assert r(name) == (ARRAYS, ARRAYS), name
    assert r("no_first") == (NO_FIRST, NO_FIRST) and r("first_decreasing") == (NO_FIRST, NO_FIRST)
    assert r("many") == (MANY, MANY)  # 67,108,864 segments: before any point is read
    assert r("first_out") == (FIRST_OUT, FIRST_OUT)
    for name in ("in_equal", "in_gap4", "in_decreasing", "in_then_out"):
        assert r(name) == (IN_POS, IN_POS), name
    assert r("in_gap5") == (OK, OK) and r("out_equal") == (OK, OK) and r("at_end") == (OK, OK)
    assert r("out_decreasing") == (OUT_POS, OUT_POS) and r("out_before_past_end") == (OUT_POS, OUT_POS)
    for name in ("past_end", "first_past_end", "in_before_past_end", "stream_order"):
        assert r(name) == (PAST_END, PAST_END), name
    # the device entry's alignment rule last; the host entries stage their own regions
    assert r("align") == (ALIGN, OK) and r("align_cap") == (ALIGN, OK) and r("align_after_points") == (IN_POS, IN_POS)
