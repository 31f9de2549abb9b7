"""CPU check of what csrc/zs_plan.h decides for a batch with Z_FULL_FLUSH points
(zs_deflate_make_req_flush, zs_deflate_validate*, zs_plan_flush, zs_plan_deflate over the segments,
zs_flush_layout, which capi.cpp runs before it launches anything): tools/emu/emu_plan_flush.cpp,
plain g++, no ROCm headers.  A batch without flush points must plan exactly what the header
planned before flush points existed: the figures test_plan_params.py pins as BEFORE."""
import os
import shutil
import subprocess

import pytest

from test_plan_params import BEFORE, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_flush.cpp")
# zs_deflate_err
OK, WBITS, LEVEL, ALIGN = 0, 1, 2, 13
FLUSH_MODE, FLUSH_INVALID, FLUSH_ARRAYS, FLUSH_POS, FLUSH_LEVEL0, FLUSH_MANY = 15, 16, 17, 18, 19, 20


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_flush")
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


def test_a_batch_without_flush_points_plans_what_the_header_planned_before(plans):
    for name, want in BEFORE.items():
        assert plans[name.replace("default", "noflush")] == fields(want), name
        req = plans[name.replace("default", "noflush_req")]
        assert (req["made"], req["valid"], req["any"]) == ("0", "0", "0"), name


def seg(plans, name):
    p = plans["seg/" + name]
    assert p["ok"] == "1" and p["fits"] == "1" and p["meta_after"] == "1", name
    return p


def test_segments_of_one_flush_point(plans):
    p = seg(plans, "one")
    assert (p["M"], ints(p["sfirst"]), ints(p["sstream"])) == ("2", [0, 2], [0, 0, 1])
    assert (ints(p["soff"]), ints(p["slen"])) == ([0, 40], [40, 60])
    assert ints(p["pos"]) == [0, 40] and ints(p["blk"]) == [0, 3] and p["B"] == "6"  # blocks, an empty one, the marker


def test_segments_at_the_ends_of_streams_of_0_1_and_3_bytes(plans):
    """a flush at 0 and at the end: empty segments, which still have their records"""
    p = seg(plans, "ends")
    # streams of 0, 1, 1, 3 bytes flushed at [0], [0], [1], [0, 3]
    assert ints(p["sfirst"]) == [0, 2, 4, 6, 9] and p["M"] == "9"
    assert ints(p["sstream"]) == [0, 0, 1, 1, 2, 2, 3, 3, 3, 4]
    assert ints(p["soff"]) == [0, 0, 0, 0, 0, 1, 0, 0, 3] and ints(p["slen"]) == [0, 0, 0, 1, 1, 0, 0, 3, 0]
    assert ints(p["pos"]) == [0, 0, 0, 0, 8, 16, 16, 16, 24]  # 8-aligned bases in the per-position tables
    assert ints(p["blk"]) == list(range(0, 27, 3)) and p["B"] == "27"
    assert p["nwin"] == "9" and ints(p["win_s"]) == list(range(9))  # a window per segment, the empty ones too


def test_segments_around_the_one_window_length(plans):
    """65,537 bytes is one sweep window, 65,538 two: per segment, not per stream"""
    p = seg(plans, "window")
    assert ints(p["slen"]) == [65537, 65537, 1, 65538, 65538] and ints(p["soff"]) == [0, 0, 65537, 0, 65538]
    assert ints(p["win_s"]) == [0, 1, 2, 3, 3, 4, 4]
    assert ints(p["blk"]) == [0, 7, 14, 17, 24] and p["max_blk"] == "7"  # 65,537 // 16,383 + 3


def test_segments_of_200000_bytes(plans):
    p = seg(plans, "long")
    assert ints(p["sfirst"]) == [0, 2, 6] and ints(p["slen"]) == [70000, 130000, 65536, 65536, 65536, 3392]
    assert ints(p["soff"]) == [0, 70000, 0, 65536, 131072, 196608]
    assert ints(p["pos"]) == [0, 70000, 200000, 265536, 331072, 396608]
    assert ints(p["win_s"]) == [0, 0, 1, 1, 1, 2, 3, 4, 5]  # 70,000: two windows; 130,000: three
    assert p["max_blk"] == "10"  # 130,000 // 16,383 + 3
    q = seg(plans, "long_l1")
    assert q["nwin"] == "0" and ints(q["blk"]) == [0, 7] and q["B"] == "17"
    assert ints(seg(plans, "blocks")["blk"]) == [0, 5]  # 32,766 bytes: two full blocks, the pending one, the marker, one spare


def test_the_layout_scan_of_256_segments_takes_two_tiles(plans):
    p = seg(plans, "many")
    assert p["M"] == "256" and p["tiles"] == "2" and int(p["scan"]) == 8 * 257 + 8 * 2
    assert ints(p["slen"]) == [4096] * 256 and ints(p["soff"]) == list(range(0, 1 << 20, 4096))
    assert seg(plans, "one")["tiles"] == "1"


def test_every_refusal_in_validation_order(plans):
    def r(name):
        p = plans["refuse/" + name]
        return int(p["made"]), int(p["device"]), int(p["host"])

    # the flush mode first, whatever else is wrong, before anything is validated
    for flush in (1, 2, 5):
        assert r("flush%d" % flush) == (FLUSH_MODE,) * 3
    for flush in (-1, 0, 4, 6):
        assert r("flush%d" % flush) == (FLUSH_INVALID,) * 3
    assert r("ok") == (OK, OK, OK)
    # windowBits and the level before the positions (these calls have equal positions too)
    assert r("wbits") == (OK, WBITS, WBITS) and r("level") == (OK, LEVEL, LEVEL)
    # the device entries' alignment rule before the positions; the host entries stage their own regions
    assert r("align") == (OK, ALIGN, FLUSH_POS)
    # the arrays before the positions, the positions before level 0
    assert r("null_first") == (OK, FLUSH_ARRAYS, FLUSH_ARRAYS) and r("null_pos") == (OK, FLUSH_ARRAYS, FLUSH_ARRAYS)
    assert r("null_pos_no_points") == (OK, OK, OK)
    for name in ("equal", "decreasing", "past_end", "first_decreasing"):
        assert r(name) == (OK, FLUSH_POS, FLUSH_POS), name
    assert r("at_end") == (OK, OK, OK)
    assert r("level0") == (OK, FLUSH_LEVEL0, FLUSH_LEVEL0) and r("level0_no_points") == (OK, OK, OK)
    assert r("many") == (OK, FLUSH_MANY, FLUSH_MANY) and r("many_fits") == (OK, OK, OK)  # 65,536 / 65,535 segments
    assert r("empty_batch") == (OK, OK, OK)
