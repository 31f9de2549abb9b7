"""CPU check of what csrc/zs_plan.h decides for a BGZF batch (zs_deflate_make_req_bgzf, zs_deflate_validate*,
zs_plan_bgzf, zs_plan_deflate over the segments, zs_bgzf_bound, which capi.cpp runs before it launches anything):
tools/emu/emu_plan_bgzf.cpp, plain g++, no ROCm headers.  The plain plan and the flushed request's plan must stay
field for field what the header planned before: the figures test_plan_params.py pins as BEFORE."""
import os
import shutil
import subprocess

import pytest

import bgzfwritecases as w
from test_plan_params import BEFORE, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_bgzf.cpp")
B = 65280
# zs_deflate_err
OK, LEVEL, ALIGN, BGZF_BLOCK, BGZF_ARRAYS, BGZF_MANY = 0, 2, 13, 21, 22, 23


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_bgzf")
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


def seg(plans, name, stored=False):
    p = plans["seg/" + name]
    assert p["ok"] == "1" and p["fits"] == "1" and p["stored"] == ("1" if stored else "0"), name
    return p


def test_plain_and_flushed_plans_are_what_the_header_planned_before(plans):
    for name, want in BEFORE.items():
        assert plans[name.replace("default", "plain")] == fields(want), name
        assert plans[name.replace("default", "noflush")] == fields(want), name
        assert plans[name.replace("default", "plain_req")] == {"bgzf": "0", "flush": "0"}, name


@pytest.mark.parametrize("name", ["b0", "b65280"])
def test_segments_around_the_block_size(plans, name):
    """lengths 0, 1, B - 1, B, B + 1, 2B + 1: block_bytes 0 is 65,280"""
    p = seg(plans, name)
    assert ints(p["sfirst"]) == [0, 0, 1, 2, 3, 5, 8] and p["M"] == "8"  # the empty stream has no segment
    assert ints(p["sstream"]) == [1, 2, 3, 4, 4, 5, 5, 5, 6]
    assert ints(p["soff"]) == [0, 0, 0, 0, B, 0, B, 2 * B] and ints(p["slen"]) == [1, B - 1, B, B, 1, B, B, 1]
    # no marker: n / 16,383 + 2 records a segment (the flushed plan has one more)
    assert ints(p["blk"]) == [0, 2, 7, 12, 17, 19, 24, 29] and p["B"] == "31" and p["max_blk"] == "5"
    assert int(p["bound"]) == sum(w.bound(n) for n in (0, 1, B - 1, B, B + 1, 2 * B + 1))


def test_segments_of_7_and_of_1_byte(plans):
    p = seg(plans, "b7")
    assert ints(p["sfirst"]) == [0, 0, 1, 2, 3, 5, 8]
    assert ints(p["soff"]) == [0, 0, 0, 0, 7, 0, 7, 14] and ints(p["slen"]) == [1, 6, 7, 7, 1, 7, 7, 1]
    assert int(p["bound"]) == sum(w.bound(n, 7) for n in (0, 1, 6, 7, 8, 15))
    q = seg(plans, "b1")
    assert ints(q["sfirst"]) == [0, 0, 1, 3, 6] and ints(q["soff"]) == [0, 0, 1, 0, 1, 2] and ints(q["slen"]) == [1] * 6
    assert int(q["bound"]) == sum(w.bound(n, 1) for n in (0, 1, 2, 3))


def test_an_empty_stream_between_two_others_has_no_segment(plans):
    p = seg(plans, "empty_between")
    assert ints(p["sfirst"]) == [0, 2, 2, 3] and ints(p["sstream"]) == [0, 0, 2, 3]
    assert ints(p["soff"]) == [0, 100, 0] and ints(p["slen"]) == [100, 50, 100]
    q = seg(plans, "all_empty")
    assert q["M"] == "0" and ints(q["sfirst"]) == [0, 0, 0] and q["tiles"] == "1" and int(q["bound"]) == 56


def test_level_0_plans_the_segments_and_no_parse(plans):
    p = seg(plans, "level0", stored=True)
    assert ints(p["sfirst"]) == [0, 0, 1, 2, 4] and ints(p["slen"]) == [1, B, B, 1]


def test_600_segments_take_three_tiles_of_the_scan(plans):
    p = seg(plans, "many")
    assert p["M"] == "600" and p["tiles"] == "3" and int(p["scan"]) == 8 * 601 + 8 * 3
    assert ints(p["slen"]) == [256] * 600
    assert ints(seg(plans, "cut")["blk"]) == [0, 3]  # 16,383 bytes: the full block, the empty one behind it, one spare


def test_every_refusal_in_order(plans):
    def r(name):
        p = plans["refuse/" + name]
        return tuple(int(p[k]) for k in ("made", "pre", "pre_host", "device", "host"))

    assert r("ok") == r("ok_m1") == r("ok_level0") == (OK,) * 5
    assert plans["refuse/ok"]["block"] == plans["refuse/ok_m1"]["block"] == "65280"
    assert plans["refuse/ok_level0"]["block"] == "1"
    # the level first, whatever else is wrong; then the block size
    assert r("level") == r("level_low") == (LEVEL,) * 5
    assert r("block") == r("block_huge") == (BGZF_BLOCK,) * 5
    # the arrays; an empty batch has none to miss
    assert r("null") == (OK, BGZF_ARRAYS, BGZF_ARRAYS, BGZF_ARRAYS, BGZF_ARRAYS)
    assert r("null_empty_batch") == (OK,) * 5
    # the device batch's alignment rule; the host entries stage their own regions
    assert r("align") == (OK, OK, OK, ALIGN, OK)
    # streams + data blocks of one device call: 65,536 refused, 65,535 taken; a host call counts per chunk
    assert r("many") == r("many_b7") == (OK, BGZF_MANY, OK, BGZF_MANY, OK)
    assert r("many_fits") == r("many_b7_fits") == (OK,) * 5
    assert r("empty_batch") == (OK,) * 5
