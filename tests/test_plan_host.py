"""CPU check of what csrc/zs_plan.h decides about a host-buffer batch before capi.cpp's host_batch_run
stages anything (zs_plan_host_chunks, zs_plan_host_pack0 and the values of options "host_chunk_min" /
"host_pack_min"): tools/emu/emu_plan_host.cpp, plain g++, no ROCm headers.  With the defaults the
bounds and the guess are the literals the host layer held before the options existed: four chunks at
n/8, 4n/8, 7n/8 from 64 streams and 32 MiB on, min(tout, max(4 tin, 64 MiB)) + 16."""
import os
import shutil
import subprocess

import pytest

from test_plan_params import fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_host.cpp")
MIN = 32 << 20
PACK = 64 << 20


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        kv = fields(line)
        out[kv.pop("case")] = kv
    return out


def bnd(p):
    return [int(x) for x in p["bnd"].split(",")]


def four(n):
    return [0, n // 8, n // 2, 7 * n // 8, n]


def test_defaults_are_the_literals_the_host_layer_held(plans):
    assert plans["defaults"] == {"chunk_min": str(MIN), "pack_min": str(PACK), "streams": "64"}


@pytest.mark.parametrize("n", [63, 64, 65, 67, 71, 520, 4096])
def test_bounds_on_both_sides_of_the_thresholds(plans, n):
    """tin one below, at and above 32 MiB; the 64-stream floor"""
    below, at, above = (plans["default/n%d/%s" % (n, w)] for w in ("below", "at", "above"))
    assert (int(below["tin"]), int(at["tin"]), int(above["tin"])) == (MIN - 1, MIN, MIN + 1)
    assert bnd(below) == [0, n] and below["K"] == "1"
    want = four(n) if n >= 64 else [0, n]
    for p in (at, above):
        assert bnd(p) == want and int(p["K"]) == len(want) - 1
    for p in (below, at, above):
        assert (p["cover"], p["nonempty"]) == ("1", "1")


def test_the_bounds_of_the_tests_batches(plans):
    assert four(64) == [0, 8, 32, 56, 64]
    assert four(67) == [0, 8, 33, 58, 67]
    assert four(71) == [0, 8, 35, 62, 71]
    assert four(520) == [0, 65, 260, 455, 520]
    for n in (64, 67, 71, 520):
        assert bnd(plans["min1/n%d/t1" % n]) == four(n)
        assert bnd(plans["min1/n%d/t5000" % n]) == four(n)
        assert bnd(plans["min1/n%d/t0" % n]) == [0, n]  # no input at all: below a threshold of 1
    for t in (0, 1, 5000):
        assert bnd(plans["min1/n63/t%d" % t]) == [0, 63]  # the floor of 64 streams is a constant


def test_small_and_empty_batches_run_as_one_chunk(plans):
    for n in (0, 1):
        for w in ("below", "at", "above"):
            p = plans["default/n%d/%s" % (n, w)]
            assert bnd(p) == [0, n] and p["cover"] == "1"
    assert bnd(plans["default/empty_input"]) == [0, 4096]


def test_host_chunk_min_0_never_chunks(plans):
    assert bnd(plans["never/n64"]) == [0, 64]
    assert bnd(plans["never/n4096"]) == [0, 4096]


def test_the_largest_values(plans):
    assert bnd(plans["max/n64/below"]) == [0, 64]
    assert bnd(plans["max/n64/at"]) == four(64)
    n = 0xFFFFFFFF
    p = plans["default/4g"]
    assert bnd(p) == four(n) and (p["cover"], p["nonempty"]) == ("1", "1")


def test_chunks_are_never_empty_and_cover_the_batch(plans):
    assert plans["sweep/64..4200"]["ok"] == "1"
    for name, p in plans.items():
        if "cover" in p:
            assert p["cover"] == "1", name
            if int(p["n"]) >= 64:
                assert p["nonempty"] == "1", name


def test_the_pack_buffers_first_guess(plans):
    """min(tout, max(4 tin, floor)) + 16, on both sides of the min and of the max"""
    seen = 0
    for name, p in plans.items():
        if not name.startswith("pack/"):
            continue
        floor = {"default": PACK, "1m": 1 << 20, "0": 0}[name.split("/")[1]]
        tin, tout = int(p["tin"]), int(p["tout"])
        assert int(p["pack0"]) == min(tout, max(4 * tin, floor)) + 16, name
        seen += 1
    assert seen == 23
    d = lambda k: int(plans["pack/default/" + k]["pack0"]) - 16
    assert (d("tout_small"), d("tout_at_floor"), d("tout_past_floor")) == (4000, PACK, PACK)
    assert (d("tin4_below_floor"), d("tin4_at_floor"), d("tin4_past_floor")) == (PACK, PACK, PACK + 4)
    assert (d("tout_below_tin4"), d("tout_at_tin4"), d("tout_past_tin4")) == (4 * PACK - 1, 4 * PACK, 4 * PACK)
    assert d("zeros_96m") == PACK  # less than the 96 MiB such a batch produces: the buffers grow in the call
    assert int(plans["pack/1m/zeros_96m"]["pack0"]) - 16 == 1 << 20
    assert int(plans["pack/1m/tout_small"]["pack0"]) - 16 == 4000


def test_option_values(plans):
    ok = lambda kind, v: plans["opt/%s/%d" % (kind, v)]["ok"] == "1"
    for v in (-(1 << 31), -1):
        assert not ok("chunk", v) and not ok("pack", v)
    for v in (0, 1, 1 << 20, 0x7FFFFFFF):
        assert ok("chunk", v) and ok("pack", v)
    assert ok("chunk", MIN) and ok("pack", PACK)
