"""CPU check of the routes of the compression strategies (csrc/zs_plan.h,
zs_plan_strategy, which capi.cpp runs before it launches anything):
tools/emu/emu_plan_strategy.cpp, plain g++, no ROCm headers.  The expected routes are
the reference's dispatch (deflate.ts:923-931) and what each strategy touches:
Z_FILTERED deflate_slow alone (deflate.ts:1381-1387), Z_HUFFMAN_ONLY and Z_RLE their own
tallies, Z_FIXED the block-type choice (trees.ts:567), the wrappers strategy >= 2
(deflate.ts:757,798)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_strategy.cpp")
LEVEL, HUFF, RLE = 0, 1, 2  # ZS_TALLY_*


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_strategy")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        kv = dict(f.split("=", 1) for f in line.split())
        out[kv["case"]] = kv
    return out


def has(case, **want):
    got = {k: case.get(k) for k in want}
    assert got == {k: str(v) for k, v in want.items()}, case["case"]


def test_level_0_is_stored_whatever_the_strategy(plans):
    for r in (0, 1):
        for s in range(5):
            has(plans["r%d/l0/s%d" % (r, s)], stored=1, tally=LEVEL, filtered=0, fixed=0, wrap_strategy=0)


def test_strategy_0_is_the_plain_path(plans):
    for r in (0, 1):
        for level in range(1, 10):
            has(plans["r%d/l%d/s0" % (r, level)], stored=0, tally=LEVEL, filtered=0, fixed=0, wrap_strategy=0,
                plan_level=level)


def test_filtered_changes_the_lazy_parse_only(plans):
    for level in range(1, 10):
        c = plans["r1/l%d/s1" % level]
        has(c, tally=LEVEL, filtered=1 if level >= 4 else 0, fixed=0, wrap_strategy=1, plan_level=level)
        plain = plans["r1/l%d/s0" % level]
        assert (c["nwin"], c["pscr"]) == (plain["nwin"], plain["pscr"])  # the match kernels and the scratch untouched


def test_huffman_only_and_rle_take_the_tally_kernels(plans):
    for level in range(1, 10):
        for r in (0, 1):
            has(plans["r%d/l%d/s2" % (r, level)], tally=HUFF, filtered=0, fixed=0, wrap_strategy=2, plan_level=1, nwin=0,
                pscr=0)
        # Z_RLE: the reference's tally is deflate_huff's (rle_ref = 1); zlib's has its own kernel
        has(plans["r1/l%d/s3" % level], tally=HUFF, wrap_strategy=3, plan_level=1, nwin=0, pscr=0)
        has(plans["r0/l%d/s3" % level], tally=RLE, wrap_strategy=3, plan_level=1, nwin=0, pscr=0)


def test_fixed_is_a_flag_of_the_trees(plans):
    for level in range(1, 10):
        has(plans["r1/l%d/s4" % level], tally=LEVEL, filtered=0, fixed=1, wrap_strategy=4, plan_level=level)


def test_the_huffman_grid_lists_every_block_once(plans):
    # lengths 0, 1, 16382, 16383, 16384, 32766, 200000: n / 16383 + 1 blocks each (the last may be empty)
    want = ["0:0", "1:0", "2:0", "3:0", "3:1", "4:0", "4:1", "5:0", "5:1", "5:2"] + ["6:%d" % b for b in range(13)]
    has(plans["chunks"], n=len(want), list=",".join(want))
    has(plans["records"], fits=1)
