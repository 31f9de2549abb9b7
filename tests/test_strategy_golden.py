"""CPU: the goldens of the compression-strategy tests (tests/golden/deflate_strategy.json)
are what gen_deflate_strategy.py writes where zlib 1.2.11 runs, and the cases are not
vacuous: on the yardstick itself each strategy's bytes differ from the bytes the cases
would also pass with -- Z_FILTERED and Z_FIXED from strategy 0 on text, zlib's Z_RLE
(rle_ref = 0) from the reference's (rle_ref = 1) on the run cases -- and they agree where
the engine routes to an existing path (Z_FILTERED at levels 1..3)."""
import os
import subprocess
import sys
import zlib

import pytest

import strategycases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "gen_deflate_strategy.py")

zlib_1_2_11 = pytest.mark.skipif(zlib.ZLIB_RUNTIME_VERSION != "1.2.11", reason="the yardstick is zlib 1.2.11")


def test_every_case_has_a_golden_and_a_unique_name():
    names = [c[0] for c in cases.all_cases()]
    assert len(names) == len(set(names))
    assert sorted(names) == sorted(cases.golden())


@zlib_1_2_11
def test_generator_check_passes():
    r = subprocess.run([sys.executable, GEN, "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_generator_refuses_another_zlib():
    src = open(GEN).read()
    assert 'WANT_ZLIB = "1.2.11"' in src and "ZLIB_RUNTIME_VERSION != WANT_ZLIB" in src


@zlib_1_2_11
def test_filtered_differs_from_strategy_0_on_the_text_cases():
    for level in cases.FILT_LEVELS:
        for c in cases.filtered_cases(level):
            assert cases.yardstick(c) != cases.compress(c[1], level, c[3], 0), c[0]


@zlib_1_2_11
def test_filtered_is_strategy_0_for_deflate_fast():
    for level in (1, 2, 3):
        for c in cases.filtered_fast_cases(level):
            assert cases.yardstick(c) == cases.compress(c[1], level, c[3], 0), c[0]


@zlib_1_2_11
def test_fixed_differs_from_strategy_0_on_text_and_keeps_stored_blocks():
    for level in cases.FIXED_LEVELS:
        by = {c[0].rsplit("/", 1)[1]: c for c in cases.fixed_cases("deflate-raw", level)}
        assert cases.yardstick(by["text20000"]) != cases.compress(by["text20000"][1], level, "deflate-raw", 0)
        z = cases.yardstick(by["text20000"])
        assert z[0] & 6 == 2  # BTYPE 01
        r = cases.yardstick(by["rand20000"])
        assert r[0] & 6 == 0 and len(r) == 20000 + 5 * 2  # stored: the 16,383-symbol block and the rest


@zlib_1_2_11
def test_zlibs_rle_differs_from_the_references_on_the_run_cases():
    differ = 0
    for a, b in zip(cases.rle_cases("deflate-raw", 6, 0), cases.rle_cases("deflate-raw", 6, 1)):
        name = a[0].split("/")[3]
        same = cases.yardstick(a) == cases.yardstick(b)
        has_match = any(cases.runs((v, 4)) in a[1] for v in set(a[1]))  # four equal bytes: a match of three
        assert same != has_match, name
        differ += not same
    assert differ >= 70


@zlib_1_2_11
def test_the_wrapper_bits_follow_the_strategy():
    x = cases.huff_inputs()[4][1]
    for level in cases.HUFF_LEVELS:
        for strategy in (cases.Z_HUFFMAN_ONLY, cases.Z_RLE, cases.Z_FIXED):
            z = cases.compress(x, level, "deflate", strategy)
            assert z[0] == 0x78 and z[1] >> 6 == 0  # deflate.ts:757
            g = cases.compress(x, level, "gzip", strategy)
            assert g[8] == (2 if level == 9 else 4) and g[9] == 0xff  # deflate.ts:798: level 9 is tested first
        assert cases.compress(x, level, "deflate", cases.Z_FILTERED)[1] >> 6 == {1: 0, 6: 2, 9: 3}[level]
