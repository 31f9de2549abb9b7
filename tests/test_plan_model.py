"""CPU check of the host layer's decisions (csrc/zs_plan.h, which capi.cpp runs
before it launches anything): tools/emu/emu_plan.cpp, built with plain g++ and
no ROCm headers, prints the inflate, segmented and deflate plans of a fixed set
of batches, one line of key=value pairs per case.  The expected values here were
worked out by hand from the routing rules (thresholds, scratch bounds, instance
choices) at the defaults of every option and 256 compute units unless a case
says otherwise.  No GPU needed; the GPU suites pin the same routes through the
lane and segmented counts of real batches."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan.cpp")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan")
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


@pytest.mark.parametrize("n,block", [(512, 1), (4608, 1), (4609, 2), (8192, 2), (16384, 4), (16385, 16),
                                     (32768, 32), (65536, 64)])
def test_lane_block_follows_the_batch_size(plans, n, block):
    # root tables (instance 1 without large members beside the lanes) exactly when the block is <= 16
    has(plans["lane%d" % n], lane_block=block, lane_rt=1 if block <= 16 else 0, wave_min=0)


def test_lane_block_option_overrides_the_batch_size(plans):
    has(plans["lane8_512"], lane_block=8, lane_rt=1)
    has(plans["lane8_65536"], lane_block=8, lane_rt=1)
    has(plans["lane32_512"], lane_block=32, lane_rt=0)


def test_a_batch_over_seg_small_batch_keeps_inflate_wave_min(plans):
    # P1: 65,536 x 20,000 bytes: below inflate_wave_min, and n > seg_small_batch
    has(plans["P1"], seg="-", split="-", wave="-", wave_min=0, lane_block=64, lane_rt=0)


def test_small_batch_of_64k_members_is_segmented(plans):
    # P2: gzip, 8,192 x (20,000 / 65,536): the threshold is seg_small_min
    has(plans["P2"], seg="0-8191", split="-", wave="-", wave_min=4096, lane_block=2, lane_rt=2)
    has(plans["P2"], walk="0/1024/0", bits=2048, seg_split=0, big="-", nwalk=8192, resolve="256/32768", decode="0/1",
        slots0=42, pmax0=356, scr0=71248, slots=42 * 8192, pieces=356 * 8192, scr=71248 * 8192, gdec=8192, gfb=256)


def test_few_large_members_take_the_wide_window_and_split_pieces(plans):
    # P3: raw, 512 x (90,000 / 262,144): the walks fit the chip at once (3 per CU)
    has(plans["P3"], seg="0-511", wave_min=4096, lane_block=1, lane_rt=2)
    has(plans["P3"], walk="0/2048/1", bits=4096, seg_split=1, resolve="512/65536", decode="0/1", slots0=144,
        pmax0=1552, scr0=286992, nwalk=512)
    has(plans["P3_1024"], seg="0-1023", walk="0/1024/1", bits=4096, seg_split=0, resolve="256/32768", nwalk=1024)


def test_expanding_members_split_up_to_the_scratch_bound(plans):
    # P4: raw, 16 x (1,000 / 1,048,576): long copies, never segmented
    has(plans["P4"], seg="-", split="-", wave="0-15", wave_refw=1, wave_lanes=0, wave_min=4096)
    # without the window-wrap copy they split: 138,412,032 scratch bytes each, 15 fit 2 GiB
    assert (2 * 64 + 4) * 1048576 == 138412032 and 15 * 138412032 <= 2 << 30 < 16 * 138412032
    has(plans["P4_nowrap"], seg="-", split="0-14", wave="15", wave_refw=0, piece_cap=1048576, val_stride=1048576)


def test_deflate64_members_segment_or_split_by_input_bits(plans):
    # P5: members of more than ZS_SEG_SPLIT_BITS (2^18) input bits split
    has(plans["P5"], seg="0,2", split="1,3", wave="-", piece_cap=65536, val_stride=65536)
    has(plans["P5"], walk="1/1024/0", decode="1/0", slots0=58, pmax0=528, scr0=74000, slots=116, pieces=1056,
        scr=148000, gdec=116, gfb=2)


def test_many_large_members_without_the_segmented_decode_run_as_lanes(plans):
    # P6: zlib, 4,096 x (100,000 / 262,144), inflate_seg = 0
    has(plans["P6"], seg="-", split="-", wave="0-4095", wave_min=32768, wave_lanes=1, wave_block=1, wave_rt=2,
        wave_refw=1)
    has(plans["P6_nolanes"], wave="0-4095", wave_lanes=0, wave_refw=1)


def test_segmented_scratch_is_bounded(plans):
    # P7: 1 MiB of scratch holds seven members of 142,496 bytes
    assert 7 * 142496 <= 1 << 20 < 8 * 142496
    has(plans["P7"], seg="0-6", split="-", wave="7-15", scr0=71248, gfb=7)


def test_big_members_walk_from_the_finders_block_starts(plans):
    # P8: 2,400,000 input bits > 2^21
    has(plans["P8"], seg="0-1", big="0-1", nwalk=2 + 2 * 63)


def test_deflate_layout_of_a_short_and_a_two_window_stream(plans):
    d = plans["D1"]  # [100, 65,538] at level 6
    has(d, pos="0,104", P=65648, win0="0,1,3", nwin=3, members=65648 + 2 * 65536, blk="0,2", max_len=65538, max_blk=6)
    # (65,538 // 16,383 + 2 = 6 blocks for the second stream: 8 in all)
    has(d, B=8)
    has(d, wins="0:0:0:100:0,1:0:0:65520:65648,1:32752:32768:65520:131184")
    has(d, prevd=2 * 196720 + 128, mres=8 * 65648 + 64, syms=4 * (65648 + 2) + 64,
        pscr=4 * 2060 * (65648 // 512 + 3), codes=4 * 316 * 8, hdr=4 * 160 * 8)
    # without the sweep (option, or levels 1..3): no windows, no members beyond the positions
    has(plans["D1_nosweep"], nwin=0, members=0, prevd=2 * 65648 + 128, pw=2)
    has(plans["D1_L1"], nwin=0, members=0, pw=1, pscr=0)


def test_window_counts_of_single_streams(plans):
    has(plans["D_65537"], nwin=1, win0="0,1", wins="0:0:0:65537:0")
    has(plans["D_200000"], nwin=6, win0="0,6", members=200000 + 6 * 65536)


def test_parse_waves(plans):
    has(plans["PW_2047"], pw=2)
    has(plans["PW_2048"], pw=1)
    for w in (1, 2, 4):
        has(plans["PW_opt%d_2047" % w], pw=w)
        has(plans["PW_opt%d_2048" % w], pw=w)
    # scratch per segment of 1024 / 512 / 256 positions
    has(plans["PW_2048"], pscr=4 * 3596 * (32768 // 1024 + 2049))
    has(plans["PW_opt2_2048"], pscr=4 * 2060 * (32768 // 512 + 2049))
    has(plans["PW_opt4_2048"], pscr=4 * 1292 * (32768 // 256 + 2049))


# ---- the routes tests/test_gpu_inflate_regions.py forces with options and asserts by count on the GPU: its batches'
# lengths (14 large members of 11,640 .. 102,571 input bytes at indices 0-13, four small ones behind them)
def test_region_batches_take_the_segmented_decode_and_its_small_batch_resolve(plans):
    # more than seg_small_min (4,096) input bytes: segmented; under 64 KiB of input on average: the 1,024-bit window,
    # 2,048-bit lanes, whole pieces
    has(plans["R_few"], seg="0-13", split="-", wave="-", wave_min=4096, lane_block=1, lane_rt=2, walk="0/1024/0",
        bits=2048, seg_split=0, nwalk=14, resolve="512/65536", decode="0/1")
    has(plans["R_few_split1"], seg="0-13", seg_split=1, resolve="512/65536")
    has(plans["R_few_bits"], seg="0-13", bits=1024, walk="0/1024/0")
    # 89,939 and 102,571 input bytes alone: the wide window, 4,096-bit lanes, pieces cut in two
    has(plans["R_wide"], seg="0-3", walk="0/2048/1", bits=4096, seg_split=1, resolve="512/65536")


def test_more_than_two_segmented_members_per_compute_unit_take_the_other_resolve(plans):
    # 520 > 2 x 256 members of 2,322 .. 24,960 input bytes, seg_small_min = 256
    for name in ("R520", "R520_gzip"):
        has(plans[name], seg="0-519", split="-", wave="-", wave_min=256, resolve="256/32768", nwalk=520, seg_split=0,
            walk="0/1024/0", bits=2048, lane_block=1, lane_rt=2, gfb=256)
    has(plans["R16"], seg="0-15", resolve="512/65536", nwalk=16, gfb=16)


def test_region_batches_without_the_segmented_decode(plans):
    # zlib / gzip, every member over one input byte large: the wave kernel, with and without the reference's calls
    has(plans["R_wave"], seg="-", split="-", wave="0-17", wave_min=1, wave_refw=1, wave_lanes=0)
    has(plans["R_wave_nowrap"], seg="-", split="-", wave="0-17", wave_refw=0, wave_lanes=0)
    # raw deflate without the window-wrap copy splits: 18 x (2 x 64 + 4) x 262,208 scratch bytes fit 2 GiB
    assert 18 * (2 * 64 + 4) * 262208 <= 2 << 30
    has(plans["R_split_raw"], seg="-", split="0-17", wave="-", piece_cap=262208, val_stride=262208)
    # members over 1,024 input bytes large: a wave each, or with lane_large_min = 1 a lane each
    has(plans["R_nolanes"], seg="-", split="-", wave="0-13,16-17", wave_min=1024, wave_refw=1, wave_lanes=0)
    has(plans["R_lanes"], seg="-", split="-", wave="0-13,16-17", wave_min=1024, wave_refw=1, wave_lanes=1, wave_block=1,
        wave_rt=2)


def test_expanding_members_leave_the_segmented_decode(plans):
    # a capacity past 64 KiB and 8 bytes of it per input byte: deflate64 splits, raw deflate takes the wave kernel
    # (the window-wrap copy) or splits (without it); the text member beside them is segmented
    has(plans["R_zeros64"], seg="2", split="0-1", wave="-", piece_cap=100064, val_stride=100064, decode="1/0")
    has(plans["R_zeros"], seg="2", split="-", wave="0-1", wave_refw=1, wave_lanes=0)
    has(plans["R_zeros_nowrap"], seg="2", split="0-1", wave="-", piece_cap=262148, val_stride=262148)
