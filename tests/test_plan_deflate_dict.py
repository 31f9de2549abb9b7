"""CPU check of the plan of a deflate batch with preset dictionaries (csrc/zs_plan.h,
zs_plan_deflate's dict_len): tools/emu/emu_plan_deflate_dict.cpp, plain g++, no
ROCm headers.  A stream with a dictionary is planned as its joined stream -- the
dictionary's last L' = min(L, 32768) bytes, then the n data bytes: the
per-position tables and the sweep's windows are those of a plain stream of
nv = L' + n bytes, but for the first window's own range, which starts at L'; the
block records follow n.  The program also runs built with AddressSanitizer and
UBSan (stand-alone, nothing preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_deflate_dict.cpp")


def build_and_run(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def parse(text):
    out = {}
    for line in text.splitlines():
        kv = dict(f.split("=", 1) for f in line.split())
        out[kv["case"]] = kv
    return out


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("emu_deflate_dict")
    plain = build_and_run(tmp, "emu_plan_deflate_dict", ["-O2"])
    san = build_and_run(tmp, "emu_plan_deflate_dict_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    return plain, san


@pytest.fixture(scope="module")
def plans(outputs):
    return parse(outputs[0])


def has(case, **want):
    got = {k: case.get(k) for k in want}
    assert got == {k: str(v) for k, v in want.items()}, case["case"]


def test_sanitized_build_prints_the_same(outputs):
    assert outputs[0] == outputs[1] and len(outputs[0].splitlines()) == 10


def test_all_zero_lengths_plan_as_today(plans):
    # (every case: the same lengths with every dict_len 0 against the plan without the argument)
    for name, c in plans.items():
        has(c, zero_same=1)
    has(plans["all_zero"], start="0,0,0", wins="0:0:0:100,1:0:0:65520,1:32752:32768:65520,2:0:0:0", B=10, B_joined=10)


def test_a_small_record_is_one_window_owning_the_data(plans):
    has(plans["small"], nwin=1, wins="0:0:32768:32868", start=32768, max_len=32868, P=32872, J=32880)


def test_65538_joined_bytes_take_the_multi_window_path(plans):
    has(plans["one_window_edge"], nwin=1, wins="0:0:32768:65537")
    has(plans["multi"], nwin=2, wins="0:0:32768:65520,0:32752:32768:65520", max_len=65538)


def test_only_the_last_32768_bytes_of_a_dictionary_count(plans):
    has(plans["tail"], start=32768, max_len=232769, nwin=7,
        wins="0:0:32768:65520,0:32752:32768:65520,0:65504:32768:65520,0:98256:32768:65520")


def test_tables_follow_nv_and_blocks_follow_n(plans):
    for name, c in plans.items():
        has(c, tables_joined=1, wins_as_joined=1, blk_same=1, P=c["P_joined"], members=c["members_joined"],
            nwin=c["nwin_joined"], B=c["B_plain"], max_blk=c["max_blk_plain"])
    has(plans["tail"], B=14, B_joined=16)          # 200001 / 16383 + 2, not 232769 / 16383 + 2
    has(plans["blocks"], B=12, B_joined=16, max_blk=5)
    has(plans["empty_data"], B=4, wins="0:0:32768:32768,1:0:1:1")


def test_mixed_batch(plans):
    has(plans["mixed"], start="0,257,0,32767", joff="0,112,5376,70928",
        wins="0:0:0:100,1:0:257:5257,2:0:0:65520,2:32752:32768:65520", nwin=7)


def test_levels_1_to_3_and_the_chain_walk_have_no_windows(plans):
    for name in ("level1", "nosweep"):
        has(plans[name], nwin=0, members=0, start="32768,32768", max_len=232769, B=16)
