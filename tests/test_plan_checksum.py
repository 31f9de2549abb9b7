"""CPU check of what csrc/zs_plan.h decides about a batch's data checksum (zs_plan_checksum and the
values of options "checksum_split" / "checksum_part", which capi.cpp runs before it launches
anything): tools/emu/emu_plan_checksum.cpp, plain g++, no ROCm headers.  The deflate plan beside
it must stay what the header planned before the options existed: the figures test_plan_params.py
pins as BEFORE."""
import os
import shutil
import subprocess

import pytest

from test_plan_params import BEFORE, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_checksum.cpp")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_checksum")
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


def unsplit(p):
    return (p["split"], p["parts"], p["ws"], p["map"], p["npfirst"], p["npstream"]) == ("0", "0", "0", "0", "0", "0")


def test_the_deflate_plan_is_what_the_header_planned_before(plans):
    for name, want in BEFORE.items():
        assert plans[name] == fields(want), name
        assert plans[name.replace("default", "small")] == fields(want), name  # whatever the two options say


def test_defaults_leave_the_benchmark_and_golden_batches_unsplit(plans):
    assert plans["defaults"] == {"split": str(1 << 18), "part": "65536"}
    assert unsplit(plans["default/256k"])  # 4,096 x 256 KiB: the largest streams of bench.py and the golden tests
    assert unsplit(plans["default/empty_batch"])


def test_a_length_at_the_threshold_stays_unsplit_and_one_past_it_splits(plans):
    assert unsplit(plans["default/at_split"])
    p = plans["default/past_split"]
    assert (p["split"], p["part_lg"], p["ok"]) == ("1", "16", "1")
    assert ints(p["pfirst"]) == [0, 1, 6, 7]  # 100 bytes: one part; 256 KiB + 1: five; an empty stream: one
    assert ints(p["pstream"]) == [0] + [1] * 5 + [2]
    assert (int(p["parts"]), int(p["ws"])) == (7, 4 * 7)
    assert unsplit(plans["p1024/below"])  # 4096 with split 4096
    assert plans["p1024/map"]["split"] == "1"  # 4097


def test_the_part_map(plans):
    """bounds 0, 1, part, part + 1, 3 part: 1, 1, 1, 2, 3 parts"""
    p = plans["p1024/issue"]
    assert (p["split"], p["part_lg"], p["parts"], p["ok"]) == ("1", "10", "8", "1")
    assert ints(p["pfirst"]) == [0, 1, 2, 3, 5, 8]
    assert ints(p["pstream"]) == [0, 1, 2, 3, 3, 4, 4, 4]
    assert int(p["ws"]) == 4 * 8
    # behind a metadata block: pfirst, then pstream at the next multiple of 256
    assert (int(p["pstream_at"]), int(p["map"])) == (256, 512)
    q = plans["p1024/map"]
    assert ints(q["pfirst"]) == [0, 1, 2, 3, 5, 8, 13] and ints(q["pstream"])[8:] == [5] * 5


def test_a_stream_of_4_gib_has_65536_parts_of_64_kib(plans):
    p = plans["default/4g"]
    assert (p["split"], p["parts"], p["npstream"], p["npfirst"], p["ok"]) == ("1", "65536", "65536", "2", "1")
    assert int(p["ws"]) == 4 * 65536 and int(p["map"]) == 256 + 4 * 65536
    q = plans["p1m/4g"]
    assert (q["parts"], q["part_lg"]) == ("4097", "20")  # 4,096 parts of 1 MiB, and one for the stream of 2 bytes


def test_checksum_split_0_never_splits(plans):
    assert unsplit(plans["p1024/never"])


def test_more_parts_than_one_launch_takes_is_one_wave_per_stream(plans):
    assert plans["p1024/most"]["parts"] == str(1 << 24) and plans["p1024/most"]["ok"] == "1"
    assert unsplit(plans["p1024/too_many"])


def test_option_values(plans):
    ok = lambda kind, v: plans["opt/%s/%d" % (kind, v)]["ok"] == "1"
    assert [ok("split", v) for v in (-1, 0, 1, 4096, 1 << 20, 0x7fffffff)] == [False, True, True, True, True, True]
    good = {1024, 65536, 1 << 20}
    for v in (-1024, -1, 0, 1, 512, 1023, 1024, 1025, 3072, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 21, 0x40000000):
        assert ok("part", v) == (v in good), v
