"""CPU check of the routes of a batch with preset dictionaries (csrc/zs_plan.h)
and of the host entries' dictionary layout (csrc/zs_dict.h: the distinct
dictionaries, their packed staging): tools/emu/emu_plan_dict.cpp, plain g++, no
ROCm headers.  The expected values follow from the routing rules: a dictionary
member is single-call (input <= 32,768 bytes, capacity <= 65,536) and decodes in
the dictionary lane instances, or it goes straight to the exact kernel; none goes
to the segmented, split or wave decoders; members without a dictionary keep the
routes the same batch gives them without dictionaries.  The program also runs
built with AddressSanitizer and UBSan (stand-alone, nothing preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_dict.cpp")


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
    tmp = tmp_path_factory.mktemp("emu_dict")
    plain = build_and_run(tmp, "emu_plan_dict", ["-O2"])
    san = build_and_run(tmp, "emu_plan_dict_san",
                        ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    return plain, san


@pytest.fixture(scope="module")
def plans(outputs):
    return parse(outputs[0])


def has(case, **want):
    got = {k: case.get(k) for k in want}
    assert got == {k: str(v) for k, v in want.items()}, case["case"]


def test_sanitized_build_prints_the_same(outputs):
    assert outputs[0] == outputs[1] and len(outputs[0].splitlines()) == 12


def test_single_call_members_take_the_dictionary_lane(plans):
    has(plans["shared64"], dict=1, dict_lane="0-63", dict_exact="-", seg="-", split="-", wave="-", wave_min=0)
    has(plans["large_batch"], dict=1, dict_lane="0-65535", dict_exact="-", seg="-", split="-", wave="-", lane_block=64,
        lane_rt=0)


def test_a_40000_byte_input_goes_to_the_exact_kernel(plans):
    # without a dictionary this small batch's 40,000-byte member is segmented
    has(plans["in40000"], dict_lane="0,2", dict_exact=1, seg="-", split="-", wave="-", nodict_seg=1)


def test_single_call_limits(plans):
    # 32,768 / 65,536 are single-call; one more byte of input or four more of capacity is not
    has(plans["edges"], dict_lane="0,3", dict_exact="1-2", seg="-", split="-", wave="-", nodict_seg="0-2")


def test_mixed_batch_members_without_a_dictionary_keep_their_routes(plans):
    c = plans["mixed_small"]
    has(c, dict_lane="0,7", dict_exact="2,4", seg="1,3", split="-", wave=5, wave_min=4096, lane_rt=2)
    # the same batch without dictionaries: the dictionary members' former routes
    has(c, nodict_seg="0-3", nodict_wave="4-5", nodict_lane_block=c["lane_block"])
    has(plans["mixed_nowrap"], dict_lane="-", dict_exact="0,2", seg="-", split=1, wave="-", nodict_seg=2,
        nodict_split="0-1")
    has(plans["mixed_noseg"], dict_lane=2, dict_exact=0, seg="-", split="-", wave=1, nodict_wave="0-1")


def test_no_dictionary_member_reaches_seg_split_or_wave(plans):
    def expand(r):
        out = set()
        for part in ([] if r == "-" else r.split(",")):
            a, _, b = part.partition("-")
            out |= set(range(int(a), int(b or a) + 1))
        return out

    for name, c in plans.items():
        if "dict_lane" not in c:
            continue
        d = expand(c["dict_lane"]) | expand(c["dict_exact"])
        assert not d & (expand(c["seg"]) | expand(c["split"]) | expand(c["wave"])), name
        assert not expand(c["dict_lane"]) & expand(c["dict_exact"]), name


def test_all_zero_lengths_plan_as_no_dictionaries(plans):
    has(plans["all_zero"], dict=0, dict_lane="-", dict_exact="-", seg=0, nodict_seg=0)


def test_distinct_dictionaries_and_packed_staging(plans):
    has(plans["one_shared"], any=1, distinct=1, total=1000, same=1, id="0,0,0,0,0", poff="0,0,0,0,0")
    # sorted by (offset, length): (1,10) (11,299) (11,300); members without one: id 0, offset 0
    has(plans["three_aliased"], any=1, distinct=3, total=609, same=1, id="0,0,2,0,1,2,0", poff="0,0,309,0,10,309,0")
    has(plans["none"], any=0, distinct=1, total=0, same=1)
    has(plans["overlapping"], any=1, distinct=3, total=28, same=1, id="0,2,1", poff="0,20,8")
