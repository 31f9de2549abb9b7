"""CPU check of what csrc/zs_plan.h decides for a batch with primed pieces (zs_deflate_make_req_primed,
zs_deflate_validate*, zs_plan_flush, zs_plan_primed, zs_plan_deflate over the segments with dict_len =
lp, which capi.cpp runs before it launches anything): tools/emu/emu_plan_primed.cpp, plain g++, no
ROCm headers.  A batch without points must plan exactly what the header planned for the _ex call:
the figures test_plan_params.py pins as BEFORE."""
import os
import shutil
import subprocess

import pytest

from test_plan_params import BEFORE, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_primed.cpp")
# zs_deflate_err
OK, WBITS, LEVEL, ALIGN = 0, 1, 2, 13
FLUSH_ARRAYS, FLUSH_POS, FLUSH_LEVEL0, FLUSH_MANY = 17, 18, 19, 20
VAR_PLAIN, VAR_DICT = 0, 2  # zs_variant


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_primed")
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


def test_a_call_without_points_plans_the_ex_call_field_for_field(plans):
    for name, want in BEFORE.items():
        assert plans[name.replace("default", "noprimed")] == fields(want), name
        req = plans[name.replace("default", "noprimed_req")]
        assert (req["made"], req["valid"], req["any"], req["same_req"]) == ("0", "0", "0", "1"), name
        assert (int(req["dict"]), int(req["variant"])) == (0, VAR_PLAIN), name  # no DICT instance, no start section


def seg(plans, name):
    p = plans["seg/" + name]
    assert p["ok"] == "1" and p["fits"] == "1", name
    assert (int(p["dict"]), int(p["variant"])) == (1, VAR_DICT), name  # the DICT instances, with d_start
    assert ints(p["start"]) == ints(p["lp"]), name                     # the parse starts behind the prime
    assert ints(p["nv"]) == [a + b for a, b in zip(ints(p["lp"]), ints(p["slen"]))], name
    assert ints(p["joff"]) == [a - b for a, b in zip(ints(p["soff"]), ints(p["lp"]))], name
    return p


def test_the_first_segment_of_every_stream_is_planned_as_the_plain_stream(plans):
    for name in ("one", "short_primes", "saturate", "window", "long", "long_l1", "ends"):
        assert seg(plans, name)["first_plain"] == "1", name


def test_one_point(plans):
    p = seg(plans, "one")
    assert (p["M"], ints(p["sfirst"])) == ("2", [0, 2])
    assert (ints(p["soff"]), ints(p["slen"]), ints(p["lp"]), ints(p["nv"])) == ([0, 40], [40, 60], [0, 40], [40, 100])
    assert ints(p["joff"]) == [0, 0]
    assert ints(p["pos"]) == [0, 40]  # the per-position tables follow nv ...
    assert ints(p["blk"]) == [0, 3]   # ... the block records slen (and the marker's slot)
    assert ints(p["win_olo"]) == [0, 40]  # the second piece's window owns the positions behind its prime


def test_primes_of_1_2_3_and_258_bytes(plans):
    p = seg(plans, "short_primes")
    assert ints(p["lp"]) == [0, 1, 2, 3, 258] and ints(p["nv"]) == [1, 2, 3, 258, 70000]
    assert ints(p["joff"]) == [0] * 5
    assert ints(p["win_s"]) == [0, 1, 2, 3, 4, 4] and ints(p["win_olo"]) == [0, 1, 2, 3, 258, 32768]
    assert p["max_len"] == "70000"


def test_the_prime_saturates_at_32768(plans):
    p = seg(plans, "saturate")
    assert ints(p["soff"])[1::2] == [32767, 32768, 32769] and ints(p["lp"])[1::2] == [32767, 32768, 32768]
    assert ints(p["joff"])[1::2] == [0, 0, 1] and ints(p["nv"])[1::2] == [70000, 70000, 69999]


def test_nv_around_the_one_window_length(plans):
    """a full prime and a piece of 32,768 / 32,769 bytes is one sweep window (nv <= 65,537), 32,770 two"""
    p = seg(plans, "window")
    assert ints(p["nv"]) == [32768, 65536, 32768, 65537, 32768, 65538]
    assert ints(p["win_s"]) == [0, 1, 2, 3, 4, 5, 5]
    assert ints(p["win_olo"]) == [0, 32768, 0, 32768, 0, 32768, 32768] and ints(p["win_base"])[-2:] == [0, 32752]


def test_pieces_of_131072_bytes_with_a_full_prime_take_five_windows(plans):
    p = seg(plans, "long")
    assert ints(p["slen"]) == [131072, 131072, 131072, 6784] and ints(p["lp"]) == [0, 32768, 32768, 32768]
    assert ints(p["joff"]) == [0, 98304, 229376, 360448] and ints(p["nv"]) == [131072, 163840, 163840, 39552]
    assert ints(p["pos"]) == [0, 131072, 294912, 458752] and p["max_len"] == "163840"
    assert ints(p["win_s"]) == [0] * 4 + [1] * 5 + [2] * 5 + [3]
    assert ints(p["blk"]) == [0, 11, 22, 33]  # 131,072 // 16,383 + 3 each: the records follow the piece, not J
    q = seg(plans, "long_l1")
    assert q["nwin"] == "0" and ints(q["blk"]) == ints(p["blk"]) and ints(q["pos"]) == ints(p["pos"])


def test_points_at_the_ends(plans):
    """a point at 0 (no prime either side), an empty last piece behind a prime"""
    p = seg(plans, "ends")
    assert ints(p["sfirst"]) == [0, 2, 5, 7]
    assert ints(p["slen"]) == [0, 0, 0, 3, 0, 40000, 0] and ints(p["lp"]) == [0, 0, 0, 0, 3, 0, 32768]
    assert ints(p["nv"]) == [0, 0, 0, 3, 3, 40000, 32768] and ints(p["joff"])[-1] == 40000 - 32768


def test_the_refusals_are_the_flush_entries(plans):
    def r(name):
        p = plans["refuse/" + name]
        return int(p["made"]), int(p["device"]), int(p["host"])

    for name in ("ok", "gzip", "zlib"):  # all three formats
        assert r(name) == (OK, OK, OK), name
    assert r("wbits") == (OK, WBITS, WBITS) and r("level") == (OK, LEVEL, LEVEL)
    assert r("align") == (OK, ALIGN, FLUSH_POS)
    assert r("null_first") == (OK, FLUSH_ARRAYS, FLUSH_ARRAYS) and r("null_pos") == (OK, FLUSH_ARRAYS, FLUSH_ARRAYS)
    assert r("null_pos_no_points") == (OK, OK, OK)
    for name in ("equal", "decreasing", "past_end"):
        assert r(name) == (OK, FLUSH_POS, FLUSH_POS), name
    assert r("level0") == (OK, FLUSH_LEVEL0, FLUSH_LEVEL0) and r("level0_no_points") == (OK, OK, OK)
    assert r("many") == (OK, FLUSH_MANY, FLUSH_MANY) and r("many_fits") == (OK, OK, OK)
    assert r("empty_batch") == (OK, OK, OK)
