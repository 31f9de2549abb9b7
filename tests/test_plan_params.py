"""CPU check of what csrc/zs_plan.h decides for deflateInit2_'s windowBits and memLevel
(zs_make_params, zs_plan_deflate, zs_plan_fast_params, which capi.cpp runs before it launches
anything): tools/emu/emu_plan_params.cpp, plain g++, no ROCm headers.  The default
parameters must plan exactly what the header planned before the parameters existed: the
figures in BEFORE are that header's (the emulator built with -DEMU_PLAN_BEFORE against it),
for streams of 0, 1, 100, 16383, 65537, 65538 and 200000 bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_params.cpp")
GROUP, SERIAL, SERIAL_GHEAD = 0, 1, 2  # zs_fast_route
LENS = [0, 1, 100, 16383, 65537, 65538, 200000]

BEFORE = {
    "default/s0/l1": "P=347584 members=0 B=35 max_len=200000 max_blk=14 pw=1 nseg=0 prevd=695296 mres=2780736 "
                     "syms=1390428 pscr=0 codes=44240 hdr=22400 pos=29268240 blk=61140267 seg=0",
    "default/s0/l6": "P=347584 members=0 B=35 max_len=200000 max_blk=14 pw=2 nseg=0 prevd=695296 mres=2780736 "
                     "syms=1390428 pscr=5652640 codes=44240 hdr=22400 pos=29268240 blk=61140267 seg=0",
    "default/s1/l1": "P=347584 members=0 B=35 max_len=200000 max_blk=14 pw=1 nseg=0 prevd=695296 mres=2780736 "
                     "syms=1390428 pscr=0 codes=44240 hdr=22400 pos=29268240 blk=61140267 seg=0",
    "default/s1/l6": "P=347584 members=871872 B=35 max_len=200000 max_blk=14 pw=2 nseg=13 prevd=1743872 mres=2780736 "
                     "syms=1390428 pscr=5652640 codes=44240 hdr=22400 pos=29268240 blk=61140267 seg=4584240420124748605",
}


def fields(text):
    return dict(f.split("=", 1) for f in text.split())


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_params")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        kv = fields(line)
        out[kv.pop("case")] = kv
    return out


def test_default_parameters_plan_what_the_header_planned_before(plans):
    for name, want in BEFORE.items():
        assert plans[name] == fields(want), name
        assert plans[name.replace("default", "explicit")] == fields(want), name  # ... and through zs_make_params(15, 8)
    # the route: the sweep at levels 4..9 unless option match_sweep is off, as before
    assert [plans["route/default/s%d/l%d" % (s, l)]["sweep"] for s in (0, 1) for l in (1, 6)] == ["0", "0", "0", "1"]
    assert plans["w15/m8"]["default"] == "1" and plans["w15/m8"]["sweep"] == "1" and plans["w15/m8"]["nseg"] == "13"


def test_the_parameters_follow_deflateInit2(plans):
    shifts = [3, 3, 4, 4, 4, 5, 5, 5, 6]  # (hash_bits + 2) / 3 in whole numbers (deflate.ts:312-315, :110)
    for wb in range(8, 16):
        for ml in range(1, 10):
            p = plans["w%d/m%d" % (wb, ml)]
            assert int(p["w_bits"]) == max(wb, 9), (wb, ml)  # 8 runs as 9 (deflate.ts:295-297)
            assert int(p["hash_bits"]) == ml + 7 and int(p["hash_shift"]) == shifts[ml - 1], (wb, ml)
            assert 3 * int(p["hash_shift"]) >= int(p["hash_bits"])  # the closed-form hash holds
            assert int(p["sym_end"]) == (1 << (ml + 6)) - 1, (wb, ml)  # lit_bufsize - 1 (deflate.ts:323,336)
            assert int(p["default"]) == (1 if (wb, ml) == (15, 8) else 0), (wb, ml)


def test_non_default_parameters_take_the_chain_walk_route(plans):
    for wb in range(8, 16):
        for ml in range(1, 10):
            if (wb, ml) != (15, 8):
                p = plans["w%d/m%d" % (wb, ml)]
                assert (p["sweep"], p["nseg"]) == ("0", "0"), (wb, ml)  # zs_k_prev_par + zs_k_match_par, no windows


def test_block_counts_follow_lit_bufsize(plans):
    for ml in (1, 8, 9):
        sym_end = (1 << (ml + 6)) - 1
        per = [n // sym_end + 2 for n in LENS]
        for wb in (9, 15):
            p = plans["w%d/m%d" % (wb, ml)]
            assert int(p["B"]) == sum(per) and int(p["max_blk"]) == max(per), (wb, ml)
            assert int(p["codes"]) == 4 * (286 + 30) * sum(per) and int(p["hdr"]) == 4 * 160 * sum(per), (wb, ml)
            assert p["fits"] == "1"
    assert plans["w15/m1"]["max_blk"] == "1576"  # 200,000 bytes: 129 times memLevel 8's records ...
    assert plans["w15/m8"]["max_blk"] == "14" and plans["w15/m9"]["max_blk"] == "8"


def test_which_parameters_keep_the_fast_tables_in_lds(plans):
    for wb in range(8, 16):
        for ml in range(1, 10):
            p = plans["w%d/m%d" % (wb, ml)]
            w, head, prev = 1 << max(wb, 9), 2 << (ml + 7), 2 << max(wb, 9)
            # the group-speculative kernel (32 KiB ring) up to 15 hash bits; memLevel 9 runs step by step
            if ml <= 8:
                assert (int(p["group_route"]), int(p["group_lds"])) == (GROUP, head + prev + 32768), (wb, ml)
            else:
                assert int(p["group_route"]) == int(p["serial_route"]), (wb, ml)
            # the step-by-step kernel (ring of w bytes): head[] in LDS unless memLevel 9 meets w_bits 14, 15
            if ml == 9 and max(wb, 9) >= 14:
                assert (int(p["serial_route"]), int(p["serial_lds"])) == (SERIAL_GHEAD, prev + w), (wb, ml)
                assert int(p["ghead"]) == 131072 * len(LENS)
            else:
                assert (int(p["serial_route"]), int(p["serial_lds"])) == (SERIAL, head + prev + w), (wb, ml)
                assert int(p["ghead"]) == 0
            assert int(p["group_lds"]) <= 160 << 10 and int(p["serial_lds"]) <= 160 << 10, (wb, ml)


def test_windowbits_argument(plans):
    ok = {-15: (15, 0), -9: (9, 0), 8: (8, 1), 9: (9, 1), 15: (15, 1), 25: (9, 2), 31: (15, 2)}
    for wbits in (-16, -15, -9, -8, -7, 0, 7, 8, 9, 15, 16, 23, 24, 25, 31, 32):
        p = plans["wbits/%d" % wbits]
        assert (int(p["window"]), int(p["wrap"])) == ok.get(wbits, (0, -1)), wbits
