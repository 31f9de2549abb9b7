"""CPU check of what csrc/zs_plan.h decides about whole deflate calls (zs_deflate_req,
zs_deflate_validate, zs_plan_deflate, zs_meta_layout): tools/emu/emu_plan_launch.cpp,
plain g++, no ROCm headers.

plan_launch_trace.txt and plan_launch_faults.txt were recorded from the host layer as it
was before the request / plan / launch split: its deflate_device, deflate_launch,
deflate_stored_batch and entry points compiled with every kernel launch replaced by a
print of the instance and its launch configuration and the HIP calls stubbed, run over
tools/emu/emu_plan_launch_cases.h.  The metadata offsets are recomputed here from that
layer's rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_launch.cpp")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_launch")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    return run


def cases(text):
    """case name -> its lines"""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("case="):
            cur = out.setdefault(line[5:], [])
        else:
            cur.append(line.strip())
    return out


def test_launch_traces_are_the_recorded_ones(emu):
    want = cases(open(os.path.join(HERE, "plan_launch_trace.txt")).read())
    got = cases(emu())
    assert list(got) == list(want) and len(want) == 486
    for name in want:
        assert got[name] == want[name], name
    # the table covers what it is meant to
    kernels = {l.split()[0] for lines in want.values() for l in lines}
    for k in ("zs_k_stored", "zs_k_huff_tally", "zs_k_rle_tally", "zs_k_bucket<0>", "zs_k_bucket<1>", "zs_k_sweep<0>",
              "zs_k_sweep<1>", "zs_k_prev<0>", "zs_k_prev_par<1>", "zs_k_match", "zs_k_match_par", "zs_k_parse",
              "zs_k_parse_2w", "zs_k_parse_2w_filt", "zs_k_parse_2w_dict", "zs_k_parse_2w_par", "zs_k_fast<2,1,0>",
              "zs_k_fast<2,0,1>", "zs_k_fast<4,0,0>", "zs_k_fast<4,1,1>", "zs_k_fast<8,1,1>", "zs_k_fast_serial<0>", "zs_k_fast_serial<1>",
              "zs_k_fast_par<2,1,0>", "zs_k_fast_par<8,0,0>", "zs_k_fast_serial_par<0,0>", "zs_k_fast_serial_par<0,1>",
              "zs_k_trees_par", "zs_k_layout_dict", "zs_k_wrap", "zs_k_wrap_par", "zs_k_wrap_dict", "zs_k_dict_join"):
        assert k in kernels, k
    # a dictionary entry whose lengths are all 0 launches what the plain entry does
    for level in range(1, 10):
        for w in (0, 1):
            assert got["dict0/l%d/w%d/opts7" % (level, w)] == got["plain/l%d/w%d" % (level, w)]


def test_default_parameters_take_163840_bytes_of_lds_on_both_fast_routes(emu):
    got = cases(emu())
    seen = set()
    for level in (1, 2, 3):
        for group in (0, 1):
            for name in ("opts/l%d/sweep1/group%d/order1" % (level, group),
                         "params15_8/l%d/group%d_order1/w1" % (level, group),
                         "dict1/l1/w1/opts%d" % (5 + 2 * group)):
                fast = [l for l in got[name] if l.startswith("zs_k_fast")]
                assert len(fast) == 1 and fast[0].endswith(" lds=163840"), (name, fast)
                seen.add(fast[0].split("<")[0])
    assert seen == {"zs_k_fast", "zs_k_fast_serial"}  # (15 / memLevel 8 is the default: no *_par instance)


def up256(x):
    return (x + 255) & ~255


def test_metadata_layout(emu):
    rows = {}
    for line in emu("layout").splitlines():
        kv = dict(f.split("=", 1) for f in line.split())
        name = kv.pop("case")
        rows[name] = {k: int(v) for k, v in kv.items()}
    grid = [r for name, r in rows.items() if not name.startswith("plan/")]
    assert len(grid) == 3 * 3 * 2 * 2
    assert {(r["n"], r["ndict"], r["nchunks"] != 0, r["nwin"] != 0) for r in grid} == {
        (n, d, c, w) for n in (1, 3, 257) for d in (0, 1, 2) for c in (False, True) for w in (False, True)}
    for r in grid:
        n, nu = r["n"], r["ndict"]
        # the sections in order, each rounded up to 256 bytes; the dictionary sections only with
        # dictionaries; the Huffman chunk list (8 bytes per chunk) last
        sections = [("in_off", 8 * n), ("in_len", 4 * n), ("out_off", 8 * n), ("out_cap", 4 * n), ("pos_base", 8 * n),
                    ("blk_base", 4 * n), ("segs", 32 * r["nwin"])]
        dict_sections = [("doff", 8 * n), ("dlen", 4 * n), ("did", 4 * n), ("start", 4 * n), ("joff", 8 * n),
                         ("jlen", 4 * n), ("uoff", 8 * nu), ("ulen", 4 * nu)]
        o = 0
        for name, size in sections:
            assert r[name] == o, (r, name)
            o += up256(size)
        first_seven = o
        if nu:
            for name, size in dict_sections:
                assert r[name] == o, (r, name)
                o += up256(size)
        else:
            assert r["chunks"] == first_seven  # the dictionary sections take no room
        assert r["chunks"] == o
        assert r["bytes"] == o + up256(8 * r["nchunks"])
    # ... and as the plan fills it in
    d, h = rows["plan/dict"], rows["plan/huff"]
    assert (d["dict"], d["ndict"], d["nwin"], d["nchunks"]) == (1, 2, 4, 0) and d["bytes"] == d["chunks"] == d["ulen"] + 256
    assert (h["dict"], h["nwin"], h["nchunks"]) == (0, 0, 7) and h["bytes"] == h["chunks"] + 256 and h["chunks"] == 6 * 256


def test_the_fault_that_wins(emu):
    want = [l.split() for l in open(os.path.join(HERE, "plan_launch_faults.txt")).read().splitlines()]
    got = [l.split() for l in emu("faults").splitlines()]
    assert len(want) == 104 and [w[0] for w in want] == [g[0] for g in got]
    for w, g in zip(want, got):
        assert g == w, w[0]
    verdict = {w[0][5:]: w[1][6:] for w in want}
    # the order read off the entries, spelled out for a few calls with several faults
    assert verdict["level+null_ctx/device"] == "null_context"
    assert verdict["strategy+null_ctx/host"] == "strategy"
    assert verdict["window_bits+mem_level+null_ctx/device"] == "window_bits"
    assert verdict["empty+level/device"] == "level" and verdict["empty+level/host"] == "ok"
    assert verdict["params_level0+align/device"] == "align"
    assert verdict["dict_level0+wbits/device"] == "wbits" and verdict["dict_level0+wbits/host"] == "dict_level0"
    assert verdict["dict_gzip+level/device"] == "level" and verdict["dict_gzip+level/host"] == "dict_gzip"
    assert verdict["empty+dict_arrays/device"] == "ok" and verdict["empty+dict_arrays/host"] == "dict_arrays"
    assert verdict["dict_long+align/device"] == "dict_long"
    assert verdict["rle_long+align/device"] == "align"


def test_a_dictionary_with_a_strategy_or_parameters_is_refused_not_dropped(emu):
    # (no public entry makes such a request; the emulator builds the two by hand)
    assert emu("combined").split() == ["strategy=dict_combined", "params=dict_combined", "plain=ok"]
