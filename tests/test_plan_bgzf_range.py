"""CPU check of what csrc/zs_plan.h decides for a batch of BGZF ranges by virtual offset (zs_bgzf_range_validate,
zs_bgzf_range_slice, zs_plan_bgzf_range): tools/emu/emu_plan_bgzf_range.cpp, plain g++, no ROCm
headers, built once more as a stand-alone program with -fsanitize=address,undefined.  The records of the slices'
starts are read here from the headers of real files (bgzfrangecases.records); the plan is held against the
contract written out in Python (bgzfrangecases.plan)."""
import os
import shutil
import subprocess

import pytest

import bgzfrangecases as rc
from bgzfrangecases import voff
from test_plan_params import fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_plan_bgzf_range.cpp")
MEMBERS, EMPTY, CHAIN = 0, 1, 2
BIG = 0xfffffffc


def small():
    """five data blocks of 300 bytes (the last of 100) and the end-of-file block"""
    return rc.bc.bgzf(rc.text(1300, 3), 300)


def seventy():
    return rc.bc.bgzf(rc.text(70 * 64, 5), 64)


def all_cases():
    """{name: [(stream, cap, vb, ve)]}"""
    s, cases = small(), {}
    for name, (vb, ve) in rc.corners(s).items():
        cases["corner/" + name] = [(s, BIG, vb, ve)]
    s70 = seventy()
    cases["corner/70 blocks"] = [(s70, BIG, voff(0, 7), voff(rc.blocks(s70)[69][0], 9))]
    for name, ((vb, ve), _) in rc.header_failures(s).items():
        cases["fail/" + name] = [(s, BIG, vb, ve)]
    # the slack behind ce holds a block cut short by the stream's end, and behind a short last block a whole one
    b = rc.blocks(s)
    cut = s[:b[3][0] + 40]
    cases["slack/truncated"] = [(cut, BIG, voff(b[1][0], 2), voff(b[2][0], 7))]
    cases["slack/whole"] = [(s, BIG, voff(b[0][0], 2), voff(b[1][0], 7))]
    # the capacity cut at every member: the range over all five data blocks from byte 10 of the first
    vb, ve = voff(0, 10), voff(b[4][0], 50)
    total = rc.out_len(s, vb, ve)[1]
    for cap in (0, 289, 290, 589, 590, 889, 890, 1189, 1190, total - 1, total):
        cases["cap/%d" % cap] = [(s, cap, vb, ve)]
    # a batch: a failing stream between two good ones contributes no member
    cases["batch/mixed"] = [(s, BIG, voff(0, 1), voff(b[1][0], 1)), (s, BIG, voff(b[1][0] + 3, 0), voff(b[2][0], 0)),
                            (s, BIG, voff(b[2][0], 0), voff(b[2][0], 0)), (s70, BIG, 0, voff(len(s70), 0))]
    cases["refused/order"] = [(s, BIG, voff(b[1][0], 1), voff(b[1][0], 0))]
    cases["refused/past_end"] = [(s, BIG, 0, voff(len(s) + 1, 0))]
    return cases


def stdin_of(cases):
    lines = []
    for name, streams in cases.items():
        lines.append("case %s %d" % (name.replace(" ", "_"), len(streams)))
        for s, cap, vb, ve in streams:
            ok = vb <= ve and (ve >> 16) <= len(s)
            recs = rc.records(s, vb, ve) if ok else [(0, 3, 0, 0, 0)]
            lines.append("stream %d %d %d %d %d" % (len(s), cap, vb, ve, len(recs) - 1))
            lines += ["%d %d %d %d %d" % r for r in recs]
    return "\n".join(lines) + "\n"


def run(exe, cases):
    r = subprocess.run([exe], input=stdin_of(cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        kv = fields(line)
        out[kv.pop("case")] = kv
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emu") / "emu_plan_bgzf_range")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    return run(exe, all_cases())


def ints(t):
    return [] if t in ("-", "") else [int(x) for x in t.split(",")]


def check_stream(p, s, cap, vb, ve, name):
    """the plan of one stream against the contract"""
    how, mem = rc.plan(s, vb, ve)
    off, n = rc.slice_of(s, vb, ve)
    assert (int(p["slice_off"]), int(p["slice_len"])) == (off, n), name
    if how == "fail":
        assert (int(p["verdict"]), int(p["vcons"]), p["soff"]) == (CHAIN, mem, "-"), name
        return 0
    if not mem:
        assert (int(p["verdict"]), int(p["vcons"]), p["soff"]) == (EMPTY, vb >> 16, "-"), name
        return 0
    assert int(p["verdict"]) == MEMBERS, name
    out, want = 0, []
    for start, end, isize, skip, take in mem:
        fits = out + take <= cap
        want.append((start, end - start, isize if fits else 0, skip, take, out, int(fits)))
        if not fits:
            break
        out += take
    got = list(zip(*(ints(p[k]) for k in ("soff", "slen", "ocap", "skip", "take", "opos", "trusted"))))
    assert got == want, name
    st = ints(p["stoff"])
    assert all(x % 4 == 0 for x in st) and all(b - a >= w[2] for a, b, w in zip(st, st[1:], want)), name
    return len(want)


def test_every_corner_follows_the_contract(plans):
    for name, streams in all_cases().items():
        key = name.replace(" ", "_")
        if name.startswith("refused/"):
            continue
        M = sum(check_stream(plans["%s/%d" % (key, i)], *st, name) for i, st in enumerate(streams))
        assert int(plans[key]["M"]) == M and plans[key]["refused"] == "0", name
        # the place's tiles: one per 4,096 bytes of (delivered bytes + 3), none for the member capacity cuts
        pt = ints(plans[key]["ptile"])
        assert len(pt) == M + 1 and pt[0] == 0 and all(b >= a for a, b in zip(pt, pt[1:])), name


def test_the_corners_are_the_ones_meant(plans):
    s = small()
    b = rc.blocks(s)
    c = rc.corners(s)
    one = plans["corner/one_block,_cb_==_ce/0"]
    assert (ints(one["soff"]), ints(one["skip"]), ints(one["take"])) == ([b[1][0]], [0], [300])
    ub = plans["corner/ub_ISIZE/0"]
    assert (ints(ub["skip"]), ints(ub["take"]), ints(ub["opos"])) == ([300, 0], [0, 300], [0, 0])  # decoded, delivers nothing
    assert ints(plans["corner/ue_0/0"]["soff"]) == [b[1][0]]  # the block at ce is not decoded
    assert ints(plans["corner/ue_ISIZE/0"]["take"]) == [300, 300]
    eof = plans["corner/ce_==_in_len/0"]
    assert ints(eof["soff"])[-1] == b[-1][0] and ints(eof["take"])[-1] == 0 and int(eof["slice_len"]) == len(s) - b[1][0]
    assert ints(plans["corner/ce_at_the_end-of-file_block/0"]["soff"])[-1] == b[-2][0]
    for name in ("empty at a block", "empty at in_len"):
        p = plans["corner/%s/0" % name.replace(" ", "_")]
        assert (int(p["verdict"]), int(p["vcons"]), int(p["slice_len"])) == (EMPTY, c[name][0] >> 16, 0)
    assert len(ints(plans["corner/2_blocks/0"]["soff"])) == 2 and len(ints(plans["corner/3_blocks/0"]["soff"])) == 3
    p70 = plans["corner/70_blocks/0"]
    assert len(ints(p70["soff"])) == 70 and ints(p70["skip"])[0] == 7 and ints(p70["take"])[-1] == 9
    assert sum(ints(p70["take"])) == 70 * 64 - 7 - 64 + 9


def test_members_behind_the_needed_end_are_dropped(plans):
    s = small()
    b = rc.blocks(s)
    p = plans["slack/truncated/0"]  # the slice ends inside block 3, whose header cannot be trusted there
    assert ints(p["soff"]) == [b[1][0], b[2][0]] and ints(p["take"]) == [298, 7]
    p = plans["slack/whole/0"]  # the slice holds blocks 2 .. 5 and the end-of-file block behind the needed end
    assert int(p["slice_len"]) == len(s) and ints(p["soff"]) == [b[0][0], b[1][0]]


def test_the_capacity_cut_at_every_member(plans):
    s = small()
    b = rc.blocks(s)
    for cap, members in ((0, 1), (289, 1), (290, 2), (589, 2), (590, 3), (889, 3), (890, 4), (1189, 4), (1190, 5)):
        p = plans["cap/%d/0" % cap]
        oc, tr = ints(p["ocap"]), ints(p["trusted"])
        assert len(oc) == members and oc[-1] == 0 and tr[-1] == 0 and all(tr[:-1]) and all(oc[:-1]), cap
        assert ints(p["soff"])[-1] == b[members - 1][0], cap  # consumed of the capacity outcome: that member's start
    total = rc.out_len(s, voff(0, 10), voff(b[4][0], 50))[1]
    assert total == 290 + 900 + 50
    assert ints(plans["cap/%d/0" % (total - 1)]["ocap"])[-1] == 0 and ints(plans["cap/%d/0" % total]["ocap"])[-1] == 100


def test_header_failures_and_their_consumed(plans):
    s = small()
    for name, (_, start) in rc.header_failures(s).items():
        p = plans["fail/%s/0" % name.replace(" ", "_")]
        assert (int(p["verdict"]), int(p["vcons"]), p["soff"]) == (CHAIN, start, "-"), name
        assert plans["fail/" + name.replace(" ", "_")]["M"] == "0", name


def test_a_failing_stream_contributes_no_member(plans):
    assert ints(plans["batch/mixed"]["rstream"]) == [0, 0] + [3] * 71
    assert [int(plans["batch/mixed/%d" % i]["verdict"]) for i in range(4)] == [MEMBERS, CHAIN, EMPTY, MEMBERS]


def test_refusals(plans):
    assert plans["refused/order"]["refused"] == "2" and plans["refused/past_end"]["refused"] == "3"


def test_the_stand_alone_program_runs_clean_under_the_sanitizers(tmp_path, plans):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "emu_plan_bgzf_range_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    assert run(exe, all_cases()) == plans
