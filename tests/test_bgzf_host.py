"""The BGZF fast path's per-lane code (csrc/zs_bgzf.h: a start sized from BSIZE and ISIZE where its header can be
trusted, by zs_members_size where not), the plan over its records and the planned members' trusted flags
(zs_plan_bgzf_trusted), run on the CPU from their own source by tools/bgzf_host and checked against the rule written
out in Python (bgzfcases.trusted) and against tools/members_host's records for the same bytes.  The same stand-alone
program runs once more built with AddressSanitizer and UBSan: lanes started at EVERY byte offset stay inside the
aligned words of their stream."""
import struct

import pytest

import bgzfcases as bc
import corpus
import memberscases as mc
from memberscases import BGZF_EOF, FINAL, member, text


@pytest.fixture(scope="module")
def host():
    return bc.build("bgzf_host")


@pytest.fixture(scope="module")
def host_san():
    return bc.build("bgzf_host_san")


@pytest.fixture(scope="module")
def members_host():
    return mc.build("members_host")


def starts(s):
    return [a for a, _ in mc.walk(s)[0]]


def record_at(res, at):
    cand, recs = res[0], res[1]
    return recs[0] if at == 0 else recs[1 + cand.index(at)]


def test_every_true_block_start_is_trusted(host):
    streams = [bc.bgzf(text(300), 100), BGZF_EOF, bc.bgzf(text(70000, 2)), bc.bgzf(b"", eof=True)]
    for s, res in zip(streams, bc.run(host, streams)):
        idx, out, end, ok = mc.walk(s)
        assert ok and end == len(s)
        nxt = idx[1:] + [(end, len(out))]
        for (a, o), (b, o2) in zip(idx, nxt):
            assert record_at(res, a) == (FINAL, b, o2 - o, 0, 1), a  # (FINAL, next start, ISIZE, 0), trusted
        assert [m[:3] + (m[4],) for m in res[4]] == [(a, b - a, o, 1) for (a, o), (b, _) in zip(idx, nxt)]
        assert res[2] == 0 and res[5] == (1, len(out))
    # memberscases.bgzf() writes BSIZE 0: nothing to follow, so its blocks are sized from the data like any member
    s = mc.bgzf(text(300), block=100)
    res, = bc.run(host, [s])
    assert [m[4] for m in res[4]] == [0, 0, 0, 1] and [m[:4] for m in res[4]] == mc.run(mc.build(), [s])[0][4]


def untrusted_cases():
    d = text(200, 5)
    good = bc.block(d)
    flg = bytearray(mc.hand_member(d, extra=mc.bc_extra(0), name=b"n"))  # FLG 0x0c
    struct.pack_into("<H", flg, 16, len(flg) - 1)
    slen4 = bytearray(mc.hand_member(d, extra=b"BC\x04\x00" + b"\x00" * 4))
    struct.pack_into("<H", slen4, 16, len(slen4) - 1)
    untiled = bytearray(mc.hand_member(d, extra=mc.bc_extra(0) + b"Q"))  # XLEN 7: one byte is no subfield
    struct.pack_into("<H", untiled, 16, len(untiled) - 1)
    past = bc.block(d, bsize_delta=1)  # the last block of its stream: BSIZE + 1 is one past the end
    tiny = bytearray(good)
    struct.pack_into("<H", tiny, 16, 12 + 6 + 8 - 1)  # total = 12 + XLEN + 8: no byte of deflate data
    big = bc.block(d, isize=65537)
    cases = {"flg 0x0c": bytes(flg), "BC with SLEN 4": bytes(slen4), "subfields do not tile XLEN": bytes(untiled),
             "BSIZE one past the end": past, "total <= 12 + XLEN + 8": bytes(tiny), "ISIZE 65,537": big}
    assert flg[3] == 0x0c
    return cases


def test_untrusted_starts_get_members_hosts_records(host, members_host):
    lead = bc.block(text(50))
    cases = []  # (name, the stream, the untrusted start)
    for name, s in untrusted_cases().items():
        cases += [(name, s, 0), (name, lead + s, len(lead))]
        if name != "BSIZE one past the end":  # (with a block behind it the size fits: a lie, not this case)
            cases.append((name, lead + s + BGZF_EOF, len(lead)))
    streams = [s for _, s, _ in cases]
    got, want = bc.run(host, streams), mc.run(members_host, streams)
    every, every_m = bc.run_every_offset(host, streams), mc.run_every_offset(members_host, streams)
    for (name, s, at), g, w, e, em in zip(cases, got, want, every, every_m):
        assert bc.trusted(s, at) is None, name
        r = record_at(g, at)
        assert r[4] == 0 and r[:4] == record_at(w, at), name
        # every lane of the stream: untrusted ones are members_host's, trusted ones the header's
        assert g[0] == w[0]
        for x, (a, b) in enumerate(zip(g[1], w[1])):
            t = bc.trusted(s, 0 if x == 0 else g[0][x - 1])
            assert a == ((FINAL,) + t + (0, 1) if t else b + (0,)), (name, x)
        # ... and from every byte offset, unbounded
        for p, (a, b) in enumerate(zip(e, em)):
            t = bc.trusted(s, p)
            assert a == ((FINAL,) + t + (0, 1) if t else b + (0,)), (name, p)
        # the plan: members_host's members (the trusted headers of these streams tell the truth)
        assert [m[:4] for m in g[4]] == w[4], name


def test_an_xy_subfield_in_front_of_bc(host):
    s = bc.xy_block(text(500, 3)) + bc.block(text(20)) + BGZF_EOF
    res, = bc.run(host, [s])
    idx = mc.walk(s)[0]
    assert [(m[0], m[2], m[4]) for m in res[4]] == [(a, o, 1) for a, o in idx] and len(idx) == 3
    assert bc.trusted(s, 0) == (idx[1][0], 500) and res[5] == (1, 520)
    # the first BC subfield with SLEN 2 counts: a second one behind it is not read
    two = bytearray(bc.block(text(500, 3), back=mc.bc_extra(7)))
    assert bc.trusted(bytes(two), 0) == (len(two), 500)
    assert bc.run(host, [bytes(two)])[0][1][0] == (FINAL, len(two), 500, 0, 1)


def test_a_mixed_chain_and_the_capacity_cut(host):
    a, b = bc.block(text(40, 1)), bc.block(text(30, 2))
    s = a + member(b"abc") + b
    res, = bc.run(host, [s])
    assert [(m[0], m[2]) for m in res[4]] == mc.walk(s)[0]
    assert [m[4] for m in res[4]] == [1, 0, 1] and res[5] == (0, 0)
    # the member cut off by capacity gets no room and no flag; one that fits exactly keeps it
    for cap, want in [(73, [(40, 1), (3, 0), (30, 1)]), (72, [(40, 1), (3, 0), (0, 0)]), (42, [(40, 1), (0, 0)]), (39, [(0, 0)]), (0, [(0, 0)])]:
        (_, _, _, _, mem, _), = bc.run(host, [s], caps=[cap])
        assert [(m[3], m[4]) for m in mem] == want, cap
    # an empty block is flagged whatever room is left: its ISIZE of 0 is its room
    (_, _, _, _, mem, _), = bc.run(host, [a + BGZF_EOF], caps=[40])
    assert [(m[3], m[4]) for m in mem] == [(40, 1), (0, 1)]


def test_a_trusted_start_needs_no_tail_round(host, members_host):
    """a level-0 block whose stored data is a complete BGZF file of more blocks than sync_pass: members_host's lane from
    offset 0 is stopped by its bound and takes a tail round, the trusted lane reads no byte between header and trailer"""
    inner = bc.bgzf(text(120, 4), 10)
    assert len(mc.candidates(inner)) > 8
    s = bc.block(inner, level=0) + bc.block(text(9)) + BGZF_EOF
    (g,), (w,) = bc.run(host, [s]), mc.run(members_host, [s])
    assert w[2] == 1 and g[2] == 0 and [m[:4] for m in g[4]] == w[4] and [m[4] for m in g[4]] == [1, 1, 1]


def test_the_sanitizer_build_from_every_byte_offset(host_san):
    three = [bc.bgzf(text(300), 100) + b"\x1f\x8b\x08",
             bc.xy_block(text(60)) + member(b"abc") + mc.hand_member(text(60), extra=mc.bc_extra(), name=b"n", comment=b"c", fhcrc=True),
             corpus.rand(5, 1024) + b"\x1f\x8b\x08\x04\xff\xff"]
    res = bc.run_every_offset(host_san, three)
    for s, recs in zip(three, res):
        assert len(recs) == len(s)
        for p, r in enumerate(recs):
            t = bc.trusted(s, p)
            assert r[4] == (t is not None), p
            if t:
                assert r == (FINAL,) + t + (0, 1), p
    # the scan, the bounded lanes, the plan and the flags on the same streams, and the tiny inputs
    for sync_pass in (1, 8):
        bc.run(host_san, three, sync_pass)
    hdr = bc.block(text(10))[:17]
    tiny = bc.run(host_san, [b"", b"\x1f", hdr, hdr + b"\x00", BGZF_EOF[:-1], BGZF_EOF])
    assert [t[1][0][4] for t in tiny] == [0, 0, 0, 0, 0, 1] and [t[5] for t in tiny] == [(0, 0)] * 5 + [(1, 0)]
    bc.run_every_offset(host_san, [b"", b"\x1f", hdr, BGZF_EOF])
