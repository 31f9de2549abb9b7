"""The member search's per-lane code (csrc/zs_members.h: the scan's candidate rule and the sizing of one
member, zs_k_members_size's lane) and the plan over its records (zs_plan_members, with its tail rounds),
run on the CPU from their own source by tools/members_host and checked against Python's zlib.  The same
stand-alone program runs once more built with AddressSanitizer and UBSan: lanes started at EVERY byte
offset of three streams stay inside the aligned words of their stream."""
import zlib

import pytest

import corpus
import memberscases as mc
from memberscases import BGZF_EOF, ERROR, FINAL, PASSED, member, text


@pytest.fixture(scope="module")
def host():
    return mc.build("members_host")


@pytest.fixture(scope="module")
def host_san():
    return mc.build("members_host_san")


def streams_of_members():
    m = [member(text(50 * k + 1, k), lv) for k, lv in enumerate([0, 1, 6, 9, 6])]
    return [
        m[0],
        m[0] + m[1],
        b"".join(m),
        member(b"abc") + member(b""),
        member(b"") + member(b"a") + member(b""),
        BGZF_EOF,
        mc.bgzf(text(300, 3), block=100),
        member(corpus.rand(3, 5000)) + mc.hand_member(text(70, 1), extra=mc.bc_extra(77), name=b"n.txt", comment=b"c", fhcrc=True),
        b"".join(member(bytes([65 + k % 26]) * (1 + k % 3)) for k in range(130)),
    ]


def check(stream, result, sync_pass=8):
    cand, recs, rounds, in_place, mem = result
    assert cand == mc.candidates(stream)  # the scan's rule over aligned words = the bytes' own
    idx, out, end, ok = mc.walk(stream)
    assert ok
    starts = idx + [(end, len(out))]
    for k, (a, o) in enumerate(idx):
        how, e, n, reach = recs[0] if a == 0 else recs[1 + cand.index(a)]
        if how == PASSED:  # only a lane its bound stopped: more than sync_pass candidates inside the member
            assert len([q for q in cand if a < q < starts[k + 1][0]]) > sync_pass
            continue
        assert (how, e, n, reach) == (FINAL, starts[k + 1][0], starts[k + 1][1] - o, 0), (k, a)
    # the planned index is the zlib-derived one; every member has its bytes and its length for room
    assert [(a, o) for a, _, o, _ in mem] == idx
    assert [(a + n, c) for a, n, _, c in mem] == [(starts[k + 1][0], starts[k + 1][1] - idx[k][1]) for k in range(len(idx))]
    assert in_place == all(o % 4 == 0 for _, o in idx[1:])
    return rounds


def test_every_true_start_is_final_with_the_next_start_and_the_length(host):
    streams = streams_of_members()
    for s, res in zip(streams, mc.run(host, streams)):
        assert check(s, res) == 0


def test_trailing_bytes_end_the_stream(host):
    base = member(text(40)) + member(b"xy")
    tails = [b"\x00" * 37, corpus.rand(5, 50), b"\x1f\x8b\x08", b"\x1f\x8b", b"\x1f\x8b\x08\xe0" + b"\x00" * 20, b"\x1f\x8b\x07\x00" + b"\x00" * 20]
    streams = [base + t for t in tails]
    for s, res in zip(streams, mc.run(host, streams)):
        check(s, res)
        assert mc.walk(s)[2] == len(base) and len(res[4]) == 2
    # 1f 8b 08 00 + garbage IS a member: the last one, issued with the input to the end and the room that is left
    s = base + b"\x1f\x8b\x08\x00" + b"\x55" * 30
    (cand, recs, rounds, in_place, mem), = mc.run(host, [s], caps=[100])
    assert len(base) in cand and recs[1 + cand.index(len(base))][0] == ERROR
    assert mem[-1] == (len(base), len(s) - len(base), 42, 100 - 42) and len(mem) == 3


def test_a_truncated_last_member(host):
    a, b = member(text(40)), mc.hand_member(text(900, 2), name=b"file")
    for cut in (7, 12, len(b) // 2, len(b) - 8, len(b) - 1):  # inside the header, the name, the data, the trailer
        s = a + b[:cut]
        (cand, recs, rounds, in_place, mem), = mc.run(host, [s], caps=[5000])
        idx, out, at, ok = mc.walk(s)
        assert not ok and at == len(a) and out == text(40)
        assert recs[1 + cand.index(len(a))][0] == ERROR, cut
        assert mem == [(0, len(a), 0, 40), (len(a), cut, 40, 4960)]


@pytest.mark.parametrize("inner,sync_pass,rounds", [(12, 8, 1), (3, 1, 1), (3, 8, 0)])
def test_stored_gz_files_take_a_tail_round_and_are_not_cut(host, inner, sync_pass, rounds):
    """one level-0 member stores `inner` tiny complete .gz files: each passes the scan's rule and sizes as a member, so
    the lane from offset 0 is stopped by its bound when there are more than sync_pass of them (PASSED) and the
    unbounded tail lane settles it; the plan does not cut inside the stored member and finds the member behind it"""
    s, data, second = mc.stored_gz_case(inner)
    res, = mc.run(host, [s], sync_pass)
    cand, recs, got_rounds, in_place, mem = res
    assert len([q for q in cand if q < second]) >= inner and second in cand
    assert (recs[0][0] == PASSED) == (inner > sync_pass)
    assert check(s, res, sync_pass) == got_rounds == rounds
    assert [(a, o) for a, _, o, _ in mem] == [(0, 0), (second, len(data) - 300)]
    # every lane kept its bound
    for x, (how, end, _, _) in enumerate(recs):
        bound = cand[x + sync_pass] if x + sync_pass < len(cand) else len(s)
        assert end <= bound, (x, how, end, bound)


def test_the_capacity_cut_from_real_records(host):
    s = member(b"abcd") + member(b"efghi") + member(b"jk")
    for cap, want in [(11, [(4, 4), (5, 5), (2, 2)]), (10, [(4, 4), (5, 5), (2, 0)]), (8, [(4, 4), (5, 0)]), (0, [(4, 0)])]:
        (_, _, _, _, mem), = mc.run(host, [s], caps=[cap])
        assert [((4, 5, 2)[k], c) for k, (_, _, _, c) in enumerate(mem)] == want, cap


def test_the_sanitizer_build_from_every_byte_offset(host_san):
    three = [member(b"abc") + member(b"") + mc.hand_member(text(60), extra=mc.bc_extra(), name=b"n", comment=b"c", fhcrc=True) + b"\x1f\x8b\x08",
             mc.stored_gz_case(3)[0],
             corpus.rand(5, 1024) + b"\x1f\x8b\x08\x04\xff\xff"]
    res = mc.run_every_offset(host_san, three)
    for s, recs in zip(three, res):
        assert len(recs) == len(s) and all(how in (FINAL, ERROR) and end <= len(s) for how, end, _, _ in recs)
        for at, (how, end, n, _) in enumerate(recs):  # FINAL exactly where zlib decodes a whole member from there
            d = zlib.decompressobj(31)
            try:
                o = d.decompress(s[at:])
                whole = d.eof
            except zlib.error:
                whole = False
            assert (how == FINAL) == whole, at
            if whole:
                assert (end, n) == (len(s) - len(d.unused_data), len(o)), at
    # ... and the scan, the bounded lanes and the plan with its tail rounds, on the same streams and the others
    for sync_pass in (1, 8):
        for s, r in zip(three[:2], mc.run(host_san, three, sync_pass)[:2]):
            check(s, r, sync_pass)
    for s, r in zip(streams_of_members(), mc.run(host_san, streams_of_members(), 2)):
        check(s, r, 2)
    mc.run(host_san, [b"", b"\x1f", b"\x1f\x8b\x08\x00", b"\x00" * 40, member(b"q")[:-3]])
