"""The restart-point search's per-lane code (csrc/zs_sync.h: the scan's candidate rule and the count-only
decode of zs_k_sync_size) and the plan over its records (zs_plan_sync), run on the CPU from their own
source by tools/sync_host and checked against Python's zlib.  The same stand-alone program runs once
more built with AddressSanitizer and UBSan: lanes started at EVERY byte offset of three streams stay
inside the aligned words of their stream and end in one of the four ways."""
import zlib

import pytest

import corpus
import synccases
from restartcases import FORMATS, flushed, text, tiny_cases
from synccases import ERROR, FINAL, LANDED, M, PASSED


@pytest.fixture(scope="module")
def host():
    return synccases.build("sync_host")


@pytest.fixture(scope="module")
def host_san():
    return synccases.build("sync_host_san")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_every_true_start_lands_on_the_next_true_point(host, fmt, level):
    cases = tiny_cases() + [(text(300, 3), list(range(0, 301, 7))), (text(70000, 4), [10000, 30000, 65536]),
                            (corpus.rand(3, 5000), [100, 2500])]
    made = [flushed(d, ps, fmt, level) for d, ps in cases]
    for (d, ps), (s, idx), (first, cand, recs, pts) in zip(cases, made, synccases.run(host, [s for s, _ in made], fmt)):
        assert cand == synccases.candidates(s, first)  # the scan's rule over aligned words = the bytes' own
        starts = [(first, 0)] + idx
        for k, (a, o) in enumerate(starts):
            how, end, n, reach = recs[0] if k == 0 else recs[1 + cand.index(a)]
            if k + 1 < len(starts):
                assert (how, end, n, reach) == (LANDED, starts[k + 1][0], starts[k + 1][1] - o, 0), (len(d), ps, k)
            else:
                trailer = {"deflate-raw": 0, "deflate": 4, "gzip": 8}[fmt]
                assert (how, end, n, reach) == (FINAL, len(s) - trailer, len(d) - o, 0), (len(d), ps, k)
        assert pts == starts


def test_reach_is_positive_exactly_where_zlib_rejects_the_segment(host):
    data = corpus.text(corpus.stream_seed(7), 3000)
    s, idx = synccases.mixed(data, [(1000, zlib.Z_SYNC_FLUSH), (2000, zlib.Z_FULL_FLUSH)])
    (first, cand, recs, pts), = synccases.run(host, [s], "deflate-raw")
    (a1, _, _), (a2, _, _) = idx
    assert cand == [a1, a2]

    def zlib_takes(seg):
        try:
            return len(zlib.decompressobj(-15).decompress(seg + b"\x03\x00"))
        except zlib.error as e:
            assert "invalid distance too far back" in str(e)
            return None

    assert zlib_takes(s[a1:a2]) is None and zlib_takes(s[a2:]) == 1000 and zlib_takes(s[:a1]) == 1000
    assert recs[0] == (LANDED, a1, 1000, 0)
    assert recs[1][:3] == (LANDED, a2, 1000) and recs[1][3] > 0
    assert recs[2][0] == FINAL and recs[2][2:] == (1000, 0)
    assert pts == [(0, 0), (a2, 2000)]  # the sync point is dropped, the full one kept


@pytest.mark.parametrize("K", [1, 8])
def test_no_start_reads_past_candidate_j_plus_k_plus_1(host, K):
    d, s, idx = synccases.pass_case(K)
    (first, cand, recs, pts), = synccases.run(host, [s], "deflate-raw", K)
    assert len(cand) == K + 4 and cand[0] == idx[0][0] and cand[-1] == idx[1][0]
    for x, (how, end, _, _) in enumerate(recs):  # lane x - 1 of the candidates (the first point: -1)
        bound = cand[x + K] if x + K < len(cand) else len(s)
        assert end <= bound and (how != PASSED or end == bound), (x, how, end, bound)
    assert recs[1][0] == PASSED and pts == [(0, 0), idx[0]]  # the chain stops at the lane that passed
    (_, _, recs, pts), = synccases.run(host, [s], "deflate-raw", K + 2)
    assert recs[1][:2] == (LANDED, idx[1][0]) and pts == [(0, 0)] + idx
    # random bytes full of markers: every lane keeps its bound
    junk = b"".join(corpus.rand(k, 9) + M for k in range(60))
    (_, cand, recs, _), = synccases.run(host, [junk], "deflate-raw", K)
    assert len(cand) >= 60
    for x, (how, end, _, _) in enumerate(recs):
        assert end <= (cand[x + K] if x + K < len(cand) else len(junk))


def test_false_candidates_and_a_marker_in_the_header(host):
    for src, at, level, n_cand, true_at in synccases.FALSE_SOURCES:
        s, idx = flushed(src, [at], "deflate-raw", level)
        (first, cand, recs, pts), = synccases.run(host, [s], "deflate-raw")
        assert len(cand) == n_cand and cand[true_at] == idx[0][0] and pts == [(0, 0)] + idx
    d = text(3000, 5)
    s, idx = flushed(d, [1000, 2000], "deflate-raw")
    g, hl = synccases.gzip_with_fields(s, d, b"a" + M + b"b" + M, b"name")
    (first, cand, recs, pts), = synccases.run(host, [g], "gzip")
    assert first == hl and cand == [a + hl for a, _ in idx] and pts == [(hl, 0)] + [(a + hl, b) for a, b in idx]
    # a gzip header that does not end: the first point is 0, which the restart path's header check fails
    (first, _, _, pts), = synccases.run(host, [g[:12]], "gzip")
    assert first == 0 and pts == [(0, 0)]


def test_the_sanitizer_build_from_every_byte_offset(host_san):
    three = [zlib.compress(text(2000), 6)[2:-4],
             flushed(b"abc" + M + b"defg" + M * 3 + text(200), [50], "deflate-raw", 0)[0],
             corpus.rand(5, 1024)]
    res = synccases.run_every_offset(host_san, three, "deflate-raw")
    for s, (first, recs) in zip(three, res):
        assert len(recs) == len(s) and all(how in (LANDED, FINAL, ERROR, PASSED) and end <= len(s) for how, end, _, _ in recs)
    assert res[0][1][0][0] == FINAL and res[0][1][0][2] == 2000
    assert LANDED in {r[0] for r in res[1][1]}
    # ... and the scan, the bounded lanes and the plan, on the same streams and the flushed cases
    synccases.run(host_san, three, "deflate-raw", 1)
    for fmt in FORMATS:
        synccases.run(host_san, [flushed(d, ps, fmt)[0] for d, ps in tiny_cases()], fmt)


def test_a_passed_tail_is_sized_to_its_end_for_its_reach(host):
    """the chain ends at a lane its bound stopped, which started behind a Z_SYNC_FLUSH and had seen no copy yet:
    the whole tail's reach drops the point, and the stream is one segment (zlib rejects the tail alone)"""
    data, s, at = synccases.passed_sync_case()
    with pytest.raises(zlib.error, match="invalid distance too far back"):
        zlib.decompressobj(-15).decompress(s[at:])
    (first, cand, recs, pts), = synccases.run(host, [s], "deflate-raw")
    assert cand[0] == at and len(cand) == 13
    assert recs[0] == (LANDED, at, 1400, 0) and recs[1][0] == PASSED and recs[1][1] == cand[9] and recs[1][3] > 0
    assert pts == [(0, 0)]
    # with the bound past the markers the lane lands behind the stored block, whose data ends with the marker's
    # bytes; the lane from there sees the copies, which reach back across both points
    (_, _, recs, pts), = synccases.run(host, [s], "deflate-raw", 12)
    assert recs[1] == (LANDED, cand[12], 156, 0) and recs[13][0] == FINAL and recs[13][3] > 156 and pts == [(0, 0)]


def test_hand_built_headers_end_as_zlib_does(host):
    """tests/bitbuild.py header_cases() as deflate-raw streams, the lane from offset 0: FINAL at the stream's end
    with zlib's length where zlib decodes the stream, ERROR where it rejects it.  Five of the decoded ones have
    an incomplete or empty distance set (a lone code of length 1, or none: inftrees.ts:128-139)."""
    import bitbuild
    from test_huffman_cases import HEADERS_ACCEPTED

    names = [name for name, _ in bitbuild.header_cases()]
    streams = [bitbuild.blocks(parts)[0] for _, parts in bitbuild.header_cases()]
    assert len(streams) == 29
    decoded = []
    for name, s, (_, recs) in zip(names, streams, synccases.run_every_offset(host, streams, "deflate-raw")):
        how, end, n, _ = recs[0]
        z = zlib.decompressobj(-15)
        try:
            out = z.decompress(s)
        except zlib.error:
            assert how == ERROR, name
            continue
        assert z.eof and (how, end, n) == (FINAL, len(s), len(out)), name
        decoded.append(name)
    assert decoded == HEADERS_ACCEPTED and len(decoded) == 11
