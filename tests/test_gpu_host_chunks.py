"""GPU tests of the host entries' four-chunk pipeline (capi.cpp, host_batch_run): a host batch
of at least 64 streams and "host_chunk_min" input bytes (default 32 MiB) runs as four chunks of streams over
three HIP streams.  With host_chunk_min = 1 the batches of hostchunkcases.py take that mode at a few hundred
KiB, on every route: each stream is compared with the oracle in all result arrays, and the chunked call with
the same call unchunked and with its four ranges issued as four calls (hostchunkcases.three_ways).  The last
tests run the real thresholds with the default options.

Every test asserts last_host_chunks() == 4 (three_ways does) before anything else, so none can pass by
running unchunked."""
import ctypes
import os

import pytest

import corpus
import dictcases
import golden_io
import hostchunkcases as hc
import oracle
import restartcases
from hostchunkcases import bounds, chunk_of, chunked, options, three_ways

pytestmark = pytest.mark.gpu

FMTS = ["deflate-raw", "deflate", "gzip"]
HEADER = {"deflate-raw": 0, "deflate": 2, "gzip": 10}
CAPACITY = (-5, 0, "output capacity exceeded")


def size_and_shift(k):
    """case k's stream count and rotation: 64, 67, 71 in turn, the seam members from another edge each time"""
    return hc.SIZES[k % 3], k % 7


# ================================================================== deflate
@pytest.mark.parametrize("level", [0, 1, 3, 4, 6, 9])
@pytest.mark.parametrize("fmt", FMTS)
def test_deflate_plain(engine, fmt, level):
    n, shift = size_and_shift(level + FMTS.index(fmt))
    items = hc.batch(n, shift)
    with options(engine, checksum_split=1, checksum_part=1024):
        res, (parts,) = three_ways(engine, n, lambda a, b: hc.deflate(engine, items[a:b], fmt, level),
                                   lambda: (engine.last_checksum_parts(),))
    hc.check_deflate(res, items, fmt, [hc.deflated(d, fmt, level) for d in items])
    # every chunk has a stream of more than one byte: all of them in parts of 1,024 bytes
    assert parts == (0 if fmt == "deflate-raw" else sum(max(1, -(-len(d) // 1024)) for d in items))


def test_deflate_520_streams(engine):
    items = hc.batch(520, 3)
    assert bounds(520) == [0, 65, 260, 455, 520]
    res, _ = three_ways(engine, 520, lambda a, b: hc.deflate(engine, items[a:b], "gzip", 6))
    hc.check_deflate(res, items, "gzip", [hc.deflated(d, "gzip", 6) for d in items])


def dictionaries():
    return [dictcases.dictionary(L, 910 + k) for k, L in enumerate((1, 257, 32767, 32768, 40000))]


def dict_assignment(n, variant):
    """One dictionary or None per stream.  "shared": every chunk sees another pair, dictionary 2 is in all
    four; "bare": chunk 1 has none at all, the others see other pairs.  Every third stream of a chunk has none."""
    D = dictionaries()
    subsets = {"shared": [(0, 2), (1, 2), (2, 3), (2, 4)], "bare": [(0, 1), (), (2, 3), (4, 0)]}[variant]
    out = []
    for i in range(n):
        sub = subsets[chunk_of(n, i)]
        k = i % (len(sub) + 1)
        out.append(D[sub[k]] if k < len(sub) else None)
    for c, sub in enumerate(subsets):  # the chunks see what this says they see
        assert {d for i, d in enumerate(out) if chunk_of(n, i) == c and d} == {D[j] for j in sub}
    return out


@pytest.mark.parametrize("variant", ["shared", "bare"])
@pytest.mark.parametrize("fmt", ["deflate-raw", "deflate"])
def test_deflate_dict(engine, fmt, variant):
    n, shift = (67, 2) if variant == "shared" else (71, 5)
    level = 6 if fmt == "deflate" else 1
    items, zd = hc.batch(n, shift), dict_assignment(n, variant)
    res, _ = three_ways(engine, n, lambda a, b: hc.deflate(engine, items[a:b], fmt, level, zdict=zd[a:b]))
    hc.check_deflate(res, items, fmt, [hc.deflated(d, fmt, level, zdict=z) for d, z in zip(items, zd)])


@pytest.mark.parametrize("strategy,rle_ref,fmt", [(2, 1, "gzip"), (4, 1, "deflate"), (1, 1, "deflate-raw"),
                                                  (3, 0, "deflate"), (3, 1, "gzip")])
def test_deflate_strategy(engine, strategy, rle_ref, fmt):
    """ZS_HUFFMAN_ONLY, ZS_FIXED, ZS_FILTERED, and ZS_RLE as zlib (rle_ref 0) and as the reference (1)"""
    n, shift = size_and_shift(strategy + rle_ref)
    items = hc.batch(n, shift)
    with options(engine, rle_ref=rle_ref):
        res, _ = three_ways(engine, n, lambda a, b: hc.deflate(engine, items[a:b], fmt, 6, strategy=strategy))
    oracle_strategy = 2 if strategy == 3 and rle_ref else strategy  # (the reference's deflate_rle finds no run)
    hc.check_deflate(res, items, fmt, [hc.deflated(d, fmt, 6, strategy=oracle_strategy) for d in items])


@pytest.mark.parametrize("code,mem_level,level", [(9, 1, 6), (-12, 9, 1), (27, 5, 9)])
def test_deflate_params(engine, code, mem_level, level):
    fmt = "deflate-raw" if code < 0 else "gzip" if code > 16 else "deflate"
    wb = -code if code < 0 else code - 16 if code > 16 else code
    n, shift = size_and_shift(mem_level)
    items = hc.batch(n, shift)
    res, _ = three_ways(engine, n, lambda a, b: hc.deflate(engine, items[a:b], fmt, level, params=(wb, mem_level)))
    hc.check_deflate(res, items, fmt, [hc.deflated(d, fmt, level, params=(wb, mem_level)) for d in items])


def test_deflate_capacity_one_byte_short(engine):
    """Z_BUF_ERROR on a seam member and on one member mid-chunk: status -5, length 0, the neighbours intact, the
    call ZS_OK (hc.deflate raises otherwise)"""
    n = 67
    items = hc.batch(n, 4)
    want = [hc.deflated(d, "deflate", 6) for d in items]
    short = {bounds(n)[2], bounds(n)[2] + 11}
    caps = [len(w) - 1 if i in short else len(w) + (i % 5) for i, w in enumerate(want)]
    res, _ = three_ways(engine, n, lambda a, b: hc.deflate(engine, items[a:b], "deflate", 6, caps=caps[a:b]))
    hc.check_deflate(res, items, "deflate", want, ok=[i not in short for i in range(n)])
    assert [i for i in range(n) if res["status"][i] != 1] == sorted(short)


# ------------------------------------------------------------------ Z_FULL_FLUSH points
def flush_positions(n, items, variant):
    """Per stream: no point, one point, a point every 1,000 bytes in turn; a point at 0 and at in_len on the seam
    slots.  variant "all": in every chunk; "mid": in chunks 1 and 2 only; "last": in chunk 3 only."""
    chunks = {"all": (0, 1, 2, 3), "mid": (1, 2), "last": (3,)}[variant]
    out = []
    for i, d in enumerate(items):
        if chunk_of(n, i) not in chunks:
            out.append([])
        elif i in hc.seams(n):
            out.append(sorted({0, len(d)}))
        else:
            out.append([[], [len(d) // 2], list(range(1000, len(d), 1000))][i % 3])
    return out


def last_flush_index(engine, per):
    """zs_last_flush_index, cut per stream"""
    total = sum(len(ps) for ps in per)
    buf = (ctypes.c_uint32 * max(1, total))()
    assert engine._L.zs_last_flush_index(engine.handle, buf, total) == total
    out, at = [], 0
    for ps in per:
        out.append(list(buf[at:at + len(ps)]))
        at += len(ps)
    return out


def flushed_call(engine, n, items, fmt, level, per):
    """the flushed batch three ways; bytes against flushcases.compress, the index of the chunked and of the
    unchunked call against the running sums of flushcases.parts; then the outputs and the index back through
    the restart decode, chunked"""
    probes = []

    def run(a, b):
        r = hc.deflate(engine, items[a:b], fmt, level, flush=per[a:b])
        if (a, b) == (0, n):
            probes.append(last_flush_index(engine, per))
        return r

    res, _ = three_ways(engine, n, run)
    hc.check_deflate(res, items, fmt, [hc.deflated(d, fmt, level, flush=tuple(ps)) for d, ps in zip(items, per)])
    want = [hc.flush_index(d, fmt, level, ps) for d, ps in zip(items, per)]
    assert len(probes) == 2
    for which, got in zip(("chunked", "unchunked"), probes):
        bad = [i for i in range(n) if got[i] != want[i]]
        assert not bad, (which, bad[:8], got[bad[0]][:4], want[bad[0]][:4])
    restart = [[(HEADER[fmt], 0)] + list(zip(idx, ps)) for idx, ps in zip(probes[0], per)]
    with chunked(engine):
        back = hc.inflate(engine, res["data"], fmt, [len(d) for d in items], restart=restart)
        assert engine.last_host_chunks() == 4
    hc.check_inflate(back, [(1, 0, "", d, len(s)) for d, s in zip(items, res["data"])], fmt)


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("fmt", FMTS)
def test_deflate_flush_every_chunk_has_points(engine, fmt, level):
    n, shift = size_and_shift(level + FMTS.index(fmt))
    items = hc.batch(n, shift)
    flushed_call(engine, n, items, fmt, level, flush_positions(n, items, "all"))


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("fmt", FMTS)
def test_deflate_flush_only_the_last_chunk_has_points(engine, fmt, level):
    n, shift = size_and_shift(level + FMTS.index(fmt) + 1)
    items = hc.batch(n, shift)
    flushed_call(engine, n, items, fmt, level, flush_positions(n, items, "last"))


def grown(cap, need):
    """the workspace buffers' ensure(): the capacity behind a request of `need` bytes (a regrow frees first:
    what the buffer held is gone)"""
    return cap if need <= cap else max(need + need // 8, 4096)


def scan_u64(m, points):
    """u64 values of a flushed device call's layout scan: one per segment and one more, one per tile of 256"""
    M = m + points
    return M + 1 + M // 256 + 1


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("fmt", FMTS)
def test_deflate_flush_only_the_middle_chunks_have_points_after_a_larger_flushed_call(fmt, level):
    """On one fresh context: a single-chunk flushed call with more points than the chunked batch has in all,
    then the chunked batch whose chunk 0 has no point.  Chunk 0 takes the plain path; had it left the scans'
    fill level (fscan_used) where the first call put it, chunks 1 and 2 would append behind it, past the room
    the host entry reserved for the call, and chunk 2's request would regrow the buffer -- a regrow frees
    first, so chunk 1's scan would be gone when zs_last_flush_index reads it.  The arithmetic, in u64 values
    (ZS_FLUSH_TILE = 256; a buffer grows to 9/8 of a request):
      first call: 20 streams of 250 bytes flushed every 10: 480 points, 500 segments; the host entry
        reserves 500 + 1 + 16 = 517 (4,136 bytes), the buffer holds 4136 + 517 = 4,653 bytes, 581 values; the
        scan fills 500 + 1 + 1 + 1 = 503;
      the batch (n = 67: chunks of 8, 25, 25, 9 streams, P1 and P2 points in chunks 1 and 2, 480 > P1 + P2 >= 25):
        reserves 67 + P + 0 + 16 <= 581: no regrow; chunk 1 would write at 503 and need 503 + 27 + P1 values,
        chunk 2 503 + 54 + P1 + P2 > 581: the regrow.
    The figures are worked out from the batch and asserted before the call."""
    import zsamd

    eng = zsamd.Engine()
    try:
        n = 67
        items = hc.batch(n, level + FMTS.index(fmt))
        per = flush_positions(n, items, "mid")
        first = [corpus.text(corpus.stream_seed(7300 + i), 250) for i in range(20)]
        first_per = [list(range(10, 250, 10))] * 20
        # --- the branch, on the host
        bnd = bounds(n)
        pts = [sum(len(per[i]) for i in range(bnd[k], bnd[k + 1])) for k in range(4)]
        assert pts[0] == 0 and pts[3] == 0 and pts[1] > 0 and pts[2] > 0
        stale_points = sum(len(ps) for ps in first_per)
        assert stale_points == 480 > sum(pts)
        mt0, mt = 20 + stale_points, n + sum(pts)
        cap = grown(0, 8 * (mt0 + mt0 // 256 + 16))
        stale = scan_u64(20, stale_points)
        assert (cap, stale) == (4653, 503)
        assert grown(cap, 8 * (mt + mt // 256 + 16)) == cap  # the batch's own reservation fits
        s1, s2 = scan_u64(bnd[2] - bnd[1], pts[1]), scan_u64(bnd[3] - bnd[2], pts[2])
        cap1 = grown(cap, 8 * (stale + s1))
        assert 8 * (stale + s1 + s2) > cap1, "chunk 2 would not regrow the scans' buffer behind a stale fill level"
        assert 8 * (stale + s1 + s2) > 1.125 * 8 * max(mt0 + mt0 // 256 + 16, mt + mt // 256 + 16)
        # --- the calls
        with chunked(eng, 0):
            r0 = hc.deflate(eng, first, fmt, level, flush=first_per)
            assert eng.last_host_chunks() == 1
            idx0 = last_flush_index(eng, first_per)
        hc.check_deflate(r0, first, fmt, [hc.deflated(d, fmt, level, flush=tuple(ps)) for d, ps in zip(first, first_per)])
        assert idx0 == [hc.flush_index(d, fmt, level, ps) for d, ps in zip(first, first_per)]
        with chunked(eng, 1):
            res = hc.deflate(eng, items, fmt, level, flush=per)
            assert eng.last_host_chunks() == 4
            got = last_flush_index(eng, per)
        hc.check_deflate(res, items, fmt, [hc.deflated(d, fmt, level, flush=tuple(ps)) for d, ps in zip(items, per)])
        want = [hc.flush_index(d, fmt, level, ps) for d, ps in zip(items, per)]
        bad = [i for i in range(n) if got[i] != want[i]]
        assert not bad, ("zs_last_flush_index", bad[:8], got[bad[0]][:4], want[bad[0]][:4])
        # the same batch the other two ways, and back through the restart decode
        flushed_call(eng, n, items, fmt, level, per)
    finally:
        eng.close()


# ================================================================== inflate
def members_of(items, fmt, level):
    enc = "deflate-raw" if fmt == "deflate64-raw" else fmt
    return [hc.deflated(d, enc, level) for d in items]


def lanes_and_segs(engine):
    return lambda: (engine.last_lane_count(), engine.last_seg_count())


@pytest.mark.parametrize("fmt", FMTS)
def test_inflate_plain(engine, fmt):
    """the deflate cases' outputs, capacities given exactly (no multiples of 4)"""
    k = FMTS.index(fmt)
    n, shift = size_and_shift(k + 1)
    items = hc.batch(n, shift)
    comp = members_of(items, fmt, (1, 6, 9)[k])
    caps = [len(d) for d in items]
    res, _ = three_ways(engine, n, lambda a, b: hc.inflate(engine, comp[a:b], fmt, caps[a:b]), lanes_and_segs(engine))
    hc.check_inflate(res, [hc.inflated(c, fmt, cap) for c, cap in zip(comp, caps)], fmt)
    assert res["status"] == [1] * n


def d64_fixtures():
    d = os.path.join(golden_io.GOLDEN, "d64")
    return [open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))]


def test_inflate_deflate64(engine):
    """the reference's deflate64 fixtures on the seam slots and beside them, raw deflate members elsewhere"""
    n = 64
    fx = [f for f in d64_fixtures() if len(f) < 32768]
    comp = members_of(hc.batch(n, 0), "deflate64-raw", 6)
    for j, i in enumerate(sorted(set(hc.seams(n)) | {s + 1 for s in hc.seams(n)})):
        comp[i] = fx[j % len(fx)]
    caps = [len(oracle.decompress(c, "deflate64-raw", cap=4 << 20)[1]) for c in comp]
    res, _ = three_ways(engine, n, lambda a, b: hc.inflate(engine, comp[a:b], "deflate64-raw", caps[a:b]),
                        lanes_and_segs(engine))
    hc.check_inflate(res, [hc.inflated(c, "deflate64-raw", cap) for c, cap in zip(comp, caps)], "deflate64-raw")
    assert res["status"] == [1] * n


def test_inflate_520_streams(engine):
    items = hc.batch(520, 6)
    comp = members_of(items, "deflate", 1)
    caps = [len(d) for d in items]
    res, _ = three_ways(engine, 520, lambda a, b: hc.inflate(engine, comp[a:b], "deflate", caps[a:b]),
                        lanes_and_segs(engine))
    hc.check_inflate(res, [hc.inflated(c, "deflate", cap) for c, cap in zip(comp, caps)], "deflate")


def damaged(member):
    """one bit flipped in the raw member's first block so that it produces no byte: the block type made the
    reserved one (a stored block: its NLEN spoiled)"""
    b = bytearray(member)
    btype = (b[0] >> 1) & 3
    if btype == 0:
        b[3] ^= 0x10
    else:
        b[0] ^= 0x02 if btype == 2 else 0x04
    return bytes(b)


def test_inflate_failures(engine):
    """Chunk 1 whole: damaged members, no byte produced (the compaction has nothing to copy for the chunk).
    Elsewhere, in turn: truncated members, members with trailing bytes (consumed < in_len), short capacities,
    clean members.  A short capacity is the engine's own outcome (ZS_BUF_ERROR, "output capacity exceeded":
    the reference has no capacity); everything else is the oracle's answer field for field."""
    n = 67
    items = hc.batch(n, 1)
    comp = members_of(items, "deflate-raw", 6)
    caps = [len(d) for d in items]
    short = []
    for i in range(n):
        if chunk_of(n, i) == 1:
            comp[i] = damaged(comp[i])
        elif i % 4 == 0 and len(comp[i]) > 4:
            comp[i] = comp[i][:len(comp[i]) * 2 // 3]
        elif i % 4 == 1:
            comp[i] = comp[i] + b"trailing!"
        elif i % 4 == 2 and len(items[i]) > 10:
            caps[i] = len(items[i]) // 2 + 1
            short.append(i)
    res, _ = three_ways(engine, n, lambda a, b: hc.inflate(engine, comp[a:b], "deflate-raw", caps[a:b]),
                        lanes_and_segs(engine))
    b = bounds(n)
    assert sum(res["len"][b[1]:b[2]]) == 0 and all(st == -3 for st in res["status"][b[1]:b[2]])
    assert any(res["consumed"][i] + 9 == len(comp[i]) and res["status"][i] == 1 for i in range(n))
    for i in short:
        assert (res["status"][i], res["phase"][i], res["msg"][i]) == CAPACITY, i
    keep = [i for i in range(n) if i not in short]
    sub = {key: [v[i] for i in keep] for key, v in res.items()}
    hc.check_inflate(sub, [hc.inflated(comp[i], "deflate-raw", caps[i]) for i in keep], "deflate-raw")


@pytest.mark.parametrize("ref_wrap", [1, 0])
@pytest.mark.parametrize("fmt", ["deflate-raw", "deflate64-raw"])
def test_inflate_mixed_routes_inside_one_call(engine, fmt, ref_wrap):
    """chunk 2 holds the large members (past inflate_wave_min by their input, or by their expansion): two of
    text of about 200 KiB and 1 MiB of zeros -- as deflate64, where a raw member's length 258 reads as code 285
    with 16 extra bits, the fixture of 100,000 zeros in its place, and the largest fixture; the other chunks
    only small ones"""
    n = 64
    items = hc.batch(n, 2 if fmt == "deflate-raw" else 0)  # (as deflate64: not the edge member of 40,000 zeros either)
    big = [corpus.text(corpus.stream_seed(7400), 200003), corpus.text(corpus.stream_seed(7401), 199999), bytes(1 << 20)]
    at = [34, 41, 47]
    for i, d in zip(at, big):
        items[i] = d
    comp = members_of(items, fmt, 1)
    if fmt == "deflate64-raw":
        fx = sorted(d64_fixtures(), key=len)
        comp[47], comp[50] = fx[0], fx[-1]
        assert len(fx[0]) == 369  # zeros_100k
    for i in at[:2] + ([50] if fmt == "deflate64-raw" else []):
        assert len(comp[i]) > 32768
    assert all(chunk_of(n, i) == 2 for i in at + [50])
    caps = [len(oracle.decompress(c, fmt, cap=8 << 20, reference_bugs=bool(ref_wrap))[1]) for c in comp]
    with options(engine, inflate_ref_wrap=ref_wrap):
        res, _ = three_ways(engine, n, lambda a, b: hc.inflate(engine, comp[a:b], fmt, caps[a:b]), lanes_and_segs(engine))
    hc.check_inflate(res, [hc.inflated(c, fmt, cap, bool(ref_wrap)) for c, cap in zip(comp, caps)], fmt)
    assert res["status"] == [1] * n


@pytest.mark.parametrize("variant", ["shared", "bare"])
@pytest.mark.parametrize("fmt", ["deflate-raw", "deflate"])
def test_inflate_dict(engine, fmt, variant):
    """the dictionary assignment of the deflate test; zlib: one member given another dictionary than it was
    written with (DICTID differs) and one FDICT member given none"""
    n, shift = (67, 2) if variant == "shared" else (71, 5)
    items, zd = hc.batch(n, shift), dict_assignment(n, variant)
    comp = [hc.deflated(d, fmt, 6, zdict=z) for d, z in zip(items, zd)]
    given = list(zd)
    want = [(1, 0, "", d, len(c)) for d, c in zip(items, comp)]
    if fmt == "deflate":
        D = dictionaries()
        wrong = next(i for i in range(bounds(n)[2], n) if zd[i] is not None)
        given[wrong] = next(d for d in D if d != zd[wrong])
        want[wrong] = (-3, 2, "", b"", None)
        none = next(i for i in range(bounds(n)[3], n) if zd[i] is not None and i != wrong)
        given[none] = None
        # the plain entry's answer, Z_NEED_DICT (how much of the header counts as consumed then is the engine's
        # own: the three ways must agree on it)
        want[none] = hc.inflated(comp[none], fmt, len(items[none]))[:4] + (None,)
        assert want[none][:4] == (2, 2, "", b"")
    caps = [len(d) for d in items]
    res, _ = three_ways(engine, n, lambda a, b: hc.inflate(engine, comp[a:b], fmt, caps[a:b], zdict=given[a:b]),
                        lanes_and_segs(engine))
    hc.check_inflate(res, want, fmt)


def restart_points(n, items):
    """0, 1 and 63 points in turn; chunks 0 and 3: every point a multiple of 4 (decoded in place), chunks 1 and
    2: any residue (the staging route)"""
    out = []
    for i, d in enumerate(items):
        k = (0, 1, 63)[i % 3]
        step = max(1, len(d) // (k + 1))
        ps = [step * j for j in range(1, k + 1) if step * j <= len(d)]
        if chunk_of(n, i) in (0, 3):
            ps = sorted({p & ~3 for p in ps})
        out.append(ps)
    return out


@pytest.mark.parametrize("fmt", ["gzip", "deflate-raw"])
def test_inflate_restart(engine, fmt):
    n, shift = (71, 3) if fmt == "gzip" else (67, 6)
    items = hc.batch(n, shift)
    pts = restart_points(n, items)
    made = [restartcases.flushed(d, ps, fmt) for d, ps in zip(items, pts)]
    restart = [[(HEADER[fmt], 0)] + idx for _, idx in made]
    comp = [s for s, _ in made]
    want = [(1, 0, "", d, len(s)) for d, s in zip(items, comp)]
    b = bounds(n)
    for c in (1, 2):
        assert any(p % 4 for i in range(b[c], b[c + 1]) for p in pts[i])
    for c in (0, 3):
        assert not any(p % 4 for i in range(b[c], b[c + 1]) for p in pts[i])
    assert {len(ps) for ps in pts} >= {0, 1, 63}
    # a false point in one stream of chunk 2: that stream alone fails
    bad = next(i for i in range(b[2] + 1, b[3]) if len(pts[i]) == 63)
    a, o = restart[bad][7]
    restart[bad][7] = (a + 1, o)
    want[bad] = restartcases.FAILED[:5]
    caps = [len(d) for d in items]
    res, _ = three_ways(engine, n, lambda x, y: hc.inflate(engine, comp[x:y], fmt, caps[x:y], restart=restart[x:y]))
    hc.check_inflate(res, want, fmt)
    assert res["check"][bad] == 0 and res["len"][bad] == 0


def test_inflate_auto(engine):
    """no member fits the entry's first capacity guess (max(64 KiB, 4 x input)): the retried members run as a
    chunked call of their own; the results are the sized call's"""
    n = 67
    items = [(hc.filler_at(i)[:700] * 100)[:66001 + 37 * i] for i in range(n)]
    comp = members_of(items, "gzip", 6)
    assert all(len(d) > max(65536, 4 * len(c)) for d, c in zip(items, comp))
    caps = [len(d) for d in items]
    with chunked(engine):
        auto = hc.inflate_auto(engine, comp, "gzip")
        assert engine.last_host_chunks() == 4
        sized = hc.inflate(engine, comp, "gzip", caps)
        assert engine.last_host_chunks() == 4
    assert hc.first_difference(auto, sized) is None, hc.first_difference(auto, sized)
    hc.check_inflate(auto, [hc.inflated(c, "gzip", cap) for c, cap in zip(comp, caps)], "gzip")
    assert auto["status"] == [1] * n


# ================================================================== the real thresholds, default options
MIB = 1 << 20
BIG = 528 * 1024  # the fillers' length: 63 of them hold 32 MiB


_BIG = []


def big_srcs():
    if not _BIG:
        import zsamd

        buf = bytes(zsamd.corpus("text", 7500, 8, BIG))
        _BIG.extend(buf[i * BIG:(i + 1) * BIG] for i in range(8))
        assert len(set(_BIG)) == 8
    return _BIG


def rotated(big, n, total):
    """n streams of the 8 contents in turn, trimmed so that they hold `total` bytes in all: neighbours differ"""
    base, extra = divmod(total, n)
    assert base + 1 <= BIG
    return [big[i % 8][:base + (i < extra)] for i in range(n)]


def oracle_of(items, fmt, level=1):
    return [hc.deflated(d, fmt, level) for d in items]


def test_the_edges_of_the_chunk_condition(engine):
    """63 streams past 32 MiB: one chunk; 64 streams one byte below: one chunk; 67 streams at 32 MiB: four"""
    a = rotated(big_srcs(), 63, 32 * MIB + 63)
    engine.compress_batch(a, "deflate-raw", 1)
    assert engine.last_host_chunks() == 1
    b = rotated(big_srcs(), 64, 32 * MIB - 1)
    engine.compress_batch(b, "deflate-raw", 1)
    assert engine.last_host_chunks() == 1
    c = rotated(big_srcs(), 67, 32 * MIB)
    got = engine.compress_batch(c, "deflate-raw", 1)
    assert engine.last_host_chunks() == 4
    assert got == oracle_of(c, "deflate-raw")
    # the same shape as gzip: streams past checksum_split, their check values in parts, chunk by chunk
    res = engine.compress_batch_detailed(c, "gzip", 1)
    assert engine.last_host_chunks() == 4
    assert engine.last_checksum_parts() == sum(-(-len(d) // 65536) for d in c)
    assert [(st, out) for st, out, _ in res] == [(1, w) for w in oracle_of(c, "gzip")]
    assert [chk for _, _, chk in res] == [hc.deflate_check(d, "gzip") for d in c]


def test_pack_regrow_in_a_single_chunk():
    """96 members of 1 MiB of zeros: about 100 KiB in, 96 MiB out.  The pack buffers' first guess is 64 MiB
    (72 MiB allocated): they grow when the one chunk's results are in"""
    import zsamd

    member = hc.deflated(bytes(MIB), "deflate-raw", 6)
    n = 96
    tin, tout = n * len(member), n * MIB
    pack0 = min(tout, max(4 * tin, 64 * MIB)) + 16
    assert grown(0, pack0) < n * MIB + 16  # the guess, as allocated, is less than the chunk packs
    eng = zsamd.Engine()
    try:
        res = eng.decompress_batch_raw([member] * n, "deflate-raw", out_caps=[MIB] * n)
        assert eng.last_host_chunks() == 1
    finally:
        eng.close()
    zeros = bytes(MIB)
    assert [(st, len(out), cons) for st, _, _, out, cons in res] == [(1, MIB, len(member))] * n
    assert all(out == zeros for _, _, _, out, _ in res)


def test_pack_regrow_between_chunks():
    """host_chunk_min = 1, host_pack_min = 1 MiB, 71 members: chunks 0 and 1 pack less than the buffers hold,
    chunk 2 runs past them -- chunks 0 and 1 reach the caller through the regrow path's scatter"""
    import zsamd

    n = 71
    b = bounds(n)
    items = hc.batch(n, 5)
    for i in range(b[2], b[3]):  # chunk 2: 27 members of about 56 KiB of text each
        items[i] = (hc.filler_at(i, 1)[:997] * 60)[:56001 + 4 * i + i % 3]
    comp = members_of(items, "deflate", 6)
    caps = [len(d) for d in items]
    pad4 = lambda v: (v + 3) & ~3
    packs = [sum(pad4(len(items[i])) for i in range(b[k], b[k + 1])) for k in range(4)]
    tin, tout = sum(len(c) for c in comp), sum(pad4(c) for c in caps)
    alloc = grown(0, min(tout, max(4 * tin, MIB)) + 16)  # the device pack buffer as first allocated: the smaller one
    assert packs[0] + packs[1] + 16 <= alloc < packs[0] + packs[1] + packs[2] + 16, (packs, alloc, tin, tout)
    eng = zsamd.Engine()
    try:
        eng.set_option("host_chunk_min", 1)
        eng.set_option("host_pack_min", MIB)
        res = hc.inflate(eng, comp, "deflate", caps)
        assert eng.last_host_chunks() == 4
    finally:
        eng.close()
    hc.check_inflate(res, [hc.inflated(c, "deflate", cap) for c, cap in zip(comp, caps)], "deflate")
    assert res["status"] == [1] * n and res["data"] == items


def test_pool_shards_chunk_at_the_real_threshold():
    """two shards on one GPU, 67 streams and a little over 32 MiB each: the pool's contexts take no options"""
    import zsamd

    items = rotated(big_srcs(), 134, 64 * MIB + 134 * 8)
    assert sum(len(d) for d in items[:67]) >= 32 * MIB and sum(len(d) for d in items[67:]) >= 32 * MIB
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        got = pool.compress_batch(items, "deflate-raw", 1)
    finally:
        pool.close()
    assert got == oracle_of(items, "deflate-raw")
