"""GPU tests of the decode that finds its own restart points (zs_inflate_batch_sync*, inflate_sync.hip,
DESIGN 4.13): restart="scan" decodes every zlib-made stream to its source, field for field as the plain
entry with inflate_ref_wrap = 0 would, and last_restart_points() is the index of the stream's
Z_FULL_FLUSH points -- the smallest shapes at which the scan, the size decode and the plan can go wrong.
Every expectation comes from the zlib-built stream itself (restartcases.py, synccases.py)."""
import ctypes
import zlib

import pytest

import corpus
import synccases
from restartcases import FAILED, FORMATS, cap4, check_value, flushed, text, tiny_cases
from synccases import M

pytestmark = pytest.mark.gpu


def good(data, stream, fmt):
    return (1, 0, "", data, len(stream), check_value(data, fmt))


def scan(engine, fmt, streams, caps):
    got = engine.decompress_batch_detailed(streams, fmt, out_caps=caps, restart="scan")
    return got, engine.last_restart_points()


def roundtrip(engine, fmt, cases, level=6, slack=8):
    """cases: [(data, flush positions)]: every stream decodes to its source and its found points are
    the index flushed() returns"""
    made = [flushed(d, ps, fmt, level) for d, ps in cases]
    got, pts = scan(engine, fmt, [s for s, _ in made], [cap4(len(d)) + slack for d, _ in cases])
    for (d, ps), (s, idx), g, p in zip(cases, made, got, pts):
        assert g == good(d, s, fmt), (fmt, len(d), ps, g[:3], g[4:], len(g[3]))
        assert p == idx, (fmt, len(d), ps)
    return made


@pytest.mark.parametrize("fmt", FORMATS)
def test_abc_and_the_empty_input_with_every_subset_of_the_positions(engine, fmt):
    roundtrip(engine, fmt, tiny_cases())
    for case in tiny_cases():
        roundtrip(engine, fmt, [case], slack=0)


@pytest.mark.parametrize("fmt", ["deflate-raw", "gzip"])
def test_a_marker_at_every_input_byte_phase(engine, fmt):
    d40 = text(sum(range(1, 41)))
    at, p40 = 0, []
    for k in range(1, 40):
        at += k
        p40.append(at)
    roundtrip(engine, fmt, [(d40, p40), (text(300, 3), list(range(1, 300)))])


@pytest.mark.parametrize("d", [-3, -2, -1, 0, 1])
def test_a_marker_that_straddles_the_scans_first_tile_boundary(engine, d):
    """one stream in the call, so it starts at an aligned address and its first tile ends at byte 4096:
    a stored block of 4090 + d bytes puts the marker's four bytes at 4096 + d"""
    data = corpus.rand(21, 4090 + d) + text(100, 2)
    (s, idx), = roundtrip(engine, "deflate-raw", [(data, [4090 + d])], level=0)
    assert idx[0][0] - 4 == 4096 + d and s[4096 + d:4100 + d] == M


def _device(engine, fmt, streams, caps, in_offs, blob, guard=64):
    """the device entry over `blob`: (statuses, lengths, consumed, checks, the regions' bytes, the whole
    output, its offsets), regions `guard` bytes apart"""
    import torch

    n = len(streams)
    out_off, o = [], guard
    for c in caps:
        out_off.append(o)
        o += c + guard
    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_out = torch.full((o,), 0x5a, dtype=torch.uint8, device="cuda")
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st, d_ph, d_msg, d_len, d_cons, d_chk = i32(), i32(), i32(), i32(), i32(), i32()
    engine.decompress_device(fmt, n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*in_offs),
                             (ctypes.c_uint32 * n)(*[len(s) for s in streams]), d_out.data_ptr(),
                             (ctypes.c_uint64 * n)(*out_off), (ctypes.c_uint32 * n)(*caps), d_st.data_ptr(),
                             d_ph.data_ptr(), d_msg.data_ptr(), d_len.data_ptr(), d_cons.data_ptr(),
                             d_check=d_chk.data_ptr(), restart="scan")
    torch.cuda.synchronize()
    assert bytes(d_in.cpu().numpy()) == bytes(blob)  # the input is only read
    out = bytes(d_out.cpu().numpy())
    lens = d_len.tolist()
    return (d_st.tolist(), lens, d_cons.tolist(), [x & 0xffffffff for x in d_chk.tolist()],
            [out[a:a + l] for a, l in zip(out_off, lens)], out, out_off)


@pytest.mark.parametrize("fmt", ["deflate-raw", "gzip"])
def test_the_device_entry_at_every_input_alignment_between_markers(engine, fmt):
    """16 streams at input offsets of every residue mod 16 (so every residue mod 4), the bytes around
    each filled with 00 00 FF FF: a read past a stream's end would show as a false point"""
    cases = [(text(300 + 7 * k, k), list(range(1 + k, 300, 37))) for k in range(15)] + [(b"", [0])]
    made = [flushed(d, ps, fmt) for d, ps in cases]
    blob, in_offs = bytearray(M * 8), []
    for k, (s, _) in enumerate(made):
        while len(blob) % 16 != k:
            blob += M[len(blob) % 4:len(blob) % 4 + 1]  # (the filler keeps its phase: 00 00 FF FF throughout)
        in_offs.append(len(blob))
        blob += s
    while len(blob) % 4:
        blob += M[len(blob) % 4:len(blob) % 4 + 1]
    blob += M * 8
    st, lens, cons, chk, outs, _, _ = _device(engine, fmt, [s for s, _ in made], [cap4(len(d)) for d, _ in cases], in_offs, blob)
    assert st == [1] * 16 and outs == [d for d, _ in cases] and cons == [len(s) for s, _ in made]
    assert chk == [check_value(d, fmt) for d, _ in cases]
    assert engine.last_restart_points() == [idx for _, idx in made]


@pytest.mark.parametrize("fmt", FORMATS)
def test_no_marker_at_all_is_one_point_and_the_plain_decode(engine, fmt):
    datas = [text(4099, 4), b"", text(200000, 11)]
    comps = [flushed(d, [], fmt)[0] for d in datas]
    assert all(synccases.candidates(c, 0) == [] for c in comps)
    caps = [cap4(len(d)) + 4 for d in datas]
    try:
        engine.set_option("inflate_ref_wrap", 0)
        plain = engine.decompress_batch_detailed(comps, fmt, out_caps=caps)
    finally:
        engine.set_option("inflate_ref_wrap", 1)
    got, pts = scan(engine, fmt, comps, caps)
    assert got == plain == [good(d, c, fmt) for d, c in zip(datas, comps)]
    assert pts == [[], [], []]
    assert engine.last_seg_count() > 0  # (the 200,000-byte stream took a large decoder)


def test_hand_built_headers_in_one_batch_as_the_plain_entry(engine):
    """tests/bitbuild.py header_cases() in one deflate-raw batch: no stream holds a marker, so each is one point,
    the first point's lane sizes it (incomplete and empty distance sets, over-subscribed sets, every refusal of a
    header) and the plain decode follows.  Every stream the plain entry decodes comes back field for field as
    the plain entry's (status, phase, message, bytes, consumed, check), and those are the 11 zlib decodes, with
    zlib's bytes; every stream the plain entry rejects is the restart entries' one failure, as the entry's
    contract says (include/zs_gpu.h: lengths 0, not the plain entry's message and consumed), a data error there too."""
    import bitbuild

    made = [bitbuild.blocks(parts) for _, parts in bitbuild.header_cases()]
    streams = [m for m, _ in made]
    assert len(streams) == 29 and all(synccases.candidates(s, 0) == [] for s in streams)
    caps = [cap4(len(e)) + 64 for _, e in made]
    try:
        engine.set_option("inflate_ref_wrap", 0)
        plain = engine.decompress_batch_detailed(streams, "deflate-raw", out_caps=caps)
    finally:
        engine.set_option("inflate_ref_wrap", 1)
    got, pts = scan(engine, "deflate-raw", streams, caps)
    assert pts == [[]] * 29
    decoded = 0
    for s, g, p in zip(streams, got, plain):
        z = zlib.decompressobj(-15)
        try:
            out = z.decompress(s)
        except zlib.error:
            assert p[0] == FAILED[0] and g == FAILED
            continue
        assert z.eof and g == p == good(out, s, "deflate-raw")
        decoded += 1
    assert decoded == 11


def test_false_candidates_are_skipped(engine):
    for src, at, level, n_cand, true_at in synccases.FALSE_SOURCES:
        s, idx = flushed(src, [at], "deflate-raw", level)
        cand = synccases.candidates(s, 0)
        assert len(cand) == n_cand and cand[true_at] == idx[0][0]
        for fmt in FORMATS:
            roundtrip(engine, fmt, [(src, [at]), (text(100), [50])], level)


@pytest.mark.parametrize("K", [1, 8])
def test_the_pass_bound_ends_the_chain_and_the_stream_still_decodes(engine, K):
    d, s, idx = synccases.pass_case(K)
    assert len(idx) == 2 and len(synccases.candidates(s, 0)) == K + 4
    try:
        engine.set_option("sync_pass", K)
        got, pts = scan(engine, "deflate-raw", [s], [cap4(len(d))])
        assert got == [good(d, s, "deflate-raw")] and pts == [idx[:1]]  # the lane from the first flush passed
        engine.set_option("sync_pass", K + 2)
        got, pts = scan(engine, "deflate-raw", [s], [cap4(len(d))])
        assert got == [good(d, s, "deflate-raw")] and pts == [idx]
    finally:
        engine.set_option("sync_pass", 8)


def test_a_chain_that_ends_at_its_bound_behind_a_sync_flush(engine):
    """the lane behind the Z_SYNC_FLUSH is stopped inside a stored block full of markers before it has seen a
    copy; the tail's copies reach back across the point, so it is no restart point: one segment, the source"""
    d, s, at = synccases.passed_sync_case()
    got, pts = scan(engine, "deflate-raw", [s, s], [cap4(len(d)), cap4(len(d))])
    assert got == [good(d, s, "deflate-raw")] * 2 and pts == [[], []]


def test_sync_flush_points_are_dropped(engine):
    F, S = zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH
    d = synccases.repeated_text(5000)
    for fmt in FORMATS:
        s, idx = synccases.mixed(d, [(1000, F), (2000, S), (3000, F), (3500, S)], fmt)
        got, pts = scan(engine, fmt, [s], [cap4(len(d))])
        assert got == [good(d, s, fmt)] and pts == [synccases.full_points(idx)], fmt
    # a sync point, 500 random bytes (stored: no copy reaches back), a full flush: the rule of the plan
    # decides, computed from the stand-in's records
    d2 = synccases.repeated_text(2000) + corpus.rand(5, 500) + synccases.repeated_text(1500)
    s2, idx2 = synccases.mixed(d2, [(2000, S), (2500, F)], "deflate-raw")
    (_, _, _, want), = synccases.run(synccases.build(), [s2], "deflate-raw")
    got, pts = scan(engine, "deflate-raw", [s2], [cap4(len(d2))])
    assert got == [good(d2, s2, "deflate-raw")] and pts == [[tuple(p) for p in want[1:]]]
    assert (idx2[1][0], idx2[1][1]) in pts[0]


def test_bytes_behind_the_end_and_a_marker_in_the_gzip_header(engine):
    d = text(3000, 5)
    s, idx = flushed(d, [1000, 2000], "deflate-raw")
    got, pts = scan(engine, "deflate-raw", [s + M + b"junk" + M + b"\x01\x02\x03"], [cap4(len(d))])
    assert got == [good(d, s, "deflate-raw")] and pts == [idx]  # consumed stops at the final block
    g, hl = synccases.gzip_with_fields(s, d, b"a" + M + b"b" + M, b"name")
    got, pts = scan(engine, "gzip", [g], [cap4(len(d))])
    assert got == [good(d, g, "gzip")] and pts == [[(a + hl, b) for a, b in idx]]  # the scan starts behind the header


@pytest.mark.parametrize("fmt", ["deflate", "gzip"])
def test_a_broken_stream_fails_alone(engine, fmt):
    d1, d2 = text(5000, 1), text(9000, 2)
    s1, i1 = flushed(d1, [2500], fmt)
    s2, i2 = flushed(d2, [3000, 6000], fmt)
    cut = s2[:(i2[0][0] + i2[1][0]) // 2]  # truncated in the middle segment
    flip = bytearray(s2)
    flip[(i2[0][0] + i2[1][0]) // 2] ^= 0x10
    caps = [cap4(5000), cap4(9000), cap4(5000), cap4(9000), cap4(9000)]
    got, pts = scan(engine, fmt, [s1, cut, s1, bytes(flip), s2], caps)
    assert got == [good(d1, s1, fmt), FAILED, good(d1, s1, fmt), FAILED, good(d2, s2, fmt)]
    assert pts[0] == i1 and pts[2] == i1 and pts[4] == i2


@pytest.mark.parametrize("fmt", FORMATS)
def test_capacity_four_bytes_short(engine, fmt):
    d = text(20000, 6)
    s, idx = flushed(d, [8000], fmt)
    got, _ = scan(engine, fmt, [s, s], [len(d) - 4, len(d)])
    assert got[0][:4] == (-5, 0, "output capacity exceeded", b"") and got[0][4:] == (0, 0)
    assert got[1] == good(d, s, fmt)


@pytest.mark.parametrize("level", [1, 6])
def test_the_engines_own_flushed_streams(engine, level):
    datas = [text(30000 + 997 * k, k) for k in range(4)]
    for fmt in FORMATS:
        comps = engine.compress_batch(datas, fmt, level, flush_every=4096)
        index = engine.last_flush_index()
        want = [list(zip(i, range(4096, len(d) + 1, 4096))) for i, d in zip(index, datas)]
        assert all(len(w) == len(d) // 4096 for w, d in zip(want, datas))
        got, pts = scan(engine, fmt, comps, [cap4(len(d)) for d in datas])
        assert got == [good(d, c, fmt) for d, c in zip(datas, comps)] and pts == want


def test_the_pool_finds_the_points_too(engine):
    import zsamd

    cases = [(text(40000 + 13 * k, k), list(range(5000 + k, 40000, 5000))) for k in range(5)] + tiny_cases()
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        for fmt in FORMATS:
            made = [flushed(d, ps, fmt) for d, ps in cases]
            got = pool.decompress_batch_detailed([s for s, _ in made], fmt, out_caps=[cap4(len(d)) for d, _ in cases],
                                                 restart="scan")
            assert got == [good(d, s, fmt) for (d, _), (s, _) in zip(cases, made)]
    finally:
        pool.close()


def test_no_store_leaves_a_region_when_good_and_failing_streams_mix(engine):
    fmt = "gzip"
    datas = [text(30000, 1), text(5, 2), text(70001, 3), text(9000, 4), b"", text(6000, 5)]
    points = [[4096, 20000], [1, 3], [65537], [4000], [0], [1001, 3003]]
    made = [flushed(d, ps, fmt) for d, ps in zip(datas, points)]
    streams = [s for s, _ in made]
    flip = bytearray(streams[3])
    flip[made[3][1][0][0] + 40] ^= 0x04  # a byte of the second segment: this stream fails
    streams[3] = bytes(flip)
    streams[5] = streams[5][:made[5][1][1][0] - 9]  # truncated in its middle segment
    caps = [cap4(len(d)) for d in datas]
    caps[2] -= 4  # ... and this one does not fit
    blob, in_offs = bytearray(b"\xa5" * 64), []
    for s in streams:
        in_offs.append(len(blob))
        blob += s
    blob += b"\xa5" * 64
    st, lens, cons, chk, outs, out, out_off = _device(engine, fmt, streams, caps, in_offs, blob)
    assert st == [1, 1, -5, -3, 1, -3] and lens == [30000, 5, 0, 0, 0, 0]
    assert cons == [len(streams[0]), len(streams[1]), 0, 0, len(streams[4]), 0]
    assert chk == [zlib.crc32(datas[0]), zlib.crc32(datas[1]), 0, 0, 0, 0]
    assert outs[0] == datas[0] and outs[1] == datas[1]
    end = 0
    for k in range(len(streams)):
        assert out[end:out_off[k]] == b"\x5a" * (out_off[k] - end), k  # the guard in front of region k
        end = out_off[k] + caps[k]
    assert out[end:] == b"\x5a" * 64


def test_the_option_the_phases_the_chunk_count_and_the_record(engine):
    import zsamd

    for v in (0, -1, 65):
        with pytest.raises(zsamd.ZsError, match="sync_pass must be 1 .. 64"):
            engine.set_option("sync_pass", v)
    for v in (1, 64, 8):
        engine.set_option("sync_pass", v)
    cases = [(text(3000 + k, k), [1000, 2000]) for k in range(70)]  # (70 streams: a plain host call may be chunked)
    engine.set_timing(True)
    try:
        engine.set_option("host_chunk_min", 1)
        made = roundtrip(engine, "gzip", cases)
        assert engine.last_host_chunks() == 1  # the scan is not chunked
        assert engine.last_ms("sync_scan") >= 0 and engine.last_ms("sync_size") >= 0 and engine.last_ms("restart_gather") >= 0
        # the found points are an index: the restart entry takes them
        pts = engine.last_restart_points()
        caps = [cap4(len(d)) for d, _ in cases]
        got = engine.decompress_batch_detailed([s for s, _ in made], "gzip", out_caps=caps, restart=pts)
        assert got == [good(d, s, "gzip") for (d, _), (s, _) in zip(cases, made)]
        assert engine.last_ms("sync_scan") < 0  # (no scan in that call)
        assert engine.last_restart_points() == []  # the last inflate call was no scan call
        assert engine.last_host_chunks() == 4
    finally:
        engine.set_option("host_chunk_min", 32 << 20)
        engine.set_timing(False)
