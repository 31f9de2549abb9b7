"""GPU tests of the decode from restart points (zs_inflate_batch_restart*, inflate_restart.hip, DESIGN
4.11): a stream given with the (in_pos, out_pos) of its Z_FULL_FLUSH markers decodes as independent
segments and comes back as one stream -- the source's bytes, the whole length, the trailer's check
value -- or as the one failure, by status alone.  Inputs are made with Python's zlib (restartcases.py)
and with the engine's own flushed compress and zs_last_flush_index."""
import ctypes
import json
import os
import zlib

import pytest

import corpus
import golden_io
import oracle
from restartcases import FAILED, FORMATS, cap4, check_value, flushed, text, tiny_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def good(data, stream, fmt):
    return (1, 0, "", data, len(stream), check_value(data, fmt))


def decode(engine, fmt, items, caps=None):
    """items: [(stream, points)]; caps default to each source's length rounded up to 4 plus 8"""
    return engine.decompress_batch_detailed([s for s, _ in items], fmt, out_caps=caps, restart=[p for _, p in items])


def roundtrip(engine, fmt, cases, level=6, slack=8):
    """cases: [(data, flush positions)]: every stream decodes to its source, field for field"""
    made = [flushed(d, ps, fmt, level) for d, ps in cases]
    got = decode(engine, fmt, made, [cap4(len(d)) + slack for d, _ in cases])
    for (d, ps), (s, _), g in zip(cases, made, got):
        assert g == good(d, s, fmt), (fmt, len(d), ps, g[:3], g[4:], len(g[3]))
    return made


@pytest.mark.parametrize("fmt", FORMATS)
def test_abc_and_the_empty_input_with_every_subset_of_the_positions(engine, fmt):
    """segments of the marker's 5 bytes alone, a last segment that is 03 00 alone, every unaligned
    out_pos (the staging route); each case alone and all of them in one call"""
    roundtrip(engine, fmt, tiny_cases())
    for case in tiny_cases():
        roundtrip(engine, fmt, [case], slack=0)


@pytest.mark.parametrize("fmt", FORMATS)
def test_points_at_multiples_of_4_decode_in_place(engine, fmt):
    cases = [(text(n, n), [p for p in ps if p <= n]) for n in (8, 12, 13, 100, 4099) for ps in ([0, 4, 8], [4, 8], [8])]
    engine.set_timing(True)
    try:
        roundtrip(engine, fmt, cases)
        assert engine.last_ms("restart_gather") >= 0 and engine.last_ms("restart_stitch") >= 0
        assert engine.last_ms("restart_place") < 0  # the segments decoded where they belong
        roundtrip(engine, fmt, cases[:3] + [(text(50), [4, 9])])
        assert engine.last_ms("restart_place") >= 0  # one point in the call is no multiple of 4: the staging route
    finally:
        engine.set_timing(False)


@pytest.mark.parametrize("fmt", ["deflate-raw", "gzip"])
def test_a_marker_at_every_input_byte_phase_and_more_segments_than_one_stitch_wave(engine, fmt):
    d40 = text(sum(range(1, 41)))
    at, p40 = 0, []
    for k in range(1, 40):
        at += k
        p40.append(at)
    d300 = text(300, 3)
    roundtrip(engine, fmt, [(d40, p40), (d300, list(range(1, 300)))])
    # the same pieces at positions that are multiples of 4: more than 64 segments in place
    roundtrip(engine, fmt, [(text(1200, 5), list(range(4, 1200, 4)))])


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("shift", [0, 1])
def test_large_segments_take_a_large_decoder(engine, level, shift):
    """200,000 bytes of text flushed every 65,536 and once at 70,000: segments past the lanes' input
    threshold, over 64 KiB of output; in place (shift 0) and through the staging route (shift 1)"""
    d = text(200000, 11)
    ps = [p + shift for p in (65536, 70000, 131072, 196608)]
    made = roundtrip(engine, "gzip", [(d, ps)], level)
    assert engine.last_seg_count() > 0  # (the segmented decode finished segments: no lane decoded them alone)
    roundtrip(engine, "deflate", [(d, ps), (d[:100], [4 + shift])], level)
    assert max(b - a for (a, _), (b, _) in zip(made[0][1], made[0][1][1:])) > 4096


def test_stored_blocks_inside_a_segment(engine):
    d = text(3000, 1) + corpus.rand(5, 70000) + text(3000, 2)
    for fmt in FORMATS:
        roundtrip(engine, fmt, [(d, [3000, 40000, 73000]), (d, [2999, 73001])])


def test_one_mebibyte_in_256_segments(engine):
    d = text(1 << 20, 21)
    roundtrip(engine, "gzip", [(d, list(range(4096, 1 << 20, 4096)))])
    roundtrip(engine, "deflate-raw", [(d, list(range(4097, 1 << 20, 4096)))])


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_broken_stream_leaves_its_neighbours_alone(engine, fmt):
    d1, d2, d8 = text(5000, 1), text(6000, 2), text(90000, 8)
    s1, i1 = flushed(d1, [], fmt)
    s2, i2 = flushed(d2, [3001], fmt)
    s8, i8 = flushed(d8, list(range(10000, 80000, 10000)), fmt)
    bad = [(i2[0][0] + 1, i2[0][1])]
    got = decode(engine, fmt, [(s8, i8), (s2, bad), (s1, i1), (s2, i2)], [cap4(90000), cap4(6000), cap4(5000), cap4(6000)])
    assert got == [good(d8, s8, fmt), FAILED, good(d1, s1, fmt), good(d2, s2, fmt)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_stream_with_only_its_first_point_is_the_plain_decode_with_zlib_semantics(engine, fmt):
    datas = [b"", b"abc", text(70000, 4), corpus.rand(9, 40000)]
    comps = [flushed(d, [], fmt)[0] for d in datas] + [b"\x01\x02garbage", flushed(text(900), [], fmt)[0][:-9]]
    caps = [cap4(len(d)) + 4 for d in datas] + [64, 1000]
    try:
        engine.set_option("inflate_ref_wrap", 0)
        plain = engine.decompress_batch_detailed(comps, fmt, out_caps=caps)
    finally:
        engine.set_option("inflate_ref_wrap", 1)
    got = engine.decompress_batch_detailed(comps, fmt, out_caps=caps, restart=[[]] * len(comps))
    for k, (p, g) in enumerate(zip(plain, got)):
        if p[0] == 1:
            assert g == p, k
        else:  # (the reference's exact status for a broken stream is the plain entry's business)
            assert g == FAILED, k
    assert [p[0] for p in plain[:4]] == [1] * 4


def test_the_window_wrap_defect_is_not_reproduced_and_the_option_stays(engine):
    """option inflate_ref_wrap is left at 1 throughout: the plain entry yields the defect's bytes for the
    golden stream, before and after; the same source with a flush point decodes to the SOURCE here"""
    j = json.load(open(os.path.join(golden_io.GOLDEN, "inffast_wrap_defect.json")))
    src = corpus.make(j["source"])
    comp = oracle.compress(src, 6, "deflate-raw")[1]
    assert corpus.sha256(comp) == j["compressed_sha256"]

    def plain():
        (st, ph, msg, out, cons), = engine.decompress_batch_raw([comp], "deflate-raw", out_caps=[len(src) + 64])
        return st == 1 and corpus.sha256(out) == j["ref_out_sha256"] and out != src

    assert plain()
    # the golden stream itself, as one segment: zlib semantics, the source
    got = engine.decompress_batch_detailed([comp], "deflate-raw", out_caps=[len(src)], restart=[[]])
    assert got == [good(src, comp, "deflate-raw")]
    for ps in ([131072], [100001]):
        roundtrip(engine, "deflate-raw", [(src, ps)])
    assert plain()  # the option is still 1


def _stored_marker_case():
    """a point behind a 00 00 FF FF that is data inside a stored block"""
    d = corpus.rand(3, 600) + b"\x00\x00\xff\xff" + corpus.rand(4, 600)
    s = zlib.compress(d, 0)
    at = s.index(b"\x00\x00\xff\xff", 7)  # (behind the stored block's own LEN / NLEN)
    return d, s, [(at + 4, 604)]


def _flip(s, byte, bit=0):
    b = bytearray(s)
    b[byte] ^= 1 << bit
    return bytes(b)


def test_every_failure_is_the_one_failure(engine):
    d = text(20000, 6)
    z, zi = flushed(d, [8000], "deflate")
    g, gi = flushed(d, [8000], "gzip")
    r, ri = flushed(d, [8000], "deflate-raw")
    (a, o), = zi
    cap = cap4(len(d))
    for fmt, s, (a, o) in (("deflate", z, zi[0]), ("gzip", g, gi[0]), ("deflate-raw", r, ri[0])):
        bad = [[(a - 1, o)], [(a + 1, o)], [(a, o - 1)], [(a, o + 1)], [(a, o - 4)], [(a, o + 4)]]
        got = decode(engine, fmt, [(s, ps) for ps in bad] + [(s, [(a, o)])], [cap] * 7)
        assert got == [FAILED] * 6 + [good(d, s, fmt)], (fmt, [x[:3] for x in got])
    # a marker that is data
    sd, ss, sp = _stored_marker_case()
    assert decode(engine, "deflate", [(ss, sp), (ss, [])], [1208, 1208]) == [FAILED, good(sd, ss, "deflate")]
    # the trailers: adler32; crc32; ISIZE -- with and without restart points
    for fmt, s, idx, byte in (("deflate", z, zi, len(z) - 1), ("deflate", z, zi, len(z) - 4), ("gzip", g, gi, len(g) - 8),
                              ("gzip", g, gi, len(g) - 5), ("gzip", g, gi, len(g) - 4), ("gzip", g, gi, len(g) - 1)):
        f = _flip(s, byte, 3)
        assert decode(engine, fmt, [(f, idx), (f, []), (s, idx)], [cap] * 3) == [FAILED, FAILED, good(d, s, fmt)], (fmt, byte)
    # a zlib header with FDICT set (and the check mod 31 kept), a wrong method, a gzip header with a reserved flag
    fdict = bytearray(z)
    fdict[1] |= 0x20
    fdict[1] = (fdict[1] & 0xe0) | (31 - ((fdict[0] << 8) + (fdict[1] & 0xe0)) % 31) % 31
    assert ((fdict[0] << 8) + fdict[1]) % 31 == 0 and fdict[1] & 0x20
    assert decode(engine, "deflate", [(bytes(fdict), zi), (_flip(z, 0, 0), zi), (_flip(z, 1, 0), zi)], [cap] * 3) == [FAILED] * 3
    assert decode(engine, "gzip", [(_flip(g, 3, 7), gi), (_flip(g, 0, 0), gi), (_flip(g, 2, 0), gi)], [cap] * 3) == [FAILED] * 3
    # a truncated trailer, a last segment without its final block
    assert decode(engine, "gzip", [(g[:-1], gi), (g[:a + 20], gi)], [cap] * 2) == [FAILED] * 2


@pytest.mark.parametrize("fmt", FORMATS)
def test_capacity_short_is_the_plain_entrys_capacity_outcome(engine, fmt):
    d = text(20000, 6)
    s, idx = flushed(d, [8000], fmt)
    s1, idx1 = flushed(d, [8001], fmt)
    (pst, pph, pmsg, pout, _), = engine.decompress_batch_raw([s], fmt, out_caps=[len(d) - 1])
    assert (pst, pph, pmsg) == (-5, 0, "output capacity exceeded")
    caps = [len(d) - 1, len(d) - 1, 7999, 100, len(d), len(d)]
    got = decode(engine, fmt, [(s, idx), (s1, idx1), (s, idx), (s1, idx1), (s, idx), (s1, idx1)], caps)
    for g in got[:4]:
        assert g[:4] == (pst, pph, pmsg, b"") and g[5] == 0
    assert got[4:] == [good(d, s, fmt), good(d, s1, fmt)]


def test_the_device_entry_keeps_inside_its_regions_and_leaves_the_input(engine):
    import torch

    fmt = "gzip"
    datas = [text(30000, 1), text(5, 2), text(70001, 3), text(9000, 4), b""]
    points = [[4096, 20000], [1, 3], [65537], [4000], [0]]
    made = [flushed(d, ps, fmt) for d, ps in zip(datas, points)]
    made[3] = (made[3][0], [(made[3][1][0][0], 4001)])  # a wrong out_pos: this stream fails
    caps = [cap4(len(d)) for d in datas]
    caps[2] -= 4  # ... and this one does not fit
    C = 64  # canary bytes around the input and around every region
    blob = bytearray(b"\xa5" * C)
    in_off = []
    for s, _ in made:
        in_off.append(len(blob))
        blob += s
    blob += b"\xa5" * C
    out_off, o = [], C
    for c in caps:
        out_off.append(o)
        o += c + C
    n = len(made)
    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_out = torch.full((o,), 0x5a, dtype=torch.uint8, device="cuda")
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st, d_ph, d_msg, d_len, d_cons, d_chk = i32(), i32(), i32(), i32(), i32(), i32()
    engine.decompress_device(fmt, n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*in_off),
                             (ctypes.c_uint32 * n)(*[len(s) for s, _ in made]), d_out.data_ptr(),
                             (ctypes.c_uint64 * n)(*out_off), (ctypes.c_uint32 * n)(*caps), d_st.data_ptr(),
                             d_ph.data_ptr(), d_msg.data_ptr(), d_len.data_ptr(), d_cons.data_ptr(),
                             d_check=d_chk.data_ptr(), restart=[i for _, i in made], headers=[s[:32] for s, _ in made])
    torch.cuda.synchronize()
    assert bytes(d_in.cpu().numpy()) == bytes(blob)
    out = bytes(d_out.cpu().numpy())
    assert d_st.tolist() == [1, 1, -5, -3, 1] and d_len.tolist() == [30000, 5, 0, 0, 0]
    assert d_cons.tolist() == [len(made[0][0]), len(made[1][0]), 0, 0, len(made[4][0])]
    assert [x & 0xffffffff for x in d_chk.tolist()] == [zlib.crc32(datas[0]), zlib.crc32(datas[1]), 0, 0, 0]
    end = 0
    for k in range(n):
        assert out[end:out_off[k]] == b"\x5a" * (out_off[k] - end), k  # the canary in front of region k
        end = out_off[k] + caps[k]
        if d_st.tolist()[k] == 1:
            assert out[out_off[k]:out_off[k] + len(datas[k])] == datas[k], k
    assert out[end:] == b"\x5a" * C


def test_the_pool_decodes_from_restart_points(engine):
    import zsamd

    cases = [(text(40000 + 13 * k, k), list(range(5000 + k, 40000, 5000))) for k in range(5)] + [(b"abc", [1])]
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        for fmt in FORMATS:
            made = [flushed(d, ps, fmt) for d, ps in cases]
            got = pool.decompress_batch_detailed([s for s, _ in made], fmt, out_caps=[cap4(len(d)) for d, _ in cases],
                                                 restart=[i for _, i in made])
            assert got == [good(d, s, fmt) for (d, _), (s, _) in zip(cases, made)]
    finally:
        pool.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_last_flush_index_is_zlibs_index(engine, fmt):
    """9 streams with 0 .. 7 flush points through the host and the device entry: the index equals the
    cumulative lengths Python's zlib gives for the same pieces, and it decodes the engine's own stream"""
    import torch

    datas = [text(3000 + 997 * k, k) for k in range(9)]
    points = [sorted({(j * 3001) % (len(datas[k]) + 1) for j in range(k % 8)}) for k in range(9)]
    assert sorted(len(p) for p in points) == [0, 0, 1, 2, 3, 4, 5, 6, 7]
    want = [[a for a, _ in flushed(d, ps, fmt)[1]] for d, ps in zip(datas, points)]
    comps = engine.compress_batch(datas, fmt, 6, flush_at=points)
    assert engine.last_flush_index() == want
    got = engine.decompress_batch_detailed(comps, fmt, out_caps=[cap4(len(d)) for d in datas],
                                           restart=[list(zip(i, ps)) for i, ps in zip(want, points)])
    assert got == [good(d, c, fmt) for d, c in zip(datas, comps)]
    # the device entry
    import zsamd

    n = len(datas)
    blob = b"".join(datas)
    offs = [sum(len(d) for d in datas[:k]) for k in range(n)]
    caps = [cap4(zsamd.deflate_bound(len(d), fmt, n_flush=len(ps))) for d, ps in zip(datas, points)]
    ooff = [sum(caps[:k]) for k in range(n)]
    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_out = torch.zeros(sum(caps), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    engine.compress_device(6, fmt, n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*offs),
                           (ctypes.c_uint32 * n)(*[len(d) for d in datas]), d_out.data_ptr(), (ctypes.c_uint64 * n)(*ooff),
                           (ctypes.c_uint32 * n)(*caps), d_st.data_ptr(), d_len.data_ptr(), flush_at=points)
    assert engine.last_flush_index() == want
    assert d_st.tolist() == [1] * n and d_len.tolist() == [len(c) for c in comps]
    engine.compress_batch(datas[:2], fmt, 6)
    assert engine.last_flush_index() == []  # the last compress call had no flush point
    assert engine._L.zs_last_flush_index(engine.handle, None, 0) == 0
