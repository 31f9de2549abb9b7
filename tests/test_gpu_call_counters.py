"""GPU checks of the counters a context keeps of its last call (include/zs_gpu.h: zs_last_host_chunks,
zs_last_checksum_parts, zs_last_inflate_seg_count, zs_last_inflate_lane_count, zs_last_flush_index): each
belongs to the last call of its kind, whatever calls ran before it -- four-chunk host calls, device calls,
the raw segment batch a restart call nests, refused calls.  One engine per test, with host_chunk_min = 1
(64 streams run as four chunks: ZS_HOST_CHUNK_STREAMS) and the checksums cut into parts of 1024 bytes."""
import contextlib
import ctypes
import zlib

import pytest

import hostchunkcases as hc
import restartcases
from hostchunkcases import bounds, chunk_of
from test_gpu_checksum_split import parts_of

pytestmark = pytest.mark.gpu

N, PART = 64, 1024
OPTIONS = {"host_chunk_min": 1, "checksum_split": 1, "checksum_part": PART}


@contextlib.contextmanager
def fresh_engine(**more):
    import zsamd

    eng = zsamd.Engine()
    try:
        for k, v in {**OPTIONS, **more}.items():
            eng.set_option(k, v)
        yield eng
    finally:
        eng.close()


def small(i):
    """a filler of less than 4,000 bytes: 4,096 bytes of input make a member of a small batch a large one"""
    pool = [f for f in hc.fillers() if len(f) < 4000]
    return pool[(5 * i + i // 8) % len(pool)]


def smalls(n=N):
    return [small(i) for i in range(n)]


def counters(eng):
    buf = (ctypes.c_uint32 * 4096)()
    k = int(eng._L.zs_last_flush_index(eng.handle, buf, 4096))
    return {"chunks": eng.last_host_chunks(), "parts": eng.last_checksum_parts(), "segs": eng.last_seg_count(),
            "lanes": eng.last_lane_count(), "flush": list(buf[:k])}


def cap4(n):
    return (n + 3) & ~3


def device_inflate(eng, comp, fmt, caps, restart=None):
    """the device entry (caps: multiples of 4); restart: the points per stream, without the start"""
    import torch

    n = len(comp)
    blob, ioffs = hc._inputs(comp)
    d_in = torch.frombuffer(bytearray(blob + bytes(8)), dtype=torch.uint8).cuda()
    offs, at = [], 0
    for c in caps:
        offs.append(at)
        at += c
    d_out = torch.zeros(at + 8, dtype=torch.uint8, device="cuda")
    res = torch.full((6, n), -1, dtype=torch.int32, device="cuda")
    eng.decompress_device(fmt, n, d_in.data_ptr(), hc._u64(ioffs), hc._u32([len(c) for c in comp]), d_out.data_ptr(),
                          hc._u64(offs), hc._u32(caps), *[res[r].data_ptr() for r in range(5)], d_check=res[5].data_ptr(),
                          restart=restart, headers=None if restart is None else [c[:64] for c in comp])
    torch.cuda.synchronize()
    r, raw = res.cpu().tolist(), d_out.cpu().numpy().tobytes()
    return {"status": r[0], "data": [raw[o:o + ln] for o, ln in zip(offs, r[3])], "check": [v & 0xFFFFFFFF for v in r[5]]}


def device_deflate(eng, items, fmt, level):
    import torch

    n = len(items)
    blob, ioffs = hc._inputs(items)
    d_in = torch.frombuffer(bytearray(blob + bytes(8)), dtype=torch.uint8).cuda()
    caps = [cap4(int(eng._L.zs_deflate_bound(len(b), hc.engine_wbits(fmt)))) for b in items]
    offs, at = [], 0
    for c in caps:
        offs.append(at)
        at += c
    d_out = torch.zeros(at + 8, dtype=torch.uint8, device="cuda")
    res = torch.full((2, n), -1, dtype=torch.int32, device="cuda")
    eng.compress_device(level, fmt, n, d_in.data_ptr(), hc._u64(ioffs), hc._u32([len(b) for b in items]), d_out.data_ptr(),
                        hc._u64(offs), hc._u32(caps), res[0].data_ptr(), res[1].data_ptr())
    torch.cuda.synchronize()
    r, raw = res.cpu().tolist(), d_out.cpu().numpy().tobytes()
    return [raw[o:o + ln] for o, ln in zip(offs, r[1])]


def lens(items):
    return [len(b) for b in items]


def test_counters_belong_to_the_last_call_of_their_kind():
    # 1: the only members of more than 4,096 input bytes (the segmented decode's, in these small batches) in chunk 2
    items1 = smalls()
    items1[34], items1[41] = hc.edges()[3], hc.edges()[4]
    assert [chunk_of(N, i) for i in (34, 41)] == [2, 2]
    comp1 = [hc.deflated(d, "deflate", 6) for d in items1]
    assert [i for i in range(N) if len(comp1[i]) > 4096] == [34, 41]
    call1 = lambda e: hc.inflate(e, comp1, "deflate", lens(items1))
    # 2: a device call of small members
    items2 = smalls(9)
    comp2 = [hc.deflated(d, "deflate", 6) for d in items2]
    caps2 = [cap4(n) for n in lens(items2)]
    call2 = lambda e: device_inflate(e, comp2, "deflate", caps2)
    # 6: a host call of small gzip members
    items6 = smalls()[::-1]
    comp6 = [hc.deflated(d, "gzip", 1) for d in items6]
    call6 = lambda e: hc.inflate(e, comp6, "gzip", lens(items6))
    alone = []
    for call in (call1, call2, call6):
        with fresh_engine() as e:
            call(e)
            alone.append(counters(e))
    assert alone[0]["segs"] > 0 and alone[1]["segs"] == alone[2]["segs"] == 0
    assert all(a["lanes"] > 0 for a in alone)
    lanes1, lanes2, lanes6 = (a["lanes"] for a in alone)

    with fresh_engine() as eng:
        r = call1(eng)
        assert r["data"] == items1
        c1 = counters(eng)
        assert c1 == {"chunks": 4, "parts": parts_of(lens(items1), PART), "segs": alone[0]["segs"], "lanes": lanes1, "flush": []}
        r = call2(eng)
        assert r["data"] == items2 and r["status"] == [1] * 9
        c2 = counters(eng)
        assert c2 == {"chunks": 0, "parts": parts_of(caps2, PART), "segs": 0, "lanes": lanes2, "flush": []}
        # 3: a checksum entry: the parts are its own; the chunks, segs and lanes stay the inflate call's
        bufs = [items1[34], b"", small(3)]
        assert eng.crc32(bufs) == [zlib.crc32(b) for b in bufs]
        assert counters(eng) == dict(c2, parts=parts_of(lens(bufs), PART))
        # 4: a host compress call with flush points in chunk 1 only
        items4 = smalls()
        per = [[len(d) // 2] if chunk_of(N, i) == 1 else [] for i, d in enumerate(items4)]
        r = hc.deflate(eng, items4, "gzip", 6, flush=per)
        assert r["data"] == [hc.deflated(d, "gzip", 6, flush=tuple(ps)) for d, ps in zip(items4, per)]
        want_idx = [x for d, ps in zip(items4, per) for x in hc.flush_index(d, "gzip", 6, ps)]
        assert len(want_idx) == bounds(N)[2] - bounds(N)[1]
        assert counters(eng) == {"chunks": 4, "parts": parts_of(lens(items4), PART), "segs": 0, "lanes": lanes2, "flush": want_idx}
        # 5: a device compress call without flush points (zlib: its check values count their own parts)
        assert device_deflate(eng, items2, "deflate", 6) == [hc.deflated(d, "deflate", 6) for d in items2]
        assert counters(eng) == {"chunks": 0, "parts": parts_of(lens(items2), PART), "segs": 0, "lanes": lanes2, "flush": []}
        r = call6(eng)
        assert r["data"] == items6
        assert counters(eng) == {"chunks": 4, "parts": parts_of(lens(items6), PART), "segs": 0, "lanes": lanes6, "flush": []}


def restart_batch(fmt):
    """64 streams of 3 checksum parts and four of 200, each with a few restart points -- multiples of 4 in
    chunks 0 and 3 (decoded in place), any residue in chunks 1 and 2 (the staging route)"""
    items = [hc.fillers()[2 + i % 4][:2049 + (37 * i) % 1000] for i in range(N)]
    for j, i in enumerate((3, 20, 40, 60)):
        items[i] = restartcases.text(199 * PART + 1 + j, 40 + j)
    pts = []
    for i, d in enumerate(items):
        ps = [len(d) // 4 + 1, len(d) // 2 + 2, len(d) - 5]
        pts.append(sorted({p & ~3 for p in ps}) if chunk_of(N, i) in (0, 3) else ps)
    assert {-(-len(d) // PART) for d in items} == {3, 200}
    assert any(p % 4 for i in range(bounds(N)[1], bounds(N)[3]) for p in pts[i])
    made = [restartcases.flushed(d, ps, fmt) for d, ps in zip(items, pts)]
    return items, [s for s, _ in made], [idx for _, idx in made]


@pytest.mark.parametrize("fmt", ["gzip", "deflate"])
def test_restart_with_a_checksum_in_parts(fmt):
    items, comp, idx = restart_batch(fmt)
    header = 10 if fmt == "gzip" else 2
    with_start = [[(header, 0)] + ix for ix in idx]
    checks = [restartcases.check_value(d, fmt) for d in items]
    with fresh_engine() as eng:
        caps = [cap4(n) for n in lens(items)]
        r = device_inflate(eng, comp, fmt, caps, restart=idx)
        assert r["status"] == [1] * N and r["data"] == items and r["check"] == checks
        assert eng.last_checksum_parts() == parts_of(caps, PART) and eng.last_host_chunks() == 0
        for chunk_min, chunks in ((0, 1), (1, 4)):
            eng.set_option("host_chunk_min", chunk_min)
            r = hc.inflate(eng, comp, fmt, lens(items), restart=with_start)
            assert r["status"] == [1] * N and r["data"] == items and r["check"] == checks
            assert eng.last_host_chunks() == chunks
            assert eng.last_checksum_parts() == parts_of(lens(items), PART) == 60 * 3 + 4 * 200
        # a raw call has no checksum: no parts, through either entry
        few = items[:9]
        made = [restartcases.flushed(d, [len(d) // 2], "deflate-raw") for d in few]
        r = hc.inflate(eng, [s for s, _ in made], "deflate-raw", lens(few), restart=[[(0, 0)] + ix for _, ix in made])
        assert r["data"] == few and eng.last_checksum_parts() == 0
        r = device_inflate(eng, [s for s, _ in made], "deflate-raw", [cap4(n) for n in lens(few)], restart=[ix for _, ix in made])
        assert r["data"] == few and eng.last_checksum_parts() == 0
        # ... and a plain gzip call behind it counts its own
        r = hc.inflate(eng, [hc.deflated(d, "gzip", 6) for d in few], "gzip", lens(few))
        assert r["data"] == few and eng.last_checksum_parts() == parts_of(lens(few), PART) == 8 * 3 + 200


def test_a_refused_call_between_two_good_ones():
    """A refused call has not begun, and neither has an empty one: the counters stay what the good call before
    it left (a four-chunk host call's 4 chunks too, behind an empty device call), and the good call behind it
    reports what the good call before it did -- the compress call's counters too, whose lane and seg counts
    are the last inflate batch's.  (Before call_begin a device decode refused for its alignment had already
    cleared "a segmented launch has run", and the seg count read 0 behind it.)"""
    items = smalls()
    items[34] = hc.edges()[3]
    comp = [hc.deflated(d, "deflate", 6) for d in items]
    per = [[len(d) // 3] if i % 2 else [] for i, d in enumerate(items)]
    with fresh_engine() as eng:
        L, h = eng._L, eng.handle

        def good_inflate():
            assert hc.inflate(eng, comp, "deflate", lens(items))["data"] == items
            return counters(eng)

        def good_deflate():
            hc.deflate(eng, items, "gzip", 1, flush=per)
            return counters(eng)

        a = (ctypes.c_uint32 * 1)(8)
        o = (ctypes.c_uint64 * 1)(2)
        z32, z64 = hc._u32([]), hc._u64([])
        not_begun = [
            # a host decode with windowBits 14; a device decode with an offset of 2; a host compress of level 11
            (-2, lambda: L.zs_inflate_batch_ex(h, 14, 1, b"\x03\x00", hc._u64([0]), hc._u32([2]), None, o, a, *[None] * 6)),
            (-2, lambda: L.zs_inflate_batch_device(h, -15, 1, None, hc._u64([0]), hc._u32([2]), None, o, a, *[None] * 6)),
            (-2, lambda: L.zs_deflate_batch_ex(h, 11, 31, 1, b"ab", hc._u64([0]), hc._u32([2]), None, o, a, None, None, None)),
            # empty batches: a device decode, a device compress, a host decode, a host compress
            (0, lambda: L.zs_inflate_batch_device(h, 15, 0, None, z64, z32, None, z64, z32, *[None] * 6)),
            (0, lambda: L.zs_deflate_batch_device_ex(h, 6, 15, 0, None, z64, z32, None, z64, z32, None, None, None, None)),
            (0, lambda: L.zs_inflate_batch_ex(h, 15, 0, b"", z64, z32, None, z64, z32, *[None] * 6)),
            (0, lambda: L.zs_deflate_batch_ex(h, 6, 15, 0, b"", z64, z32, None, z64, z32, None, None, None)),
        ]
        for good in (good_inflate, good_deflate):
            first = good()
            assert first["chunks"] == 4 and first["parts"] == parts_of(lens(items), PART)
            for rc, call in not_begun:
                assert call() == rc
                assert counters(eng) == first
                assert good() == first
        assert first["flush"] and good_inflate()["segs"] > 0
