"""GPU: compressing against a preset dictionary (zs_deflate_batch_dict*, raw deflate
and zlib, levels 1..9).  Every output is compared with the committed goldens of C
zlib 1.2.11 (tests/golden/deflate_dict.json, written by gen_deflate_dict.py), never
with the zlib of the machine the test runs on; that zlib only decodes."""
import ctypes
import zlib

import pytest

import deflatedictcases as cases
import dictcases

pytestmark = pytest.mark.gpu

W = dictcases.W


def want_check(fmt, x):
    return zlib.adler32(x) if fmt == "deflate" else 1


def run(engine, batch, **kw):
    """batch: [(name, data, dictionary, level, fmt)] of one level and format; returns [(status, bytes, check)]"""
    level, fmt = batch[0][3], batch[0][4]
    assert all(c[3] == level and c[4] == fmt for c in batch)
    return engine.compress_batch_detailed([c[1] for c in batch], fmt, level, zdict=[c[2] for c in batch], **kw)


def check_golden(batch, res):
    import zsamd

    g = cases.golden()
    for (name, x, d, level, fmt), (st, out, chk) in zip(batch, res):
        assert st == zsamd.Z_STREAM_END, (name, st)
        assert cases.digest(out) == g[name], (name, len(out), g[name])
        assert chk == want_check(fmt, x), name
        assert len(out) <= zsamd.deflate_bound(len(x), fmt, len(d or b"")), name


def check_python_decodes(batch, res):
    for (name, x, d, level, fmt), (st, out, chk) in zip(batch, res):
        o = zlib.decompressobj(W[fmt], d) if d else zlib.decompressobj(W[fmt])
        assert o.decompress(out) == x and o.eof and not o.unused_data, name


def check_round_trip(engine, batch, res):
    fmt = batch[0][4]
    got = engine.decompress_batch([r[1] for r in res], fmt, [dictcases.cap4(len(c[1])) for c in batch],
                                  zdict=[c[2] for c in batch])
    assert got == [c[1] for c in batch]


@pytest.mark.parametrize("fmt", cases.FMTS)
@pytest.mark.parametrize("L", dictcases.DICT_LENS)
def test_small_records(engine, L, fmt):
    for level in cases.LEVELS:
        batch = cases.set1(fmt, level, L)
        res = run(engine, batch)
        check_golden(batch, res)
        check_python_decodes(batch, res)
        check_round_trip(engine, batch, res)


@pytest.mark.parametrize("level", cases.CORNER_LEVELS)
def test_window_slide_and_block_corners(engine, level):
    batch = cases.set2(level)
    res = run(engine, batch)
    check_golden(batch, res)
    check_python_decodes(batch, res)


def mixed_run(engine, fmt, level):
    """set 3 through zs_deflate_batch_dict itself: one dictionary buffer, the blob's slices at
    odd byte offsets and aliased among the streams.  Returns [(status, bytes, check)]."""
    import zsamd

    L = zsamd.lib()
    xs = cases.mixed_inputs()
    n = len(xs)
    d257, d32k, blob = dictcases.dictionary(257), dictcases.dictionary(32768), cases.mixed_blob()
    dbuf = b"\xee" + d257 + d32k + blob  # (every dictionary at an odd byte offset)
    doff, dlen = [], []
    for k in range(n):
        d = cases.mixed_dict(k)
        if d is None:
            doff.append(0), dlen.append(0)
        elif isinstance(d, tuple):
            doff.append(1 + 257 + 32768 + d[1]), dlen.append(d[2])
        else:
            doff.append(1 if len(d) == 257 else 1 + 257), dlen.append(len(d))
    blob_in, offs, lens = zsamd._layout(xs)
    caps = [zsamd.deflate_capacity(len(x), fmt, dl) for x, dl in zip(xs, dlen)]
    ooffs = [sum(caps[:i]) for i in range(n)]
    out = ctypes.create_string_buffer(sum(caps))
    status, olen, chk = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    r = L.zs_deflate_batch_dict(engine.handle, level, zsamd.compress_wbits(fmt), n, blob_in,
                                (ctypes.c_uint64 * n)(*offs), (ctypes.c_uint32 * n)(*lens), out,
                                (ctypes.c_uint64 * n)(*ooffs), (ctypes.c_uint32 * n)(*caps), status, olen, chk, dbuf,
                                (ctypes.c_uint64 * n)(*doff), (ctypes.c_uint32 * n)(*dlen))
    assert r == 0, L.zs_last_error()
    return [(status[i], out.raw[ooffs[i]:ooffs[i] + olen[i]], chk[i]) for i in range(n)]


@pytest.mark.parametrize("fmt", cases.FMTS)
@pytest.mark.parametrize("level", cases.MIXED_LEVELS)
def test_mixed_batch(engine, level, fmt):
    batch = cases.set3(fmt, level)
    res = mixed_run(engine, fmt, level)
    check_golden(batch, res)
    check_python_decodes(batch, res)
    check_round_trip(engine, batch, res)
    assert run(engine, batch) == res  # the Python entry (equal dictionaries stored once)
    # the streams without a dictionary: the plain entry's bytes
    plain = engine.compress_batch([c[1] for c in batch[0::4]], fmt, level)
    assert [r[1] for r in res[0::4]] == plain


OPTIONS = [("match_sweep", 0, 1), ("fast_group", 0, 1), ("parse_waves", 1, 0), ("parse_waves", 2, 0),
           ("parse_waves", 4, 0), ("lane_order", 0, 1)]


@pytest.mark.parametrize("level", cases.CORNER_LEVELS)
def test_option_paths(engine, level):
    """every input kind of set 2 against the 32,768-byte dictionary, and the split inputs"""
    batch = [c for c in cases.set2(level) if "/d32768/" in c[0] or "/split/" in c[0]]
    base = run(engine, batch)
    check_golden(batch, base)
    for name, value, default in OPTIONS:
        engine.set_option(name, value)
        try:
            got = run(engine, batch)
        finally:
            engine.set_option(name, default)
        assert got == base, (name, value)


def test_boundary(engine):
    import zsamd

    d = dictcases.dictionary(257)
    xs = list(cases.small_inputs()[12:])  # four records, then 0, 1, 2 and 3 bytes
    # gzip, and level 0, with a dictionary: the call fails as the stream layer's init does
    pool = zsamd.Pool([0])
    try:
        for e in (engine, pool):
            for fmt, level, word in (("gzip", 6, "deflate-raw"), ("deflate", 0, "level 0")):
                with pytest.raises(zsamd.ZsError) as err:
                    e.compress_batch_detailed(xs, fmt, level, zdict=d)
                assert err.value.status == zsamd.Z_STREAM_ERROR and str(err.value) == "init failed: -2"
                assert word in err.value.msg, err.value.msg
                # ... but not when no stream has one: exactly the plain entry's results
                assert e.compress_batch_detailed(xs, fmt, level, zdict=[None, b""] * 4) == \
                    e.compress_batch_detailed(xs, fmt, level)
        # a one-device pool equals the engine
        for fmt in cases.FMTS:
            zd = [d if i % 2 else None for i in range(8)]
            assert pool.compress_batch_detailed(xs, fmt, 6, zdict=zd) == engine.compress_batch_detailed(xs, fmt, 6, zdict=zd)
    finally:
        pool.close()
    with pytest.raises(zsamd.ZsError):
        engine.compress_batch_detailed(xs, "deflate", 10, zdict=d)  # invalid level, as the plain entry
    # all dict_len zero: the plain entry's bytes
    for fmt in cases.FMTS:
        assert engine.compress_batch_detailed(xs, fmt, 6, zdict=[None] * 8) == engine.compress_batch_detailed(xs, fmt, 6)
    # a 64-byte capacity: Z_BUF_ERROR, nothing produced (the device entry)
    import torch

    n = len(xs)
    blob, offs, lens = zsamd._layout(xs)
    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_dict = torch.frombuffer(bytearray(b"\xee" + d), dtype=torch.uint8).cuda()
    d_out = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    engine.compress_device(6, "deflate", n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*offs), (ctypes.c_uint32 * n)(*lens),
                           d_out.data_ptr(), (ctypes.c_uint64 * n)(*[64 * i for i in range(n)]),
                           (ctypes.c_uint32 * n)(*[64] * n), res[0].data_ptr(), res[1].data_ptr(), 0, res[2].data_ptr(),
                           d_dict.data_ptr(), (ctypes.c_uint64 * n)(*[1] * n), (ctypes.c_uint32 * n)(*[257] * n))
    torch.cuda.synchronize()
    g = cases.golden()
    want = [g["s1/deflate/l6/d257/i%d" % (12 + i)] for i in range(n)]
    for i in range(n):
        st, ol, ck = res[0][i].item(), res[1][i].item(), res[2][i].item() & 0xffffffff
        if want[i][0] <= 64:
            assert (st, ol, ck) == (zsamd.Z_STREAM_END, want[i][0], zlib.adler32(xs[i])), i
            assert cases.digest(bytes(d_out[64 * i:64 * i + ol].cpu().numpy())) == want[i], i
        else:
            assert (st, ol, ck) == (zsamd.Z_BUF_ERROR, 0, 0), i
    assert any(w[0] > 64 for w in want) and any(w[0] <= 64 for w in want)


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_device_entry_keeps_to_its_regions(engine, fmt):
    """set 3 through zs_deflate_batch_dict_device: dictionaries at odd byte offsets of one device
    buffer, every output region of exactly zs_deflate_bound_dict (rounded to 4) between canaries"""
    import torch
    import zsamd

    level = 6
    batch = cases.set3(fmt, level)
    xs = [c[1] for c in batch]
    n = len(xs)
    d257, d32k, blob = dictcases.dictionary(257), dictcases.dictionary(32768), cases.mixed_blob()
    doff, dlen = [], []
    for k in range(n):
        d = cases.mixed_dict(k)
        if d is None:
            doff.append(0), dlen.append(0)
        elif isinstance(d, tuple):
            doff.append(3 + 257 + 32768 + d[1]), dlen.append(d[2])
        else:
            doff.append(3 if len(d) == 257 else 3 + 257), dlen.append(len(d))
    in_blob, offs, lens = zsamd._layout(xs)
    caps = [zsamd.deflate_capacity(len(x), fmt, dl) for x, dl in zip(xs, dlen)]
    ooffs, oo = [], 16
    for c in caps:
        ooffs.append(oo)
        oo += c + 16  # 16 canary bytes between the regions (offsets stay multiples of 4)
    d_in = torch.frombuffer(bytearray(b"\xee" + in_blob + b"\0" * 16), dtype=torch.uint8).cuda()
    d_dict = torch.frombuffer(bytearray(b"\xee" * 3 + d257 + d32k + blob + b"\xee" * 16), dtype=torch.uint8).cuda()
    d_out = torch.full((oo,), 0xa5, dtype=torch.uint8, device="cuda")
    res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    engine.compress_device(level, fmt, n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*[o + 1 for o in offs]),
                           (ctypes.c_uint32 * n)(*lens), d_out.data_ptr(), (ctypes.c_uint64 * n)(*ooffs),
                           (ctypes.c_uint32 * n)(*caps), res[0].data_ptr(), res[1].data_ptr(), 0, res[2].data_ptr(),
                           d_dict.data_ptr(), (ctypes.c_uint64 * n)(*doff), (ctypes.c_uint32 * n)(*dlen))
    torch.cuda.synchronize()
    st, ol, ck = [r.tolist() for r in res]
    raw = bytes(d_out.cpu().numpy())
    check_golden(batch, [(st[i], raw[ooffs[i]:ooffs[i] + ol[i]], ck[i] & 0xffffffff) for i in range(n)])
    inside = bytearray(len(raw))
    for a, c in zip(ooffs, caps):
        inside[a:a + c] = b"\1" * c
    assert all(b == 0xa5 for b, i in zip(raw, inside) if not i), "a byte outside [out_off, out_off + out_cap) changed"
