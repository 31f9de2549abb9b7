"""GPU: the compression strategies (zs_deflate_batch_strategy*: Z_FILTERED,
Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED).  Every output is compared with the committed goldens
of C zlib 1.2.11 (tests/golden/deflate_strategy.json, written by
gen_deflate_strategy.py), never with the zlib of the machine the test runs on; that
zlib only decodes.  Every batch has at least 70 streams of mixed lengths, and every
output goes back through the engine's own inflate."""
import ctypes
import zlib

import pytest

import strategycases as cases

pytestmark = pytest.mark.gpu

MIN_BATCH = 70


def want_check(fmt, x):
    return {"deflate-raw": 1, "deflate": zlib.adler32(x), "gzip": zlib.crc32(x)}[fmt]


def padded(batch):
    """the batch, and its shortest cases again until MIN_BATCH streams run in one call"""
    small = sorted(batch, key=lambda c: len(c[1]))[:8]
    out = list(batch)
    while len(out) < MIN_BATCH:
        out.append(small[len(out) % len(small)])
    return out


def run(engine, batch, **options):
    """batch: cases of one level, format, strategy and rle_ref; returns [(status, bytes, check)]"""
    _, _, level, fmt, strategy, rle_ref = batch[0]
    assert all(c[2:] == batch[0][2:] for c in batch)
    options["rle_ref"] = rle_ref
    try:
        for k, v in options.items():
            engine.set_option(k, v)
        return engine.compress_batch_detailed([c[1] for c in batch], fmt, level, strategy=strategy)
    finally:
        for k in options:
            engine.set_option(k, 1)  # (the defaults of rle_ref and match_sweep)


def check(engine, batch, res):
    import zsamd

    g = cases.golden()
    fmt = batch[0][3]
    for (name, x, level, _, strategy, rle_ref), (st, out, chk) in zip(batch, res):
        assert st == zsamd.Z_STREAM_END, (name, st)
        assert cases.digest(out) == g[name], (name, len(out), g[name])
        assert chk == want_check(fmt, x), name
        assert len(out) <= zsamd.deflate_bound(len(x), fmt), name
        assert zlib.decompress(out, cases.W[fmt]) == x, name
    back = engine.decompress_batch([r[1] for r in res], fmt, [max(4, (len(c[1]) + 3) & ~3) for c in batch])
    assert back == [c[1] for c in batch]


@pytest.mark.parametrize("level", cases.HUFF_LEVELS)
@pytest.mark.parametrize("fmt", cases.FMTS)
def test_huffman_only(engine, fmt, level):
    batch = padded(cases.huff_cases(fmt, level))
    assert len(batch) >= MIN_BATCH and {len(c[1]) for c in batch} >= set(cases.HUFF_LENS)
    check(engine, batch, run(engine, batch))


@pytest.mark.parametrize("rle_ref", [0, 1])
def test_rle(engine, rle_ref):
    batch = padded(cases.rle_cases("deflate-raw", 6, rle_ref))
    check(engine, batch, run(engine, batch))


@pytest.mark.parametrize("rle_ref", [0, 1])
@pytest.mark.parametrize("fmt,level", [("deflate", 1), ("deflate", 9), ("gzip", 1), ("gzip", 9)])
def test_rle_wrappers(engine, fmt, level, rle_ref):
    batch = padded(cases.rle_cases(fmt, level, rle_ref)[:16])
    check(engine, batch, run(engine, batch))


def test_rle_ref_1_is_huffman_only(engine):
    xs = [c[1] for c in cases.rle_cases("deflate-raw", 6, 1)]
    for fmt in cases.FMTS:
        assert engine.compress_batch_detailed(xs, fmt, 6, strategy=cases.Z_RLE) == \
            engine.compress_batch_detailed(xs, fmt, 6, strategy=cases.Z_HUFFMAN_ONLY)


@pytest.mark.parametrize("match_sweep", [1, 0])
@pytest.mark.parametrize("level", cases.FILT_LEVELS)
def test_filtered(engine, level, match_sweep):
    batch = padded(cases.filtered_cases(level))  # 4 KiB, 64 KiB and 200,000 bytes (the windowed path) in one call
    res = run(engine, batch, match_sweep=match_sweep)
    check(engine, batch, res)
    plain = engine.compress_batch_detailed([c[1] for c in batch[:6]], "deflate-raw", level)
    assert all(a[1] != b[1] for a, b in zip(res, plain))


@pytest.mark.parametrize("level", [1, 2, 3])
def test_filtered_is_strategy_0_for_deflate_fast(engine, level):
    batch = padded(cases.filtered_fast_cases(level))
    res = run(engine, batch)
    check(engine, batch, res)
    assert res == engine.compress_batch_detailed([c[1] for c in batch], "deflate-raw", level)


@pytest.mark.parametrize("fmt,level", [("deflate-raw", 1), ("deflate-raw", 4), ("deflate-raw", 9), ("deflate", 6), ("gzip", 6)])
def test_fixed(engine, fmt, level):
    batch = padded(cases.fixed_cases(fmt, level))
    res = run(engine, batch)
    check(engine, batch, res)
    head = 0 if fmt == "deflate-raw" else 2 if fmt == "deflate" else 10
    types = {c[0].rsplit("/", 1)[1]: r[1][head] >> 1 & 3 for c, r in zip(batch, res)}
    assert types["text20000"] == 1 and types["zeros20000"] == 1 and types["rand20000"] == 0  # the stored choice survives


def through_the_new_entry(engine, xs, fmt, level, strategy):
    import zsamd

    L = zsamd.lib()
    return zsamd._deflate_host(L, L.zs_deflate_batch_strategy, engine.handle, xs, fmt, level, engine._check,
                               strategy=strategy)


def mixed_inputs():
    xs = [x for _, x in cases.huff_inputs()[:9]] + [x for _, x in cases.rle_inputs()[:40]] + [x for _, x in cases.fixed_inputs()]
    return xs + xs[:MIN_BATCH - len(xs)]


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_strategy_0_through_the_new_entry_is_the_ex_entry(engine, fmt):
    xs = mixed_inputs()
    assert len(xs) >= MIN_BATCH
    for level in (1, 6, 9):
        assert through_the_new_entry(engine, xs, fmt, level, 0) == engine.compress_batch_detailed(xs, fmt, level)


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_level_0_with_each_strategy_is_plain_level_0(engine, fmt):
    xs = mixed_inputs()
    plain = engine.compress_batch_detailed(xs, fmt, 0)
    for strategy in range(5):
        assert through_the_new_entry(engine, xs, fmt, 0, strategy) == plain, strategy
    for rle_ref in (0, 1):
        engine.set_option("rle_ref", rle_ref)
        try:
            assert through_the_new_entry(engine, xs, fmt, 0, cases.Z_RLE) == plain
        finally:
            engine.set_option("rle_ref", 1)


def test_invalid_arguments(engine):
    import zsamd

    for bad in (-1, 5):
        with pytest.raises(zsamd.ZsError) as err:
            through_the_new_entry(engine, [b"abc"], "deflate", 6, bad)
        assert str(err.value) == "init failed: -2" and err.value.msg == "invalid strategy"
        with pytest.raises(zsamd.ZsError) as err:
            engine.compress_batch([b"abc"], "deflate", 6, strategy=bad)
        assert str(err.value) == "init failed: -2"
    with pytest.raises(zsamd.ZsError) as err:
        engine.compress_batch([b"abc"], "deflate", 10, strategy=2)  # invalid level, as the plain entry
    assert str(err.value) == "init failed: -2" and err.value.msg == "invalid level"
    with pytest.raises(ValueError):
        engine.compress_batch([b"abc"], "deflate", 6, zdict=b"abc", strategy=2)


@pytest.mark.parametrize("strategy,rle_ref", [(1, 1), (2, 1), (3, 0), (4, 1)])
def test_short_capacity_is_buf_error_as_the_plain_entry(engine, strategy, rle_ref):
    """the host entry with exact capacities: one byte short is Z_BUF_ERROR, no length, no check value"""
    import zsamd

    L = zsamd.lib()
    fmt, level = "deflate", 6
    xs = [cases.runs(b"ab", (60, 700), cases.norun(900)), cases.huff_inputs()[4][1], b"", cases.norun(50)] * 18
    n = len(xs)
    engine.set_option("rle_ref", rle_ref)
    try:
        full = engine.compress_batch_detailed(xs, fmt, level, strategy=strategy)
        assert all(st == zsamd.Z_STREAM_END for st, _, _ in full)
        caps = [len(o) - (i % 2) for i, (_, o, _) in enumerate(full)]  # every other stream one byte short
        blob, offs, lens = zsamd._layout(xs)
        ooffs = [sum((c + 3) & ~3 for c in caps[:i]) for i in range(n)]
        out = ctypes.create_string_buffer(sum((c + 3) & ~3 for c in caps) + 4)
        st, ol, ck = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
        r = L.zs_deflate_batch_strategy(engine.handle, level, strategy, cases.W[fmt], n, blob, (ctypes.c_uint64 * n)(*offs),
                                        (ctypes.c_uint32 * n)(*lens), out, (ctypes.c_uint64 * n)(*ooffs),
                                        (ctypes.c_uint32 * n)(*caps), st, ol, ck)
        assert r == 0
    finally:
        engine.set_option("rle_ref", 1)
    for i in range(n):
        if i % 2:
            assert (st[i], ol[i], ck[i]) == (zsamd.Z_BUF_ERROR, 0, 0), i
        else:
            assert (st[i], ol[i], ck[i]) == (zsamd.Z_STREAM_END, len(full[i][1]), zlib.adler32(xs[i])), i
            assert out.raw[ooffs[i]:ooffs[i] + ol[i]] == full[i][1], i


def test_device_entry(engine):
    """zs_deflate_batch_strategy_device on device buffers: inputs at odd offsets, canaries between the regions"""
    import torch
    import zsamd

    fmt, level = "gzip", 9
    batch = padded(cases.huff_cases(fmt, level)[:8])
    xs = [c[1] for c in batch]
    n = len(xs)
    blob, offs, lens = zsamd._layout(xs)
    caps = [zsamd.deflate_capacity(len(x), fmt) for x in xs]
    ooffs, oo = [], 16
    for c in caps:
        ooffs.append(oo)
        oo += c + 16
    d_in = torch.frombuffer(bytearray(b"\xee" + blob + b"\0" * 16), dtype=torch.uint8).cuda()
    d_out = torch.full((oo,), 0xa5, dtype=torch.uint8, device="cuda")
    res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    engine.compress_device(level, fmt, n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*[o + 1 for o in offs]),
                           (ctypes.c_uint32 * n)(*lens), d_out.data_ptr(), (ctypes.c_uint64 * n)(*ooffs),
                           (ctypes.c_uint32 * n)(*caps), res[0].data_ptr(), res[1].data_ptr(), 0, res[2].data_ptr(),
                           strategy=cases.Z_HUFFMAN_ONLY)
    torch.cuda.synchronize()
    st, ol, ck = [r.tolist() for r in res]
    raw = bytes(d_out.cpu().numpy())
    check(engine, batch, [(st[i], raw[ooffs[i]:ooffs[i] + ol[i]], ck[i] & 0xffffffff) for i in range(n)])
    inside = bytearray(len(raw))
    for a, c in zip(ooffs, caps):
        inside[a:a + c] = b"\1" * c
    assert all(b == 0xa5 for b, i in zip(raw, inside) if not i), "a byte outside [out_off, out_off + out_cap) changed"


def test_pool_of_two_contexts_on_one_device_equals_one_context(engine):
    import zsamd

    xs = mixed_inputs()
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        assert len(pool.devices) == 2
        for strategy in range(5):  # (the pool's contexts keep rle_ref = 1)
            for fmt, level in (("deflate-raw", 6), ("gzip", 9)):
                assert pool.compress_batch_detailed(xs, fmt, level, strategy=strategy) == \
                    engine.compress_batch_detailed(xs, fmt, level, strategy=strategy), (strategy, fmt)
    finally:
        pool.close()
