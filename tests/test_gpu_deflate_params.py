"""GPU: deflateInit2_'s windowBits and memLevel (zs_deflate_batch_params*).  Every output is
compared with the committed goldens of C zlib 1.2.11 (tests/golden/deflate_params.json,
written by gen_deflate_params.py), never with the zlib of the machine the test runs on;
that zlib only decodes.  Every output also goes back through the engine's own inflate and
stays within deflateBound for its parameters.  One engine call has one (level, format,
window_bits, mem_level): a test runs its group's calls one after the other."""
import ctypes
import zlib

import pytest

import paramcases as cases

pytestmark = pytest.mark.gpu


def want_check(fmt, x):
    return {"deflate-raw": 1, "deflate": zlib.adler32(x), "gzip": zlib.crc32(x)}[fmt]


def run(engine, batch, **options):
    """batch: cases of one level, format, window_bits and mem_level; returns [(status, bytes, check)]"""
    _, _, level, fmt, wb, ml = batch[0]
    assert all(c[2:] == batch[0][2:] for c in batch)
    return engine.compress_batch_detailed([c[1] for c in batch], fmt, level, window_bits=wb, mem_level=ml)


def check(engine, batch, res):
    import zsamd

    g = cases.golden()
    fmt = batch[0][3]
    for (name, x, level, _, wb, ml), (st, out, chk) in zip(batch, res):
        assert st == zsamd.Z_STREAM_END, (name, st)
        assert cases.digest(out) == g[name], (name, len(out), g[name])
        assert chk == want_check(fmt, x), name
        assert len(out) <= cases.bound(len(x), fmt, wb, ml, level), name
        assert len(out) <= zsamd.lib().zs_deflate_bound_params(len(x), cases.wbits_code(fmt, wb), ml, level), name
        assert zlib.decompress(out, cases.wbits_code(fmt, max(wb, 9))) == x, name
    back = engine.decompress_batch([r[1] for r in res], fmt, [max(4, (len(c[1]) + 3) & ~3) for c in batch])
    assert back == [c[1] for c in batch]


def run_group(engine, name, keep=lambda c: True):
    calls = cases.by_call([c for c in cases.group(name) if keep(c)])
    assert calls
    for batch in calls:
        check(engine, batch, run(engine, batch))
    return calls


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_empty_and_tiny_inputs_in_every_window(engine, fmt):
    calls = run_group(engine, "tiny", lambda c: c[3] == fmt)
    assert {c[4] for b in calls for c in b} == set(cases.TINY_WINDOWS[fmt])


def test_zlib_header_carries_the_window(engine):
    for wb in range(8, 16):
        out = engine.compress_batch([b"abc"], "deflate", 6, window_bits=wb)[0]
        assert out[0] == 0x08 | (max(wb, 9) - 8) << 4 and (out[0] << 8 | out[1]) % 31 == 0, wb


@pytest.mark.parametrize("level", cases.HASH_LEVELS)
def test_every_hash_width(engine, level):
    """memLevel 1..9: at 9 the global-head instance (levels 1..3, window 15), the LDS-head one
    (window 12) and the two-pass link build (levels 4..9)"""
    calls = run_group(engine, "hash", lambda c: c[2] == level)
    assert {c[5] for b in calls for c in b} == set(range(1, 10))


@pytest.mark.parametrize("level", [1, 6])
def test_block_cut_at_lit_bufsize_minus_1_symbols(engine, level):
    run_group(engine, "cut", lambda c: c[2] == level)


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("wb", cases.SLIDE_WINDOWS)
def test_lengths_around_the_slides(engine, wb, level):
    run_group(engine, "slide", lambda c: c[2] == level and c[4] == wb)


@pytest.mark.parametrize("level", [1, 6])
@pytest.mark.parametrize("wb", cases.SLIDE_WINDOWS)
def test_distance_limit_and_the_nil_corner(engine, wb, level):
    for batch in cases.by_call([c for c in cases.group("dist") if c[2] == level and c[4] == wb]):
        res = run(engine, batch)
        check(engine, batch, res)
        for c, (_, out, _) in zip(batch, res):  # the cases are what they say: the match is found, or out of reach
            found, want = cases.dist_found(c, out)
            assert found == want, c[0]


def test_no_stored_block_once_its_start_slid_out(engine):
    calls = run_group(engine, "stored")
    g = cases.golden()
    size = {c[0]: g[c[0]][0] for b in calls for c in b}
    for level in (1, 6):
        at15 = size["stored/deflate-raw/l%d/w15/m8/rand40000" % level]
        assert at15 == 40015  # stored blocks
        for wb in (9, 12):  # dynamic blocks: larger than stored ones
            assert size["stored/deflate-raw/l%d/w%d/m8/rand40000" % (level, wb)] > at15
            # memLevel 1: 41,575 bytes under zs_deflate_bound_params = 41,588
            assert size["stored/deflate-raw/l%d/w%d/m1/rand40000" % (level, wb)] == 41575
    assert cases.bound(40000, "deflate-raw", 9, 1, 6) == 41588


@pytest.mark.parametrize("wb,ml", cases.LONG_PARAMS)
def test_long_streams(engine, wb, ml):
    run_group(engine, "long", lambda c: (c[4], c[5]) == (wb, ml))


def option_batch(level):
    """one non-default case set per level: slides, a NIL corner and text in one call (window 12, memLevel 4)"""
    xs = [c[1] for c in cases.group("slide") if c[2] == 6 and c[4] == 12][:6]
    xs += [c[1] for c in cases.group("dist") if c[2] == 6 and c[4] == 12][:6] + [x for _, x in cases.hash_inputs()]
    return xs


@pytest.mark.parametrize("option,values,level", [("fast_group", (0, 1), 1), ("fast_group", (0, 1), 3),
                                                 ("lane_order", (0, 1), 1), ("lane_order", (0, 1), 6),
                                                 ("parse_waves", (1, 2, 4), 6)])
def test_options_leave_the_bytes_unchanged(engine, option, values, level):
    xs = option_batch(level)
    want = [cases.compress(x, level, "deflate-raw", 12, 4) for x in xs] if zlib.ZLIB_RUNTIME_VERSION == "1.2.11" else None
    got = []
    try:
        for v in values:
            engine.set_option(option, v)
            got.append(engine.compress_batch(xs, "deflate-raw", level, window_bits=12, mem_level=4))
    finally:
        engine.set_option(option, 0 if option == "parse_waves" else 1)
    assert all(g == got[0] for g in got)
    assert want is None or got[0] == want


def test_pool_of_two_contexts_on_one_device_equals_one_context(engine):
    import zsamd

    xs = option_batch(6) * 3
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        assert len(pool.devices) == 2
        for fmt, level, wb, ml in (("deflate-raw", 1, 9, 1), ("deflate", 6, 12, 4), ("gzip", 9, 15, 9)):
            assert pool.compress_batch_detailed(xs, fmt, level, window_bits=wb, mem_level=ml) == \
                engine.compress_batch_detailed(xs, fmt, level, window_bits=wb, mem_level=ml), (fmt, level)
    finally:
        pool.close()


def test_device_entry(engine):
    """zs_deflate_batch_params_device on device buffers: inputs at odd offsets, canaries between the regions"""
    import torch
    import zsamd

    fmt, level, wb, ml = "deflate", 6, 12, 4
    xs = option_batch(6)
    n = len(xs)
    blob, offs, lens = zsamd._layout(xs)
    code = cases.wbits_code(fmt, wb)
    caps = [(int(zsamd.lib().zs_deflate_bound_params(len(x), code, ml, level)) + 3) & ~3 for x in xs]
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
                           window_bits=wb, mem_level=ml)
    torch.cuda.synchronize()
    st, ol, ck = [r.tolist() for r in res]
    raw = bytes(d_out.cpu().numpy())
    got = [(st[i], raw[ooffs[i]:ooffs[i] + ol[i]], ck[i] & 0xffffffff) for i in range(n)]
    assert got == engine.compress_batch_detailed(xs, fmt, level, window_bits=wb, mem_level=ml)
    inside = bytearray(len(raw))
    for a, c in zip(ooffs, caps):
        inside[a:a + c] = b"\1" * c
    assert all(b == 0xa5 for b, i in zip(raw, inside) if not i), "a byte outside [out_off, out_off + out_cap) changed"


def through_the_new_entry(engine, xs, fmt, level, wb, ml):
    import zsamd

    L = zsamd.lib()
    return zsamd._deflate_host(L, L.zs_deflate_batch_params, engine.handle, xs, fmt, level, engine._check,
                               params=(cases.wbits_code(fmt, wb), ml))


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_default_parameters_through_the_new_entry_are_the_ex_entry(engine, fmt):
    xs = option_batch(6)
    for level in (0, 1, 6, 9):
        assert through_the_new_entry(engine, xs, fmt, level, 15, 8) == engine.compress_batch_detailed(xs, fmt, level)


def test_refusals(engine):
    import zsamd

    with pytest.raises(zsamd.ZsError) as err:  # level 0 with other parameters is not built
        engine.compress_batch([b"abc"], "deflate", 0, window_bits=12)
    assert str(err.value) == "init failed: -2"
    for wb, ml in ((7, 8), (16, 8), (12, 0), (12, 10), (True, 8), (12, 8.0)):
        with pytest.raises(zsamd.ZsError) as err:
            engine.compress_batch([b"abc"], "deflate", 6, window_bits=wb, mem_level=ml)
        assert str(err.value) == "init failed: -2"
    for fmt, wbits in (("deflate-raw", -8), ("gzip", 24), ("deflate", 7), ("deflate", 16), ("gzip", 32)):
        with pytest.raises(zsamd.ZsError) as err:
            L = zsamd.lib()
            zsamd._deflate_host(L, L.zs_deflate_batch_params, engine.handle, [b"abc"], fmt, 6, engine._check,
                                params=(wbits, 8))
        assert str(err.value) == "init failed: -2" and err.value.msg == "invalid window bits"
    with pytest.raises(ValueError):
        engine.compress_batch([b"abc"], "deflate", 6, zdict=b"abc", window_bits=12)
    with pytest.raises(ValueError):
        engine.compress_batch([b"abc"], "deflate", 6, strategy=2, mem_level=4)
