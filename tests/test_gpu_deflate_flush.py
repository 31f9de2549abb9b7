"""GPU: Z_FULL_FLUSH points (zs_deflate_batch_flush*).  Every output is compared with the committed
goldens of C zlib 1.2.11 (tests/golden/deflate_flush.json, written by gen_deflate_flush.py), never
with the zlib of the machine the test runs on; that zlib only decodes.  Every output also goes back
through the engine's own inflate, stays within zs_deflate_bound_flush, and a deflate-raw output
inflates from behind each marker to the rest of its data.  One engine call has one level and
format: a test runs its group's calls one after the other."""
import ctypes
import zlib

import pytest

import flushcases as cases

pytestmark = pytest.mark.gpu


def want_check(fmt, x):
    return {"deflate-raw": 1, "deflate": zlib.adler32(x), "gzip": zlib.crc32(x)}[fmt]


def run(engine, batch):
    """batch: cases of one level and format; returns [(status, bytes, check)]"""
    _, _, level, fmt, _ = batch[0]
    assert all(c[2:4] == batch[0][2:4] for c in batch)
    return engine.compress_batch_detailed([c[1] for c in batch], fmt, level, flush_at=[list(c[4]) for c in batch])


def check(engine, batch, res):
    import zsamd

    g = cases.golden()
    fmt = batch[0][3]
    for (name, x, level, _, pos), (st, out, chk) in zip(batch, res):
        assert st == zsamd.Z_STREAM_END, (name, st)
        assert cases.digest(out) == g[name][:2], (name, len(out), g[name][:2])
        assert chk == want_check(fmt, x), name
        assert len(out) <= zsamd.deflate_bound(len(x), fmt, n_flush=len(pos)) == cases.bound(len(x), fmt, len(pos)), name
        assert zlib.decompress(out, cases.WBITS[fmt]) == x, name
        if fmt == "deflate-raw":  # a decoder restarts behind every marker
            for off, p in zip(g[name][2], pos):
                assert out[off - 4:off] == cases.MARKER and zlib.decompress(out[off:], -15) == x[p:], (name, p)
    back = engine.decompress_batch([r[1] for r in res], fmt, [max(4, (len(c[1]) + 3) & ~3) for c in batch])
    assert back == [c[1] for c in batch]


def run_group(engine, name, keep=lambda c: True):
    calls = cases.by_call([c for c in cases.group(name) if keep(c)])
    assert calls
    for batch in calls:
        check(engine, batch, run(engine, batch))
    return calls


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_every_subset_of_positions_in_three_bytes(engine, fmt):
    calls = run_group(engine, "tiny", lambda c: c[3] == fmt)
    assert sum(len(b) for b in calls) == 2 * 18


def test_a_flush_at_0_and_at_the_end_write_the_marker_alone(engine):
    out = engine.compress_batch([b"abc", b"abc", b""], "deflate-raw", 6, flush_at=[[0], [3], [0]])
    plain = engine.compress_batch([b"abc"], "deflate-raw", 6)[0]
    assert out[0] == b"\x00" + cases.MARKER + plain
    assert out[1].endswith(cases.MARKER + b"\x03\x00") and out[1][0] & 1 == 0  # BFINAL in the last block alone
    assert out[2] == b"\x00" + cases.MARKER + b"\x03\x00"


@pytest.mark.parametrize("level", [1, 6])
def test_a_piece_that_ends_on_the_symbol_cut_drops_its_empty_block(engine, level):
    run_group(engine, "cut", lambda c: c[2] == level)
    if level == 1:  # filler(16383): finished alone one block more than flushed
        import deflate_header

        x = cases.filler(16383)
        alone = engine.compress_batch([x], "deflate-raw", 1)[0]
        flushed = engine.compress_batch([x + b"tail"], "deflate-raw", 1, flush_at=[16383])[0]
        assert [b.type for b in deflate_header.parse(alone)][1:] == [1]
        assert [b.type for b in deflate_header.parse(flushed)][1:] == [0, 1]


@pytest.mark.parametrize("level", [1, 6])
def test_segments_share_output_words_at_every_byte_phase(engine, level):
    run_group(engine, "seams", lambda c: c[2] == level)


def test_stored_blocks_align_inside_their_segment(engine):
    run_group(engine, "stored")


@pytest.mark.parametrize("level", cases.WINDOW_LEVELS)
def test_segments_of_one_and_of_several_sweep_windows(engine, level):
    run_group(engine, "windows", lambda c: c[2] == level)


def test_256_segments_of_one_stream(engine):
    run_group(engine, "many")


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_streams_with_0_1_and_7_flush_points_in_one_call(engine, fmt):
    calls = run_group(engine, "mixed", lambda c: c[3] == fmt)
    for batch in calls:  # the ones without points: the _ex entry's bytes
        level = batch[0][2]
        res = run(engine, batch)
        plain = engine.compress_batch_detailed([c[1] for c in batch if not c[4]], fmt, level)
        assert [r for c, r in zip(batch, res) if not c[4]] == plain


def option_batch():
    return [c for c in cases.group("mixed") if c[3] == "deflate-raw" and c[2] == 6] + \
        [c for c in cases.group("seams") if c[3] == "deflate-raw" and c[2] == 6]


def test_no_flush_points_through_the_new_entry_are_the_ex_entry(engine):
    xs = [c[1] for c in option_batch()]
    for fmt in cases.FMTS:
        for level in (0, 1, 6):
            assert engine.compress_batch_detailed(xs, fmt, level, flush_at=[]) == \
                engine.compress_batch_detailed(xs, fmt, level), (fmt, level)


def test_a_capacity_one_byte_short_is_a_buf_error_for_that_stream_alone(engine):
    import zsamd

    L = zsamd.lib()
    batch = [c for c in cases.group("mixed") if c[3] == "gzip" and c[2] == 6]
    g = cases.golden()
    n = len(batch)
    blob, offs, lens = zsamd._layout([c[1] for c in batch])
    short = 3  # the stream with seven flush points
    assert len(batch[short][4]) == 7
    caps = [g[c[0]][0] - (1 if i == short else 0) for i, c in enumerate(batch)]  # exact capacities: the host entry takes any
    ooffs = [sum((c + 3) & ~3 for c in caps[:i]) for i in range(n)]
    out = ctypes.create_string_buffer(sum((c + 3) & ~3 for c in caps) + 4)
    status, olen, chk = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    first, pos = zsamd._flush_arrays([list(c[4]) for c in batch])
    r = L.zs_deflate_batch_flush(engine.handle, 6, 31, n, blob, zsamd._arr(ctypes.c_uint64, offs),
                                 zsamd._arr(ctypes.c_uint32, lens), out, zsamd._arr(ctypes.c_uint64, ooffs),
                                 zsamd._arr(ctypes.c_uint32, caps), status, olen, chk, zsamd.Z_FULL_FLUSH, first, pos)
    assert r == 0
    for i, c in enumerate(batch):
        if i == short:
            assert (status[i], olen[i], chk[i]) == (zsamd.Z_BUF_ERROR, 0, 0)
        else:
            assert status[i] == zsamd.Z_STREAM_END and cases.digest(out.raw[ooffs[i]:ooffs[i] + olen[i]]) == g[c[0]][:2]


def test_device_entry(engine):
    """zs_deflate_batch_flush_device on device buffers: inputs at odd offsets, canaries between the regions"""
    import torch
    import zsamd

    fmt, level = "deflate", 6
    batch = [c for c in cases.group("mixed") if c[3] == fmt and c[2] == level] + \
        [c for c in cases.group("seams") if c[3] == fmt and c[2] == level]
    xs, per = [c[1] for c in batch], [list(c[4]) for c in batch]
    n = len(xs)
    blob, offs, lens = zsamd._layout(xs)
    caps = [(zsamd.deflate_bound(len(x), fmt, n_flush=len(p)) + 3) & ~3 for x, p in zip(xs, per)]
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
                           flush_at=per)
    torch.cuda.synchronize()
    st, ol, ck = [r.tolist() for r in res]
    raw = bytes(d_out.cpu().numpy())
    got = [(st[i], raw[ooffs[i]:ooffs[i] + ol[i]], ck[i] & 0xffffffff) for i in range(n)]
    g = cases.golden()
    assert [cases.digest(o) for _, o, _ in got] == [g[c[0]][:2] for c in batch]
    assert got == engine.compress_batch_detailed(xs, fmt, level, flush_at=per)
    inside = bytearray(len(raw))
    for a, c in zip(ooffs, caps):
        inside[a:a + c] = b"\1" * c
    assert all(b == 0xa5 for b, i in zip(raw, inside) if not i), "a byte outside [out_off, out_off + out_cap) changed"


@pytest.mark.parametrize("option,values,level", [("match_sweep", (0, 1), 6), ("fast_group", (0, 1), 1),
                                                 ("lane_order", (0, 1), 1), ("lane_order", (0, 1), 6),
                                                 ("parse_waves", (1, 2, 4), 6)])
def test_options_leave_the_bytes_unchanged(engine, option, values, level):
    batch = [c for c in cases.group("mixed") + cases.group("seams") + cases.group("windows")[:2]
             if c[3] == "deflate-raw" and c[2] == level]
    assert len(batch) >= 9
    g = cases.golden()
    try:
        for v in values:
            engine.set_option(option, v)
            res = run(engine, batch)
            assert [cases.digest(o) for _, o, _ in res] == [g[c[0]][:2] for c in batch], (option, v)
    finally:
        engine.set_option(option, 0 if option == "parse_waves" else 1)


def test_pool_of_two_contexts_on_one_device_equals_one_context(engine):
    import zsamd

    batch = option_batch() * 2
    xs, per = [c[1] for c in batch], [list(c[4]) for c in batch]
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        assert len(pool.devices) == 2
        for fmt, level in (("deflate-raw", 1), ("deflate", 6), ("gzip", 9)):
            assert pool.compress_batch_detailed(xs, fmt, level, flush_at=per) == \
                engine.compress_batch_detailed(xs, fmt, level, flush_at=per), (fmt, level)
        assert pool.compress_batch(xs, "gzip", 6, flush_every=100) == engine.compress_batch(xs, "gzip", 6, flush_every=100)
    finally:
        pool.close()


def test_flush_every(engine):
    x = cases.group("many")[0][1][:20000]
    assert engine.compress_batch([x, x[:4096], b""], "gzip", 6, flush_every=4096) == \
        engine.compress_batch([x, x[:4096], b""], "gzip", 6, flush_at=[[4096, 8192, 12288, 16384], [], []])


def flush_call(engine, xs, per, level=6, wbits=-15, flush=3, first=True, pos=True):
    """zs_deflate_batch_flush as given; returns (return code, zs_last_error())"""
    import zsamd

    L = zsamd.lib()
    n = len(xs)
    blob, offs, lens = zsamd._layout(xs)
    caps = [(len(x) + 200 + 12 * len(p) + 3) & ~3 for x, p in zip(xs, per)]
    ooffs = [sum(caps[:i]) for i in range(n)]
    out = ctypes.create_string_buffer(sum(caps) + 4)
    status, olen = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)()
    f, p = zsamd._flush_arrays(per)
    r = L.zs_deflate_batch_flush(engine.handle, level, wbits, n, blob, zsamd._arr(ctypes.c_uint64, offs),
                                 zsamd._arr(ctypes.c_uint32, lens), out, zsamd._arr(ctypes.c_uint64, ooffs),
                                 zsamd._arr(ctypes.c_uint32, caps), status, olen, None, flush, f if first else None,
                                 p if pos else None)
    return r, L.zs_last_error().decode()


def test_refusals(engine):
    import zsamd

    xs = [b"hello world", b"abc"]
    for flush in (1, 2, 5):
        assert flush_call(engine, xs, [[3], []], flush=flush) == (-2, "flush mode not built")
    for flush in (-1, 0, 4, 6, 99):
        assert flush_call(engine, xs, [[3], []], flush=flush) == (-2, "invalid flush")
    assert flush_call(engine, xs, [[3], []], first=False) == (-2, "null flush arrays")
    assert flush_call(engine, xs, [[3], []], pos=False) == (-2, "null flush arrays")
    for per in ([[3, 3], []], [[5, 4], []], [[12], []], [[], [4]], [[0, 0], []]):
        assert flush_call(engine, xs, per) == (-2, "invalid flush positions"), per
    assert flush_call(engine, xs, [[3], []], level=0) == (-2, "level 0 with a flush point is not built")
    assert flush_call(engine, xs, [[], []], level=0)[0] == 0  # no flush point: the plain level-0 path
    assert flush_call(engine, xs, [[3], []], level=10) == (-2, "invalid level")
    assert flush_call(engine, xs, [[3], []], wbits=-12) == (-2, "unsupported windowBits (use -15, 15 or 31)")
    assert flush_call(engine, [b"x" * 70000], [list(range(1, 65536))])[0] == -2  # 65,536 segments
    with pytest.raises(zsamd.ZsError) as err:
        engine.compress_batch(xs, "deflate", 6, flush_at=[[5, 4], []])
    assert str(err.value) == "init failed: -2" and err.value.msg == "invalid flush positions"
    for kw in ({"zdict": b"abc"}, {"strategy": 2}, {"window_bits": 12}, {"mem_level": 4}, {"flush_every": 4}):
        with pytest.raises(ValueError):
            engine.compress_batch(xs, "deflate", 6, flush_at=[1], **kw)
    with pytest.raises(ValueError):
        engine.compress_batch(xs, "deflate", 6, flush_every=0)
