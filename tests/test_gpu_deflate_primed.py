"""GPU: primed pieces (zs_deflate_batch_primed*; pigz's construction).  Every output is compared with the
committed goldens of C zlib 1.2.11 (tests/golden/deflate_primed.json, written by gen_deflate_primed.py),
never with the zlib of the machine the test runs on; that zlib only decodes -- every output as ONE
stream.  Every output stays within zs_deflate_bound_flush.  One engine call has one level and format: a
test runs its group's calls one after the other."""
import ctypes
import zlib

import pytest

import primedcases as cases

pytestmark = pytest.mark.gpu


def want_check(fmt, x):
    return {"deflate-raw": 1, "deflate": zlib.adler32(x), "gzip": zlib.crc32(x)}[fmt]


def run(engine, batch):
    """batch: cases of one level and format; returns [(status, bytes, check)]"""
    _, _, level, fmt, _ = batch[0]
    assert all(c[2:4] == batch[0][2:4] for c in batch)
    return engine.compress_batch_detailed([c[1] for c in batch], fmt, level, flush_at=[list(c[4]) for c in batch],
                                          primed=True)


def check(batch, res):
    import zsamd

    g = cases.golden()
    fmt = batch[0][3]
    for (name, x, level, _, pos), (st, out, chk) in zip(batch, res):
        assert st == zsamd.Z_STREAM_END, (name, st)
        assert cases.digest(out) == g[name][:2], (name, len(out), g[name][:2])
        assert chk == want_check(fmt, x), name
        assert len(out) <= zsamd.deflate_bound(len(x), fmt, n_flush=len(pos)) == cases.bound(len(x), fmt, len(pos)), name
        assert zlib.decompress(out, cases.WBITS[fmt]) == x, name


def run_group(engine, name, keep=lambda c: True):
    calls = cases.by_call([c for c in cases.group(name) if keep(c)])
    assert calls
    for batch in calls:
        check(batch, run(engine, batch))
    return calls


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_every_subset_of_positions_in_three_bytes(engine, fmt):
    calls = run_group(engine, "tiny", lambda c: c[3] == fmt)
    assert sum(len(b) for b in calls) == 2 * 16


def test_a_point_at_0_and_at_the_end_write_the_marker_alone(engine):
    out = engine.compress_batch([b"abc", b"abc", b""], "deflate-raw", 6, flush_at=[[0], [3], [0]], primed=True)
    plain = engine.compress_batch([b"abc"], "deflate-raw", 6)[0]
    assert out[0] == b"\x00" + cases.MARKER + plain  # no prime in front of the piece at 0
    assert out[1].endswith(cases.MARKER + b"\x03\x00") and out[1][0] & 1 == 0  # BFINAL in the last block alone
    assert out[2] == b"\x00" + cases.MARKER + b"\x03\x00"


@pytest.mark.parametrize("level", cases.LEVELS)
def test_primes_of_1_byte_up_to_the_window(engine, level):
    calls = run_group(engine, "prime", lambda c: c[2] == level)
    assert len(calls) == 1 and len(calls[0]) == len(cases.PRIME_AT)


@pytest.mark.parametrize("level", cases.LEVELS)
def test_matches_reach_back_across_a_point(engine, level):
    calls = run_group(engine, "across", lambda c: c[2] == level)
    if level == 6:  # X || X with a point at 1,000: the second piece is one match into its prime, not 1,000 literals
        g = cases.golden()
        assert g["across/deflate-raw/l6/XX@1000"][0] < 1500  # (flushed: above 2,000, both halves stored)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_a_full_prime_and_pieces_around_the_one_window_limit(engine, level):
    calls = run_group(engine, "windows", lambda c: c[2] == level)
    assert len(calls[0]) == len(cases.WINDOW_PIECES)


def test_stored_blocks_behind_a_prime(engine):
    run_group(engine, "stored")


@pytest.mark.parametrize("level", [1, 6])
def test_a_primed_piece_that_ends_on_the_symbol_cut_drops_its_empty_block(engine, level):
    run_group(engine, "cut", lambda c: c[2] == level)


def test_segments_share_output_words_at_every_byte_phase(engine):
    run_group(engine, "seams")


def test_256_segments_of_one_stream(engine):
    run_group(engine, "many")


@pytest.mark.parametrize("fmt", cases.FMTS)
def test_streams_with_0_1_and_7_points_in_one_call(engine, fmt):
    calls = run_group(engine, "mixed", lambda c: c[3] == fmt)
    for batch in calls:  # the ones without points: the _ex entry's bytes
        level = batch[0][2]
        res = run(engine, batch)
        plain = engine.compress_batch_detailed([c[1] for c in batch if not c[4]], fmt, level)
        assert [r for c, r in zip(batch, res) if not c[4]] == plain


@pytest.mark.parametrize("level", [1, 6, 9])
def test_two_long_streams_every_131072_bytes(engine, level):
    calls = run_group(engine, "long", lambda c: c[2] == level)
    x = calls[0][0][1]
    assert engine.compress_batch([x], "deflate-raw", level, flush_every=cases.LONG_EVERY, primed=True)[0] == \
        run(engine, calls[0][:1])[0][1]


def option_batch():
    return [c for c in cases.group("mixed") if c[3] == "deflate-raw" and c[2] == 6] + \
        [c for c in cases.group("seams") if c[3] == "deflate-raw" and c[2] == 6]


def test_no_points_through_the_new_entry_are_the_ex_entry(engine):
    xs = [c[1] for c in option_batch()]
    for fmt in cases.FMTS:
        for level in (0, 1, 6):
            assert engine.compress_batch_detailed(xs, fmt, level, flush_at=[], primed=True) == \
                engine.compress_batch_detailed(xs, fmt, level), (fmt, level)


def primed_call(engine, xs, per, level=6, wbits=-15, first=True, pos=True, caps=None, check=False):
    """zs_deflate_batch_primed as given; returns (return code, zs_last_error(), status, bytes, check values)"""
    import zsamd

    L = zsamd.lib()
    n = len(xs)
    blob, offs, lens = zsamd._layout(xs)
    if caps is None:
        caps = [(len(x) + 200 + 12 * len(p) + 3) & ~3 for x, p in zip(xs, per)]
    ooffs = [sum((c + 3) & ~3 for c in caps[:i]) for i in range(n)]
    out = ctypes.create_string_buffer(sum((c + 3) & ~3 for c in caps) + 4)
    status, olen, chk = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    f, p = zsamd._flush_arrays(per)
    r = L.zs_deflate_batch_primed(engine.handle, level, wbits, n, blob, zsamd._arr(ctypes.c_uint64, offs),
                                  zsamd._arr(ctypes.c_uint32, lens), out, zsamd._arr(ctypes.c_uint64, ooffs),
                                  zsamd._arr(ctypes.c_uint32, caps), status, olen, chk if check else None,
                                  f if first else None, p if pos else None)
    raw = out.raw
    return r, L.zs_last_error().decode(), list(status), [raw[ooffs[i]:ooffs[i] + olen[i]] for i in range(n)], list(chk)


def test_a_capacity_one_byte_short_is_a_buf_error_for_that_stream_alone(engine):
    import zsamd

    batch = [c for c in cases.group("mixed") if c[3] == "gzip" and c[2] == 6]
    g = cases.golden()
    short = 3  # the stream with seven points
    assert len(batch[short][4]) == 7
    caps = [g[c[0]][0] - (1 if i == short else 0) for i, c in enumerate(batch)]  # exact capacities: the host entry takes any
    r, _, status, outs, chk = primed_call(engine, [c[1] for c in batch], [list(c[4]) for c in batch], wbits=31, caps=caps,
                                          check=True)
    assert r == 0
    for i, c in enumerate(batch):
        if i == short:
            assert (status[i], outs[i], chk[i]) == (zsamd.Z_BUF_ERROR, b"", 0)
        else:
            assert status[i] == zsamd.Z_STREAM_END and cases.digest(outs[i]) == g[c[0]][:2]


def test_device_entry(engine):
    """zs_deflate_batch_primed_device on device buffers: inputs at odd offsets, canaries between the regions"""
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
                           flush_at=per, primed=True)
    torch.cuda.synchronize()
    st, ol, ck = [r.tolist() for r in res]
    raw = bytes(d_out.cpu().numpy())
    got = [(st[i], raw[ooffs[i]:ooffs[i] + ol[i]], ck[i] & 0xffffffff) for i in range(n)]
    g = cases.golden()
    assert [cases.digest(o) for _, o, _ in got] == [g[c[0]][:2] for c in batch]
    assert got == engine.compress_batch_detailed(xs, fmt, level, flush_at=per, primed=True)
    inside = bytearray(len(raw))
    for a, c in zip(ooffs, caps):
        inside[a:a + c] = b"\1" * c
    assert all(b == 0xa5 for b, i in zip(raw, inside) if not i), "a byte outside [out_off, out_off + out_cap) changed"


@pytest.mark.parametrize("option,values,level", [("match_sweep", (0, 1), 6), ("fast_group", (0, 1), 1),
                                                 ("lane_order", (0, 1), 1), ("lane_order", (0, 1), 6),
                                                 ("parse_waves", (1, 2, 4), 6)])
def test_options_leave_the_bytes_unchanged(engine, option, values, level):
    batch = [c for c in cases.group("mixed") + cases.group("seams") + cases.group("windows")[:12:5] + cases.group("prime")
             if c[3] == "deflate-raw" and c[2] == level]
    assert len(batch) >= 9 + len(cases.PRIME_AT)
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
            assert pool.compress_batch_detailed(xs, fmt, level, flush_at=per, primed=True) == \
                engine.compress_batch_detailed(xs, fmt, level, flush_at=per, primed=True), (fmt, level)
        assert pool.compress_batch(xs, "gzip", 6, flush_every=100, primed=True) == \
            engine.compress_batch(xs, "gzip", 6, flush_every=100, primed=True)
    finally:
        pool.close()
    g = cases.golden()
    assert [cases.digest(o) for o in engine.compress_batch(xs, "deflate-raw", 6, flush_at=per, primed=True)] == \
        [g[c[0]][:2] for c in batch]


def test_a_host_call_of_four_chunks(engine):
    """at least 64 streams and host_chunk_min = 1: a stream's segments stay in one chunk, whose J are slices of
    that chunk's staged input"""
    import hostchunkcases as hc

    base = [c for c in cases.group("mixed") + cases.group("seams") + cases.group("across")
            if c[3] == "deflate-raw" and c[2] == 6]
    batch = (base * 4)[:67]
    assert len(batch) == 67
    g = cases.golden()
    with hc.chunked(engine):
        res = run(engine, batch)
        assert engine.last_host_chunks() == 4
    assert [cases.digest(o) for _, o, _ in res] == [g[c[0]][:2] for c in batch]
    assert res == run(engine, batch) and engine.last_host_chunks() == 1
    gz = [cases.case("x", "x", c[1], 6, "gzip", c[4]) for c in batch]
    with hc.chunked(engine):
        res = run(engine, gz)
        assert engine.last_host_chunks() == 4
    for c, (st, out, chk) in zip(gz, res):
        assert st == 1 and chk == zlib.crc32(c[1]) and zlib.decompress(out, 31) == c[1]


def test_last_flush_index_points_just_behind_each_marker(engine):
    g = cases.golden()
    batch = [c for c in cases.group("mixed") + cases.group("seams") + cases.group("windows") + cases.group("tiny")
             if c[3] == "deflate-raw" and c[2] == 6]
    res = run(engine, batch)
    idx = engine.last_flush_index()
    assert len(idx) == len(batch)
    for c, (st, out, _), offs in zip(batch, res, idx):
        assert list(offs) == g[c[0]][2] and len(offs) == len(c[4]), c[0]
        for off in offs:
            assert out[off - 4:off] == cases.MARKER, c[0]
    # a wrapped format: the offsets count the header
    z = [cases.case("x", "x", c[1], 6, "gzip", c[4]) for c in batch[:8]]
    res = run(engine, z)
    for c, (st, out, _), offs in zip(batch[:8], res, engine.last_flush_index()):
        assert [o - 10 for o in offs] == g[c[0]][2] and all(out[o - 4:o] == cases.MARKER for o in offs), c[0]


def test_the_engines_own_inflate_reads_a_primed_stream(engine):
    for fmt in cases.FMTS:
        batch = [c for c in cases.group("tiny") + cases.group("seams") + cases.group("mixed") + cases.group("stored")
                 if c[3] == fmt and c[2] == 6]
        assert batch
        res = run(engine, batch)
        back = engine.decompress_batch([r[1] for r in res], fmt, [max(4, (len(c[1]) + 3) & ~3) for c in batch])
        assert back == [c[1] for c in batch], fmt


def test_refusals(engine):
    import zsamd

    xs = [b"hello world", b"abc"]
    assert primed_call(engine, xs, [[3], []])[0] == 0
    assert primed_call(engine, xs, [[3], []], first=False)[:2] == (-2, "null flush arrays")
    assert primed_call(engine, xs, [[3], []], pos=False)[:2] == (-2, "null flush arrays")
    for per in ([[3, 3], []], [[5, 4], []], [[12], []], [[], [4]], [[0, 0], []]):
        assert primed_call(engine, xs, per)[:2] == (-2, "invalid flush positions"), per
    assert primed_call(engine, xs, [[3], []], level=0)[:2] == (-2, "level 0 with a flush point is not built")
    assert primed_call(engine, xs, [[], []], level=0)[0] == 0  # no point: the plain level-0 path
    assert primed_call(engine, xs, [[3], []], level=10)[:2] == (-2, "invalid level")
    assert primed_call(engine, xs, [[3], []], wbits=-12)[:2] == (-2, "unsupported windowBits (use -15, 15 or 31)")
    assert primed_call(engine, [b"x" * 70000], [list(range(1, 65536))])[:2] == \
        (-2, "too many flush points (streams + flush points above 65,535 in one call)")  # 65,536 segments
    for wbits in (-15, 15, 31):  # all three formats are taken
        r, _, status, outs, _ = primed_call(engine, xs, [[3], [1]], wbits=wbits)
        assert (r, status) == (0, [1, 1]) and [zlib.decompress(o, wbits) for o in outs] == xs
    with pytest.raises(zsamd.ZsError) as err:
        engine.compress_batch(xs, "deflate", 6, flush_at=[[5, 4], []], primed=True)
    assert str(err.value) == "init failed: -2" and err.value.msg == "invalid flush positions"
    for kw in ({"zdict": b"abc"}, {"strategy": 2}, {"window_bits": 12}, {"mem_level": 4}, {"flush_every": 4}):
        with pytest.raises(ValueError):
            engine.compress_batch(xs, "deflate", 6, flush_at=[1], primed=True, **kw)
    with pytest.raises(ValueError):
        engine.compress_batch(xs, "deflate", 6, primed=True)
    with pytest.raises(ValueError):
        engine.compress_batch(xs, "gzip", 6, primed=True, flush_every=4, bgzf=True)
    # the existing refusal of Z_SYNC_FLUSH by the _flush entries stays
    L = zsamd.lib()
    off, ln, cap = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint32 * 1)(3), (ctypes.c_uint32 * 1)(64)
    st, ol = (ctypes.c_int32 * 1)(), (ctypes.c_uint32 * 1)()
    first, pos = (ctypes.c_uint64 * 2)(0, 1), (ctypes.c_uint32 * 1)(1)
    assert L.zs_deflate_batch_flush(engine.handle, 6, -15, 1, b"abc", off, ln, ctypes.create_string_buffer(64), off, cap,
                                    st, ol, None, 2, first, pos) == -2
    assert L.zs_last_error() == b"flush mode not built"
