"""GPU: the BGZF writer (zs_deflate_batch_bgzf*, deflate_bgzf.hip).  The bytes are compared with
the committed goldens (tests/golden/deflate_bgzf.json, written by gen_deflate_bgzf.py from C zlib 1.2.11 and the
framing of include/zs_gpu.h), never with the zlib of the machine the test runs on; that zlib only decodes.  (Level
0 is written out by hand, and the other entries' outputs are compared with the host entry's, which the goldens
pin.)  Every golden output also stays within zs_deflate_bound_bgzf, carries the crc32 of the whole input as its
check value, and its blocks are where zs_last_bgzf_blocks says.  One engine call has one level and block size: a test runs its group's
calls one after the other."""
import ctypes
import gzip
import struct
import zlib

import pytest

import bgzfcases
import bgzfwritecases as cases
import hostchunkcases as hc

pytestmark = pytest.mark.gpu
B = cases.B


def run(engine, batch):
    """batch: cases of one level and block size; returns [(status, bytes, check)]"""
    _, _, level, bb = batch[0]
    assert all(c[2:4] == batch[0][2:4] for c in batch)
    return engine.compress_batch_detailed([c[1] for c in batch], "gzip", level, bgzf=bb)


def check(engine, batch, res):
    import zsamd

    g = cases.golden()
    blocks = engine.last_bgzf_blocks()
    assert len(blocks) == len(batch)
    for (name, x, level, bb), (st, out, chk), idx in zip(batch, res, blocks):
        assert st == zsamd.Z_STREAM_END, (name, st)
        assert cases.digest(out) == g[name], (name, len(out), g[name])
        assert chk == zlib.crc32(x), name
        assert len(out) <= zsamd.deflate_bound(len(x), "gzip", bgzf=bb) == cases.bound(len(x), bb), name
        assert gzip.decompress(out) == x, name
        ok, total, chain = bgzfcases.chain(out)
        assert (ok, total) == (1, len(x)), name
        assert idx == [(i, o) for o, i in chain], name


def run_group(engine, name, keep=lambda c: True):
    calls = cases.by_call([c for c in cases.group(name) if keep(c)])
    assert calls
    for batch in calls:
        check(engine, batch, run(engine, batch))
    return calls


def test_the_empty_input_is_the_end_of_file_block(engine):
    run_group(engine, "empty")
    for level in (0, 1, 6, 9):
        assert engine.compress_batch([b"", b""], "gzip", level, bgzf=True) == [cases.EOF] * 2
        assert engine.last_bgzf_blocks() == [[(0, 0)]] * 2
    assert len(cases.EOF) == 28


@pytest.mark.parametrize("level", cases.EDGE_LEVELS)
def test_one_byte_and_lengths_around_the_block_size(engine, level):
    calls = run_group(engine, "edge", lambda c: c[2] == level)
    assert sum(len(b) for b in calls) == len(cases.EDGE_LENS)
    # B + 1: a one-byte last block
    out = run(engine, [c for c in cases.group("edge") if c[2] == level and len(c[1]) == B + 1])[0][1]
    idx = bgzfcases.chain(out)[2]
    assert [i for _, i in idx] == [0, B, B + 1] and struct.unpack_from("<I", out, idx[2][0] - 4)[0] == 1


@pytest.mark.parametrize("level", [1, 6])
def test_frames_share_output_words_at_every_byte_phase(engine, level):
    calls = run_group(engine, "phases", lambda c: c[2] == level)
    res = run(engine, [c for c in cases.group("phases") if c[2] == level and c[3] == 1])
    starts = {o % 4 for o, _ in bgzfcases.chain(res[0][1])[2]}
    assert starts == {0, 1, 2, 3} and len(calls) == 2


@pytest.mark.parametrize("level", [1, 6])
def test_a_piece_that_ends_on_the_symbol_cut_keeps_its_empty_block(engine, level):
    run_group(engine, "cut", lambda c: c[2] == level)
    if level == 1:  # filler(16383): the finished piece has the empty static block the flushed layout drops
        import deflate_header

        c = [c for c in cases.group("cut") if c[2] == 1][0]
        out = run(engine, [c])[0][1]
        end = bgzfcases.trusted(out, 0)[0]
        assert [b.type for b in deflate_header.parse(out[18:end - 8])][1:] == [1]
        assert out[18:end - 8] == engine.compress_batch([cases.filler(cases.CUT)], "deflate-raw", 1)[0]


@pytest.mark.parametrize("level", [1, 6, 9])
def test_stored_blocks_inside_the_largest_member(engine, level):
    batch = [c for c in cases.group("stored") if c[2] == level]
    res = run(engine, batch)
    check(engine, batch, res)
    out = res[0][1]
    assert struct.unpack_from("<H", out, 16)[0] == len(out) - 28 - 1 == 18 + B + 4 * 5 + 8 - 1  # BSIZE


def test_600_segments_of_one_stream(engine):
    run_group(engine, "many")


def test_streams_of_0_1_and_3_blocks_in_one_call(engine):
    calls = run_group(engine, "mixed")
    assert [len(c[1]) for c in calls[0]] == [3000, 0, 2 * cases.MIXED_BLOCK + 1]
    assert [len(b) for b in engine.last_bgzf_blocks()] == [2, 1, 4]


def test_level_0_is_stored_blocks(engine):
    run_group(engine, "level0")
    # at every byte phase, and with an empty stream between
    xs = [cases.group("phases")[1][1], b"", cases.group("phases")[0][1][:9]]
    for bb in (1, 7):
        assert engine.compress_batch(xs, "gzip", 0, bgzf=bb) == [cases.compress(x, 0, bb) for x in xs]
        assert engine.last_bgzf_blocks() == [cases.index(x, 0, bb) for x in xs]


def host_call(engine, xs, level, bb, caps):
    """zs_deflate_batch_bgzf on caller-owned memory, a canary round the regions: the result arrays and the bytes"""
    L, n = engine._L, len(xs)
    blob, ioffs = hc._inputs(xs)
    offs, total = hc.regions(caps)
    out = ctypes.create_string_buffer(hc.canary(total), total)
    status, olen, chk = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    rc = L.zs_deflate_batch_bgzf(engine.handle, level, n, blob, hc._u64(ioffs), hc._u32([len(x) for x in xs]), out,
                                 hc._u64(offs), hc._u32(caps), status, olen, chk, bb)
    data = hc._collect(engine, rc, "zs_deflate_batch_bgzf", out, total, offs, list(olen))
    return {"status": list(status), "len": list(olen), "check": list(chk), "data": data}


@pytest.mark.parametrize("level", [0, 6])
def test_a_short_capacity_is_a_buf_error_for_that_stream_alone(engine, level):
    bb = cases.MIXED_BLOCK
    batch = list(cases.group("mixed"))
    xs = [c[1] for c in batch] + [b""]
    want = engine.compress_batch(xs, "gzip", level, bgzf=bb)  # (pinned: the goldens, level 0 by hand)
    assert [cases.digest(w) for w in want[:3]] == [cases.digest(cases.compress(x, 0, bb)) if level == 0 else
                                                   cases.golden()[c[0]] for c, x in zip(batch, xs)]
    assert want[3] == cases.EOF
    exact = host_call(engine, xs, level, bb, [len(w) for w in want])
    hc.check_deflate(exact, xs, "gzip", want)
    for short, cap in ((2, len(want[2]) - 1), (2, 0), (1, 27), (3, 0), (0, len(want[0]) - 1)):
        caps = [cap if i == short else len(w) for i, w in enumerate(want)]
        res = host_call(engine, xs, level, bb, caps)
        hc.check_deflate(res, xs, "gzip", want, ok=[i != short for i in range(len(xs))])
        assert res["check"][short] == 0


def test_device_entry(engine):
    """zs_deflate_batch_bgzf_device on device buffers: inputs at odd offsets, canaries between the regions"""
    import torch
    import zsamd

    for level, batch in ((6, list(cases.group("mixed")) + [c for c in cases.group("phases") if c[2] == 6 and c[3] == 7]),
                         (0, list(cases.group("mixed")))):
        bb = cases.MIXED_BLOCK
        xs = [c[1] for c in batch]
        n = len(xs)
        blob, offs, lens = zsamd._layout(xs)
        caps = [(zsamd.deflate_bound(len(x), "gzip", bgzf=bb) + 3) & ~3 for x in xs]
        ooffs, oo = [], 16
        for c in caps:
            ooffs.append(oo)
            oo += c + 16
        d_in = torch.frombuffer(bytearray(b"\xee" + blob + b"\0" * 16), dtype=torch.uint8).cuda()
        d_out = torch.full((oo,), 0xa5, dtype=torch.uint8, device="cuda")
        res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
        engine.compress_device(level, "gzip", n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*[o + 1 for o in offs]),
                               (ctypes.c_uint32 * n)(*lens), d_out.data_ptr(), (ctypes.c_uint64 * n)(*ooffs),
                               (ctypes.c_uint32 * n)(*caps), res[0].data_ptr(), res[1].data_ptr(), 0, res[2].data_ptr(),
                               bgzf=bb)
        torch.cuda.synchronize()
        blocks = engine.last_bgzf_blocks()
        st, ol, ck = [r.tolist() for r in res]
        raw = bytes(d_out.cpu().numpy())
        got = [(st[i], raw[ooffs[i]:ooffs[i] + ol[i]], ck[i] & 0xffffffff) for i in range(n)]
        assert [g[0] for g in got] == [1] * n and [g[2] for g in got] == [zlib.crc32(x) for x in xs], level
        if level == 0:
            assert [g[1] for g in got] == [cases.compress(x, 0, bb) for x in xs]
        else:
            assert [cases.digest(g[1]) for g in got[:3]] == [cases.golden()[c[0]] for c in batch[:3]]
            assert [gzip.decompress(g[1]) for g in got] == xs
        assert blocks == [[(i, o) for o, i in bgzfcases.chain(g[1])[2]] for g in got]
        assert got == engine.compress_batch_detailed(xs, "gzip", level, bgzf=bb)
        inside = bytearray(len(raw))
        for a, c in zip(ooffs, caps):
            inside[a:a + c] = b"\1" * c
        assert all(b == 0xa5 for b, i in zip(raw, inside) if not i), "a byte outside [out_off, out_off + out_cap) changed"


@pytest.mark.parametrize("option,values,level", [("match_sweep", (0, 1), 6), ("fast_group", (0, 1), 1)])
def test_options_leave_the_bytes_unchanged(engine, option, values, level):
    batch = [c for g in ("phases", "cut", "many") for c in cases.group(g) if c[2] == level]
    g = cases.golden()
    try:
        for v in values:
            engine.set_option(option, v)
            for call in cases.by_call(batch):
                res = run(engine, call)
                assert [cases.digest(o) for _, o, _ in res] == [g[c[0]] for c in call], (option, v)
    finally:
        engine.set_option(option, 1)


def test_pool_of_two_contexts_on_one_device_equals_one_context(engine):
    import zsamd

    xs = [c[1] for c in cases.group("mixed")] * 2 + [cases.group("phases")[1][1]]
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        assert len(pool.devices) == 2
        for level, bb in ((1, 7), (6, cases.MIXED_BLOCK), (0, 100), (9, True)):
            assert pool.compress_batch_detailed(xs, "gzip", level, bgzf=bb) == \
                engine.compress_batch_detailed(xs, "gzip", level, bgzf=bb), (level, bb)
    finally:
        pool.close()


@pytest.mark.parametrize("level", [0, 6])
def test_a_host_call_of_four_chunks_equals_one_chunk_and_its_blocks_are_right(engine, level):
    bb = 1000
    xs = [hc.filler_at(i) if i % 9 else b"" for i in range(64)]
    with hc.chunked(engine, 1):
        four = engine.compress_batch_detailed(xs, "gzip", level, bgzf=bb)
        assert engine.last_host_chunks() == 4
        blocks = engine.last_bgzf_blocks()
    with hc.chunked(engine, 0):
        one = engine.compress_batch_detailed(xs, "gzip", level, bgzf=bb)
        assert engine.last_host_chunks() == 1
        assert engine.last_bgzf_blocks() == blocks
    assert four == one
    assert [(st, chk) for st, _, chk in four] == [(1, zlib.crc32(x)) for x in xs]
    assert [gzip.decompress(out) for _, out, _ in four] == xs
    if level == 0:
        assert [out for _, out, _ in four] == [cases.compress(x, 0, bb) for x in xs]
    else:  # each stream alone: the same bytes
        distinct = sorted(set(xs))
        alone = dict(zip(distinct, engine.compress_batch(distinct, "gzip", level, bgzf=bb)))
        assert [out for _, out, _ in four] == [alone[x] for x in xs]
    assert blocks == [[(i, o) for o, i in bgzfcases.chain(out)[2]] for _, out, _ in four]
    assert [[i for i, _ in b] for b in blocks] == [list(range(0, len(x), bb)) + [len(x)] for x in xs]


def test_round_trip_through_the_bgzf_reader(engine):
    xs = [c[1] for c in cases.group("mixed")] + [cases.group("edge")[4][1], cases.group("phases")[1][1]]
    for level, bb in ((6, True), (1, 4096), (0, 7)):
        files = engine.compress_batch(xs, "gzip", level, bgzf=bb)
        blocks = sum(len(b) for b in engine.last_bgzf_blocks())  # data blocks + end-of-file blocks
        assert engine.decompress_batch(files, "gzip", members="bgzf") == xs, (level, bb)
        assert engine.last_bgzf_trusted() == blocks
        assert [[m[0] for m in ms] for ms in engine.last_members()] == \
            [[o for o, _ in bgzfcases.chain(f)[2]] for f in files]


def bgzf_call(engine, xs, level=6, bb=0, null=False):
    """zs_deflate_batch_bgzf as given; returns (return code, zs_last_error())"""
    import zsamd

    L = zsamd.lib()
    n = len(xs)
    blob, offs, lens = zsamd._layout(xs)
    caps = [(cases.bound(len(x), bb if 0 < bb <= B else B) + 3) & ~3 for x in xs]
    ooffs = [sum(caps[:i]) for i in range(n)]
    out = ctypes.create_string_buffer(sum(caps) + 4)
    status, olen = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)()
    r = L.zs_deflate_batch_bgzf(engine.handle, level, n, blob, None if null else zsamd._arr(ctypes.c_uint64, offs),
                                zsamd._arr(ctypes.c_uint32, lens), out, zsamd._arr(ctypes.c_uint64, ooffs),
                                zsamd._arr(ctypes.c_uint32, caps), status, olen, None, bb)
    return r, L.zs_last_error().decode()


def test_refusals(engine):
    import zsamd

    xs = [b"hello world", b"abc"]
    assert bgzf_call(engine, xs)[0] == 0
    for level in (-2, 10):
        assert bgzf_call(engine, xs, level=level, bb=65281, null=True) == (-2, "invalid level")
    assert bgzf_call(engine, xs, bb=65281, null=True) == (-2, "invalid BGZF block size")
    assert bgzf_call(engine, xs, null=True) == (-2, "null arrays")
    many = "too many BGZF blocks (streams + blocks above 65,535 in one call)"
    assert bgzf_call(engine, [b"x" * 65535], bb=1) == (-2, many)  # one host chunk: one device call
    with pytest.raises(zsamd.ZsError) as err:
        engine.compress_batch(xs, "gzip", 6, bgzf=65281)
    assert str(err.value) == "init failed: -2" and err.value.msg == "invalid BGZF block size"
    for kw in ({"zdict": b"abc"}, {"strategy": 2}, {"window_bits": 12}, {"mem_level": 4}, {"flush_every": 4},
               {"flush_at": [1]}):
        with pytest.raises(ValueError):
            engine.compress_batch(xs, "gzip", 6, bgzf=True, **kw)
    with pytest.raises(ValueError):
        engine.compress_batch(xs, "deflate", 6, bgzf=True)
    # the flushed entry's index is not a BGZF call's, and the other way round
    engine.compress_batch(xs, "gzip", 6, bgzf=True)
    assert engine.last_flush_index() == []
    engine.compress_batch(xs, "gzip", 6, flush_at=[1])
    assert engine.last_bgzf_blocks() == []
    engine.compress_batch(xs, "gzip", 6)
    assert engine.last_bgzf_blocks() == []
