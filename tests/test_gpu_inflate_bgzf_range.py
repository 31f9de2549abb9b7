"""GPU tests of BGZF ranges by virtual offset (zs_inflate_batch_bgzf_range*, inflate_bgzf_range.hip):
ranges=[(vb, ve)] with members="bgzf" delivers the bytes between two virtual offsets.  The expected bytes are zlib's
on the host, the decompressed file sliced at the positions the offsets name (bgzfrangecases.expect); failures are held
against the contract of include/zs_gpu.h.  Every case is a few hundred KB at the most."""
import ctypes
import random
import zlib

import pytest

import bgzfrangecases as rc
import corpus
import memberscases as mc
from bgzfrangecases import RANGE, voff
from memberscases import BGZF_EOF, CAPACITY, cap4, member, text

bc = rc.bc
pytestmark = pytest.mark.gpu
LENGTH_CHECK = (-3, 2, "incorrect length check")


def rng(engine, streams, ranges, caps=None):
    return engine.decompress_batch_detailed(streams, "gzip", out_caps=caps, members="bgzf", ranges=ranges)


def file_of(block_bytes, blocks=5, seed=3):
    """a file of `blocks` data blocks, the last one short, and the end-of-file block"""
    return bc.bgzf(text(block_bytes * (blocks - 1) + max(1, block_bytes // 3), seed), block_bytes)


def alignments(s):
    """ub through 0..3 and with it the second member's destination (ISIZE - ub) through every alignment, from the
    first block and from the second; the range's end moves the last member's length through 0..3 as well"""
    b = rc.blocks(s)
    out = {}
    for k in range(4):
        if k <= b[0][2] and k <= b[1][2]:
            out["ub %d from block 0" % k] = (voff(b[0][0], k), voff(b[2][0], min(b[2][2], k + 1)))
            out["ub %d from block 1" % k] = (voff(b[1][0], k), voff(b[3][0], min(b[3][2], k + 1)))
    return out


@pytest.mark.parametrize("block_bytes", [1, 3, 64, 300, 4099])
def test_every_corner_over_files_of_small_blocks(engine, block_bytes):
    s = file_of(block_bytes)
    cases = dict(rc.corners(s))
    cases.update(alignments(s))
    if block_bytes >= 3:
        assert any(k.startswith("ub 3") for k in cases)
    names = list(cases)
    ranges = [cases[k] for k in names]
    want = [rc.expect(s, *r) for r in ranges]
    assert all(w[0] == 1 for w in want)
    data, idx = rc.whole(s)
    upos = lambda v: dict(idx)[v >> 16] + (v & 0xffff)
    for (vb, ve), w in zip(ranges, want):  # the decompressed file sliced at the positions the offsets name
        assert w[3] == data[upos(vb):upos(ve)]
    got = rng(engine, [s] * len(ranges), ranges, [cap4(len(w[3])) for w in want])
    for k, g, w in zip(names, got, want):
        assert g == w, (block_bytes, k, g[:3], g[4:], w[4:])
    assert engine.last_host_chunks() == 1 and engine.last_members() == []
    # exact capacities, and sized from the headers by the binding
    assert rng(engine, [s] * len(ranges), ranges, [len(w[3]) for w in want]) == want
    assert engine.decompress_batch([s] * len(ranges), "gzip", members="bgzf", ranges=ranges) == [w[3] for w in want]


def test_full_blocks_span_several_place_tiles(engine):
    data = corpus.rand(1, 30000) + text(3 * 65280 - 30000, 21)
    s = bc.bgzf(data)
    b = rc.blocks(s)
    assert [x[2] for x in b] == [65280] * 3 + [0]
    ranges = [(voff(0, k), voff(b[2][0], 65279 - k)) for k in range(4)]
    ranges += [(0, voff(len(s), 0)), (voff(b[1][0], 65275), voff(b[2][0], 3)), (voff(b[1][0], 4097), voff(b[1][0], 65280)),
               (voff(b[0][0], 65280), voff(b[1][0], 1))]
    want = [rc.expect(s, *r) for r in ranges]
    assert want[4][3] == data and want[5][3] == data[2 * 65280 - 5:2 * 65280 + 3] and want[7][3] == data[65280:65281]
    engine.set_timing(True)
    try:
        got = rng(engine, [s] * len(ranges), ranges, [cap4(len(w[3])) for w in want])
        placed, sized = engine.last_ms("bgzf_range_place"), engine.last_ms("bgzf_size")
    finally:
        engine.set_timing(False)
    assert got == want, [(g[:3], g[4:], w[4:]) for g, w in zip(got, want)]
    assert placed > 0 and sized > 0
    assert engine.last_bgzf_trusted() == 4 * 3 + 4 + 2 + 1 + 2  # every planned block is sized from its header


def test_seventy_blocks_are_more_than_one_round_of_the_stitch(engine):
    s = bc.bgzf(text(70 * 64, 5), 64)
    b = rc.blocks(s)
    assert len(b) == 71
    bad = bytearray(s)
    bad[b[66][0] + 20] ^= 0xff  # block 66's deflate data: behind the first round of 64
    bad = bytes(bad)
    ranges = [(voff(0, 7), voff(b[69][0], 9)), (0, voff(len(s), 0)), (voff(b[1][0], 63), voff(b[68][0], 0))]
    want = [rc.expect(s, *r) for r in ranges]
    assert len(want[0][3]) == 70 * 64 - 7 - 55
    got = rng(engine, [s, s, s, bad], ranges + [ranges[0]], [cap4(len(w[3])) for w in want] + [cap4(len(want[0][3]))])
    assert got[:3] == want
    g = got[3]
    assert g[0] != 1 and g[3] == want[0][3][:66 * 64 - 7] and g[4] == b[66][0] and g[5] == 0, (g[:3], g[4:])


def throughout():
    """the truthful streams that are BGZF throughout: the whole-file range equals members="bgzf" """
    b100 = bc.bgzf(text(300), 100)
    return {
        "one block + EOF": bc.bgzf(text(500, 1)),
        "EOF only": BGZF_EOF,
        "three blocks of 100": b100,
        "three blocks of 101": bc.bgzf(text(303, 2), 101),
        "300 one-byte blocks": bc.bgzf(text(300, 3), 1),
        "one 65,280-byte block": bc.bgzf(corpus.rand(1, 20000) + text(45280, 4), 65280),
        "XY then BC": bc.xy_block(text(500, 3)) + bc.block(text(20)) + BGZF_EOF,
        "trailing zeros": b100 + b"\x00" * 37,
        "trailing noise": b100 + corpus.rand(5, 50),
        "a BGZF file stored inside a block": bc.block(bc.bgzf(text(120, 4), 10), level=0) + bc.block(text(9)) + BGZF_EOF,
        "no EOF block": bc.bgzf(text(90, 1), 30, eof=False),
    }


def test_the_whole_file_range_equals_the_bgzf_entry_in_every_field(engine):
    t = throughout()
    streams, caps = [], []
    for s in t.values():
        assert bc.chain(s)[0] == 1
        n = len(mc.walk(s)[1])
        streams += [s, s, s]
        caps += [n, max(n - 1, 0), 0]  # enough, one short, none
    full = engine.decompress_batch_detailed(streams, "gzip", out_caps=caps, members="bgzf")
    trusted = engine.last_bgzf_trusted()
    names = [k for k in t for _ in range(3)]
    for k, g, c in zip(names, full, caps):
        assert g[0] == 1 or g[:3] == CAPACITY, (k, c)
    # consumed_full: what the _bgzf entry reports for the stream with room
    ranges = [(0, voff(full[3 * (i // 3)][4], 0)) for i in range(len(streams))]
    got = rng(engine, streams, ranges, caps)
    for k, g, w, c in zip(names, got, full, caps):
        assert g == w, (k, c, g[:3], g[4:], w[:3], w[4:])
    assert engine.last_bgzf_trusted() == trusted
    assert sum(g[0] == 1 for g in got) >= len(t) + 1 and sum(g[:3] == CAPACITY for g in got) >= 2 * len(t) - 3


def test_a_chain_through_a_member_that_is_no_bgzf_block_fails_there(engine):
    first = bc.block(text(40, 1))
    s = first + member(text(33, 2)) + bc.block(text(30, 4)) + BGZF_EOF
    t = first + mc.hand_member(text(50, 3), name=b"n.txt") + BGZF_EOF
    z = mc.bgzf(text(300, 6), block=100)  # BSIZE 0: nothing to follow
    ok = bc.bgzf(text(640, 8), 320)
    got = rng(engine, [s, ok, t, z, s], [(0, voff(len(s), 0)), (0, voff(len(ok), 0)), (voff(0, 3), voff(len(t), 0)),
                                         (0, voff(len(z), 0)), (voff(0, 5), voff(len(first), 0))], [200, 640, 200, 300, 40])
    assert got[0] == RANGE + (b"", len(first), 0) and got[2] == RANGE + (b"", len(first), 0) and got[3] == RANGE + (b"", 0, 0)
    assert got[1] == rc.expect(ok, 0, voff(len(ok), 0)) and got[1][3] == text(640, 8)
    assert got[4] == (1, 0, "", text(40, 1)[5:], len(first), zlib.crc32(text(40, 1)[5:]))  # ... and a range in front of it


def test_64_ranges_that_name_the_same_input_and_through_the_pool(engine):
    import zsamd

    s = file_of(300, blocks=9, seed=11)
    data, idx = rc.whole(s)
    r = random.Random(5)
    ranges = []
    for _ in range(64):
        a = r.randrange(len(data))
        e = r.randrange(a, min(len(data), a + 900) + 1)
        ranges.append((rc.voffset(idx, a), rc.voffset(idx, e)))
        assert rc.expect(s, *ranges[-1])[3] == data[a:e]
    want = [rc.expect(s, *x) for x in ranges]
    got = rng(engine, [s] * 64, ranges)
    assert got == want
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        assert pool.decompress_batch_detailed([s] * 64, "gzip", members="bgzf", ranges=ranges) == want
        assert pool.decompress_batch([s] * 3, "gzip", out_caps=[1000] * 3, members="bgzf", ranges=ranges[:3]) == [w[3] for w in want[:3]]
    finally:
        pool.close()


def _device(engine, streams, ranges, caps, guard=64):
    """The device entry.  Streams that are the same object lie once in the blob, at odd offsets; the regions are `guard`
    bytes of 0x5a apart and filled with 0x5a.  Returns the streams' fields; asserts that the input is only read, that no
    byte outside the regions rounded up to 4 changed and that none changed behind a delivered length rounded up to 4."""
    import torch

    n = len(streams)
    blob, at = bytearray(b"\x1f\x8b\x08\x04" * 4), {}
    for k, s in enumerate(streams):
        if id(s) not in at:
            blob += b"\x1f\x8b\x08\x04"[: 1 + len(at) % 3]  # (odd offsets; the filler would pass the scan's test)
            at[id(s)] = len(blob)
            blob += s
    blob += b"\x1f\x8b\x08\x04" * 4
    in_offs = [at[id(s)] for s in streams]
    out_off, o = [], guard
    for c in caps:
        assert c % 4 == 0
        out_off.append(o)
        o += c + guard
    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_out = torch.full((o,), 0x5a, dtype=torch.uint8, device="cuda")
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device="cuda")
    d_st, d_ph, d_msg, d_len, d_cons, d_chk = i32(), i32(), i32(), i32(), i32(), i32()
    engine.decompress_device("gzip", n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*in_offs),
                             (ctypes.c_uint32 * n)(*[len(s) for s in streams]), d_out.data_ptr(),
                             (ctypes.c_uint64 * n)(*out_off), (ctypes.c_uint32 * n)(*caps), d_st.data_ptr(),
                             d_ph.data_ptr(), d_msg.data_ptr(), d_len.data_ptr(), d_cons.data_ptr(),
                             d_check=d_chk.data_ptr(), members="bgzf", ranges=ranges)
    torch.cuda.synchronize()
    assert bytes(d_in.cpu().numpy()) == bytes(blob)
    out = bytes(d_out.cpu().numpy())
    lens = d_len.tolist()
    keep = bytearray(b"\x01" * len(out))
    for a, c, l in zip(out_off, caps, lens):
        assert l <= c
        keep[a:a + cap4(l)] = b"\x00" * cap4(l)
    assert all(b == 0x5a for b, k in zip(out, keep) if k)  # every canary is as it was
    msg = lambda m: engine._L.zs_inflate_message(m).decode()
    return [(st, ph, msg(m), out[a:a + l], c, k & 0xffffffff)
            for st, ph, m, l, c, k, a in zip(d_st.tolist(), d_ph.tolist(), d_msg.tolist(), lens, d_cons.tolist(),
                                             d_chk.tolist(), out_off)]


def test_the_device_entry_with_canaries(engine):
    s, big = file_of(300), file_of(4099)
    cases = [(s, r) for r in list(rc.corners(s).values()) + list(alignments(s).values())]
    cases += [(big, r) for r in list(rc.corners(big).values()) + list(alignments(big).values())]
    cases += [(s, r) for r, _ in rc.header_failures(s).values()]
    want = [rc.expect(x, *r) for x, r in cases]
    caps = [cap4(len(w[3])) + (8 if i % 3 == 0 else 0) for i, w in enumerate(want)]  # some with room to spare
    # ... and the capacity cut: the range over the five data blocks from byte 10, room for two and a half of them
    b = rc.blocks(s)
    cut = (voff(0, 10), voff(b[4][0], 50))
    cases.append((s, cut))
    caps.append(800)
    want.append(rc.expect(s, *cut, cap=800))
    assert want[-1] == CAPACITY + (text(1300, 3)[10:600], b[2][0], 0)
    assert sum(w[:3] == RANGE for w in want) == len(rc.header_failures(s))
    got = _device(engine, [x for x, _ in cases], [r for _, r in cases], caps)
    for (x, r), g, w in zip(cases, got, want):
        assert g == w, (len(x), hex(r[0]), hex(r[1]), g[:3], g[4:], w[:3], w[4:])
    assert rng(engine, [x for x, _ in cases], [r for _, r in cases], caps) == want  # the host entry: the same fields


def broken():
    """{name: (stream, the failing block's index)} over three data blocks and the end-of-file block: a corrupt
    first, interior and last block (a flipped byte of stored data: the CRC fails), an ISIZE that lies both ways in the
    middle block"""
    d = [text(500, 1), text(700, 2), text(300, 3)]
    good = [bc.block(d[0], level=0), bc.block(d[1], level=0), bc.block(d[2], level=0)]
    out = {}
    for k, name in enumerate(("corrupt first", "corrupt interior", "corrupt last")):
        x = bytearray(good[k])
        x[18 + 5 + 100] ^= 0x10
        out[name] = (b"".join(bytes(x) if j == k else g for j, g in enumerate(good)) + BGZF_EOF, k)
    out["ISIZE one too small"] = (good[0] + bc.block(d[1], isize=699) + good[2] + BGZF_EOF, 1)
    out["ISIZE one too large"] = (good[0] + bc.block(d[1], isize=701) + good[2] + BGZF_EOF, 1)
    return out, d


def test_failures_follow_the_contract_and_leave_the_neighbours_whole(engine):
    cases, d = broken()
    ok = bc.bgzf(text(640, 8), 320)
    whole = bc.bgzf(text(900, 5), 300)
    wb = rc.blocks(whole)
    cut = whole[:wb[2][0] + (wb[2][1] - wb[2][0]) // 2]  # the last data block truncated in its data
    streams, ranges, want, caps = [], [], [], []

    def add(s, r, w, cap=1600):
        streams.append(s)
        ranges.append(r)
        want.append(w)
        caps.append(cap)

    # what the _bgzf entry reports for the failing member: its status, phase and message are the range's
    names = list(cases)
    heads = [g[:3] for g in engine.decompress_batch_detailed([cases[k][0] for k in names], "gzip", out_caps=[1600] * len(names),
                                                              members="bgzf")]
    assert all(h[0] != 1 for h in heads) and heads[3] == LENGTH_CHECK and heads[4][2] == "incorrect length check"
    for k, head in zip(names, heads):
        s, bad = cases[k]
        b = rc.blocks(s)
        for ub, last, ue in ((2, 2, 7), (0, 3, 0)):  # from inside block 0 into block 2; whole blocks to the EOF block
            before = b"".join(d[:bad])[ub:]
            add(ok, (0, voff(len(ok), 0)), rc.expect(ok, 0, voff(len(ok), 0)), 640)
            add(s, (voff(0, ub), voff(b[last][0], ue)), head + (before, b[bad][0], 0))
    # the truncated last block cannot be trusted: the headers fail the stream, nothing decodes
    add(cut, (voff(0, 1), voff(wb[2][0], 5)), RANGE + (b"", wb[2][0], 0))
    add(cut, (voff(0, 1), voff(wb[2][0], 0)), rc.expect(cut, voff(0, 1), voff(wb[2][0], 0)))  # ... in front of it: fine
    add(ok, (voff(0, 5), voff(rc.blocks(ok)[1][0], 9)), rc.expect(ok, voff(0, 5), voff(rc.blocks(ok)[1][0], 9)), 324)
    got = rng(engine, streams, ranges, caps)
    for g, w, r in zip(got, want, ranges):
        assert g == w, (hex(r[0]), hex(r[1]), g[:3], g[4:], w[:3], w[4:])
    # through the device entry: the same fields, no byte behind a delivered length, a failed stream's region untouched
    assert _device(engine, streams, ranges, [cap4(c) for c in caps]) == want


def test_header_failures_leave_the_region_untouched(engine):
    s = file_of(300)
    f = rc.header_failures(s)
    ok = (voff(0, 1), voff(rc.blocks(s)[1][0], 2))
    streams = [s] * (len(f) + 2)
    ranges = [ok] + [r for r, _ in f.values()] + [ok]
    want = [rc.expect(s, *ok)] + [RANGE + (b"", start, 0) for _, start in f.values()] + [rc.expect(s, *ok)]
    assert _device(engine, streams, ranges, [1400] * len(streams)) == want  # (out_len 0: every byte of the region is a canary)


def test_round_trip_with_the_writer_and_the_index(engine):
    data = text(5000, 9)
    (s,) = engine.compress_batch([data], "gzip", 6, bgzf=300)
    (blocks,) = engine.last_bgzf_blocks()
    import zsamd

    # (the writer's pairs are (uncompressed, compressed); the last one is the end-of-file block's)
    assert blocks[-1] == (len(data), len(s) - 28) and len(blocks) == 17 + 1
    r = random.Random(2)
    pos = [(0, len(data)), (299, 300), (300, 300), (4999, 5000)]
    while len(pos) < 32:
        a = r.randrange(len(data) + 1)
        pos.append((a, r.randrange(a, len(data) + 1)))
    ranges = [(zsamd.bgzf_voffset(blocks, a, written=True), zsamd.bgzf_voffset(blocks, e, written=True)) for a, e in pos]
    assert zsamd.bgzf_voffset(blocks, len(data) + 1, written=True) is None
    assert all(v is not None for x in ranges for v in x)
    assert engine.decompress_batch([s] * 32, "gzip", members="bgzf", ranges=ranges) == [data[a:e] for a, e in pos]


def test_python_refuses_what_it_cannot_size_or_route(engine):
    s = file_of(300)
    with pytest.raises(ValueError, match="stream 1: the virtual offsets do not follow a chain of BGZF blocks"):
        engine.decompress_batch([s, s], "gzip", members="bgzf", ranges=[(0, 0), (voff(3, 0), voff(len(s), 0))])
    for members in (False, True):
        with pytest.raises(ValueError, match='ranges need members="bgzf"'):
            engine.decompress_batch([s], "gzip", out_caps=[16], members=members, ranges=[(0, 0)])
    # the engine's own refusal of a range behind its end, as an error of the call
    import zsamd

    with pytest.raises(zsamd.ZsError):
        engine.decompress_batch([s], "gzip", out_caps=[16], members="bgzf", ranges=[(voff(0, 1), 0)])
