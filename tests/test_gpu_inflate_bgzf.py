"""GPU tests of the BGZF fast path (zs_inflate_batch_bgzf*, inflate_bgzf.hip): members="bgzf" sizes
a block from its header where that can be trusted and gives, for every stream whose trusted headers tell the truth,
field for field what members=True gives -- successes and failures; where a trusted header lies the stream reports
what the plain entry with inflate_ref_wrap = 0 reports for the block's BSIZE + 1 bytes in ISIZE bytes of room, an
ISIZE that is too small as "incorrect length check".  Every case is a few hundred KB at the most."""
import ctypes
import struct
import zlib

import pytest

import bgzfcases as bc
import corpus
import memberscases as mc
from memberscases import BGZF_EOF, CAPACITY, cap4, good, member, text

pytestmark = pytest.mark.gpu
LENGTH_CHECK = (-3, 2, "incorrect length check")  # ZS_DATA_ERROR, ZS_PHASE_PROCESS, zlib's words


def dec(engine, streams, caps, members="bgzf"):
    """(the streams' fields, the members' index, the members sized from their headers)"""
    got = engine.decompress_batch_detailed(streams, "gzip", out_caps=caps, members=members)
    return got, engine.last_members(), engine.last_bgzf_trusted()


def plain(engine, streams, caps):
    try:
        engine.set_option("inflate_ref_wrap", 0)
        return engine.decompress_batch_detailed(streams, "gzip", out_caps=caps)
    finally:
        engine.set_option("inflate_ref_wrap", 1)


def nested():
    """a level-0 block whose stored data is a complete BGZF file of more blocks than sync_pass (8)"""
    inner = bc.bgzf(text(120, 4), 10)
    assert len(mc.candidates(inner)) > 8
    return bc.block(inner, level=0) + bc.block(text(9)) + BGZF_EOF


def truthful():
    b100 = bc.bgzf(text(300), 100)
    return {
        "one block + EOF": bc.bgzf(text(500, 1)),
        "EOF only": BGZF_EOF,
        "three blocks of 100 (in place)": b100,
        "three blocks of 101 (staging)": bc.bgzf(text(303, 2), 101),
        "300 one-byte blocks": bc.bgzf(text(300, 3), 1),
        "one 65,280-byte block": bc.bgzf(corpus.rand(1, 20000) + text(45280, 4), 65280),
        "XY then BC": bc.xy_block(text(500, 3)) + bc.block(text(20)) + BGZF_EOF,
        "mixed BGZF / plain / FNAME": bc.block(text(40, 1)) + member(text(33, 2)) + mc.hand_member(text(50, 3), name=b"n.txt")
                                      + bc.block(text(30, 4)) + BGZF_EOF,
        "trailing zeros": b100 + b"\x00" * 37,
        "trailing noise": b100 + corpus.rand(5, 50),
        "a BGZF file stored inside a block": nested(),
        "BSIZE 0 (nothing to follow)": mc.bgzf(text(300, 6), block=100),
    }


def headers_trusted(s):
    """the members of a stream whose size comes from their header, counted in Python"""
    return sum(bc.trusted(s, a) is not None for a, _ in mc.walk(s)[0])


@pytest.fixture(scope="module")
def reference(engine):
    """members=True over the truthful streams, one call, computed once: {name: (fields, index)}"""
    t = truthful()
    streams = list(t.values())
    got, idx, trusted = dec(engine, streams, [len(mc.walk(s)[1]) for s in streams], members=True)
    assert trusted == 0  # no header is trusted by a members=True call
    return {k: (g, i) for k, g, i in zip(t, got, idx)}


@pytest.mark.parametrize("name", list(truthful()))
def test_a_truthful_stream_equals_members_true(engine, reference, name):
    s = truthful()[name]
    idx, out, end, ok = mc.walk(s)
    assert ok
    for cap in (len(out), len(out) + 8):
        (g,), (i,), trusted = dec(engine, [s], [cap])
        assert g == reference[name][0] == good(s), (name, g[:3], g[4:])
        assert i == reference[name][1] == idx
        assert trusted == headers_trusted(s), name
    if "mixed" in name:
        assert headers_trusted(s) == 3 and len(idx) == 5
    elif "BSIZE 0" in name:
        assert headers_trusted(s) == 1 and len(idx) == 4
    else:
        assert headers_trusted(s) == len(idx) and bc.chain(s)[2] == idx  # the index read from the headers


def test_a_trusted_block_needs_no_tail_round(engine):
    """members=True sizes the outer block by decoding it and its lane is stopped by its bound (the stored BGZF file holds
    more than sync_pass candidates), so it takes a tail round (tests/test_bgzf_host.py shows it on the CPU); "bgzf" reads
    no byte between the header and the trailer.  zs_last_phase_ms answers -1 for a phase that did not run and the time
    of the tail rounds for "members_size" after a _bgzf call, whose sizing launch is "bgzf_size": no time at all."""
    s = nested()
    out = mc.walk(s)[1]
    engine.set_timing(True)
    try:
        (g,), _, trusted = dec(engine, [s], [len(out)])
        tail, sizing = engine.last_ms("members_size"), engine.last_ms("bgzf_size")
        (m,), _, _ = dec(engine, [s], [len(out)], members=True)
        tail_m, sizing_m = engine.last_ms("members_size"), engine.last_ms("bgzf_size")
    finally:
        engine.set_timing(False)
    assert g == m == good(s) and trusted == 3
    assert tail <= 0 and sizing > 0
    assert tail_m > 0 and sizing_m <= 0


def test_bgzf_blocks_decode_on_the_lane_path(engine):
    """FEXTRA alone no longer sends a member to the exact kernel when it decodes with zlib semantics, as the members of
    these calls do: a BGZF file's data blocks are the lane kernel's (the exact kernel took 52 ms for the 1,029 blocks
    of DESIGN 5's file, the lane kernel takes 0.5).  A name in the header still does."""
    s = bc.bgzf(text(300), 100)
    for mode in ("bgzf", True):
        (g,), _, _ = dec(engine, [s], [300], members=mode)
        assert g == good(s) and engine.last_lane_count() >= 3, mode
    named = b"".join(mc.hand_member(text(100, k), extra=mc.bc_extra(0), name=b"n") for k in range(3))
    (g,), _, _ = dec(engine, [named], [300])
    assert g == good(named) and engine.last_lane_count() == 0


def test_full_size_blocks_decode_on_the_segmented_path(engine):
    """a small batch's members of more than 4 KiB of input are the segmented decode's, whose header parse takes an extra
    field that stands alone as the lane kernel's does: three blocks of 65,280 bytes (22 KB of input each) and the
    end-of-file block, none left to the exact kernel but for a name in the header"""
    data = text(3 * 65280, 21)
    s = bc.bgzf(data)
    assert all(b - a > 4096 for (a, _), (b, _) in zip(mc.walk(s)[0], mc.walk(s)[0][1:]))
    for mode in ("bgzf", True):
        (g,), idx, _ = dec(engine, [s], [len(data)], members=mode)
        assert g == (1, 0, "", data, len(s), zlib.crc32(data)) and len(idx[0]) == 4, mode
        assert engine.last_seg_count() == 3, mode
    named = b"".join(mc.hand_member(data[k * 65280:(k + 1) * 65280], extra=mc.bc_extra(0), name=b"n") for k in range(3))
    (g,), _, _ = dec(engine, [named], [len(data)])
    assert g[:4] == (1, 0, "", data) and engine.last_seg_count() == 0


def test_all_of_them_in_one_batch_and_through_the_pool(engine, reference):
    import zsamd

    t = truthful()
    streams = list(t.values())
    caps = [len(mc.walk(s)[1]) for s in streams]
    got, idx, trusted = dec(engine, streams, caps)
    assert got == [reference[k][0] for k in t] and idx == [reference[k][1] for k in t]
    assert trusted == sum(headers_trusted(s) for s in streams)
    assert engine.last_host_chunks() == 1
    # 0 after any other inflate call
    plain(engine, [BGZF_EOF], [0])
    assert engine.last_bgzf_trusted() == 0
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        assert pool.decompress_batch_detailed(streams, "gzip", out_caps=caps, members="bgzf") == got
        assert pool.decompress_batch(streams[:3], "gzip", members="bgzf") == [mc.walk(s)[1] for s in streams[:3]]
    finally:
        pool.close()


def _device(engine, streams, caps, members, guard=64):
    """the device entry over the streams at odd offsets in one blob, regions `guard` bytes of 0x5a apart: (the
    streams' fields as the host entries give them, the whole output buffer with the regions' unwritten tails, the
    index, the trusted count); asserts that no byte outside the regions rounded up to 4 changed"""
    import torch

    n = len(streams)
    blob, in_offs = bytearray(b"\x1f\x8b\x08\x04" * 4), []
    for k, s in enumerate(streams):
        blob += b"\x1f\x8b\x08\x04"[: 1 + k % 3]  # (odd offsets; the filler would pass the scan's test)
        in_offs.append(len(blob))
        blob += s
    blob += b"\x1f\x8b\x08\x04" * 4
    out_off, o = [], guard
    for c in caps:
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
                             d_check=d_chk.data_ptr(), members=members)
    torch.cuda.synchronize()
    assert bytes(d_in.cpu().numpy()) == bytes(blob)  # the input is only read
    out = bytes(d_out.cpu().numpy())
    keep = bytearray(b"\x01" * len(out))
    for a, c in zip(out_off, caps):
        keep[a:a + cap4(c)] = b"\x00" * cap4(c)
    assert all(b == 0x5a for b, k in zip(out, keep) if k)  # every canary is as it was
    msg = lambda m: engine._L.zs_inflate_message(m).decode()
    fields = [(st, ph, msg(m), out[a:a + l], c, k & 0xffffffff)
              for st, ph, m, l, c, k, a in zip(d_st.tolist(), d_ph.tolist(), d_msg.tolist(), d_len.tolist(), d_cons.tolist(),
                                               d_chk.tolist(), out_off)]
    return fields, engine.last_members(), engine.last_bgzf_trusted()


def test_the_device_entry_with_canaries_round_every_region(engine, reference):
    t = truthful()
    streams = list(t.values())
    caps = [cap4(len(mc.walk(s)[1])) for s in streams]
    got, idx, trusted = _device(engine, streams, caps, "bgzf")
    assert got == [reference[k][0] for k in t] and idx == [reference[k][1] for k in t]
    assert trusted == sum(headers_trusted(s) for s in streams)
    m, midx, mtrusted = _device(engine, streams, caps, True)
    assert m == got and midx == idx and mtrusted == 0


def corrupt_cases():
    """block 2 of 3 with its deflate data corrupted so that both sizings see the same member: a stored block's data
    byte (the CRC fails), a stored block's LEN (invalid lengths), a compressed block's bits early in the data where
    zlib finds an invalid code"""
    d = [text(500, 1), text(700, 2), text(300, 3)]
    blocks = [bc.block(d[0]), bc.block(d[1], level=0), bc.block(d[2])]
    a = bytearray(blocks[1])
    a[18 + 5 + 100] ^= 0x10  # a byte of the stored data
    b = bytearray(blocks[1])
    b[18 + 1] ^= 0x01  # LEN's low byte
    c = bc.block(d[1])
    for at in range(18 + 20, 18 + (len(c) - 26) // 4):
        x = bytearray(c)
        x[at] ^= 0x5a
        try:
            zlib.decompressobj(31).decompress(bytes(x))
        except zlib.error as e:
            if "invalid" in str(e):
                c = bytes(x)
                break
    else:
        raise AssertionError("no flip gives an invalid code")
    return [blocks[0] + bytes(m) + blocks[2] + BGZF_EOF for m in (a, b, c)], d[0], len(blocks[0])


def test_failures_are_those_of_members_true(engine):
    corrupt, first, start2 = corrupt_cases()
    whole = bc.bgzf(text(900, 5), 300)
    last = len(whole) - 28 - len(bc.block(text(900, 5)[600:]))  # the last data block's start
    size = len(whole) - 28 - last
    cuts = [last + c for c in (7, 17, size // 2, size - 8, size - 1)]  # in the header (twice), the data, the trailer (twice)
    truncated = [whole[:c] for c in cuts]
    streams = corrupt + truncated + [whole, whole, whole]
    caps = [1500] * 3 + [900] * 5 + [899, 0, 900]
    got, idx, trusted = dec(engine, streams, caps)
    m, midx, _ = dec(engine, streams, caps, members=True)
    assert got == m and idx[3:] == midx[3:]  # (a corrupt block's header still says where the next one starts)
    for g in got[:3]:
        assert g[0] == -3 and g[3] == first and g[4] == start2 and g[5] == 0, g[:3]
    for g in got[3:8]:
        assert g[0] != 1 and g[3] == text(900, 5)[:600] and g[4] == last and g[5] == 0, g[:3]
    assert got[8] == CAPACITY + (text(900, 5)[:600], last, 0)  # one byte short: the last data block gets no room
    assert got[9] == CAPACITY + (b"", 0, 0)
    assert got[10] == good(whole)
    # the blocks in front of the failure were sized from their headers, the truncated one from its bytes
    assert trusted == 3 * 4 + 5 * 2 + 2 + 0 + 4


def lying_cases(engine):
    """[(name, the stream, block 2's start, the bytes and the room its header claims)], block 2 of 3 in each"""
    d = [text(500, 1), text(700, 2), text(300, 3)]
    b1, b3 = bc.block(d[0]), bc.block(d[2])
    low_d, low_b, low_isize = bc.crc_low_block()
    cases = []
    for name, b2 in [("ISIZE one too small", bc.block(d[1], isize=699)), ("ISIZE one too large", bc.block(d[1], isize=701)),
                     ("BSIZE shortened by 3", bc.block(d[1], bsize_delta=-3)),
                     ("BSIZE shortened by 3, still trusted", bytes(bc.block(low_d, bsize_delta=-3)))]:
        s = b1 + b2 + b3 + BGZF_EOF
        cases.append((name, s, len(b1), bc.trusted(s, len(b1))))
    assert cases[3][3] == (len(b1) + len(low_b) - 3, low_isize)
    return cases, d[0]


def test_lying_headers(engine):
    cases, first = lying_cases(engine)
    ok = bc.bgzf(text(640, 8), 320)
    streams, want = [ok], [good(ok)]
    for name, s, start, t in cases:
        if t is None:
            # the shortened size moves the word read as ISIZE into the CRC: above 65,536, the header is not trusted
            # and the block is sized from its data -- nothing lies to the decode
            assert name == "BSIZE shortened by 3"
            want.append(good(s))
        else:
            end, isize = t
            (p,), = [plain(engine, [s[start:end]], [isize])]
            assert p[0] != 1, name
            head = LENGTH_CHECK if p[:3] == CAPACITY else p[:3]
            want.append(head + (first, start, 0))
        streams += [s, ok]
        want.append(good(ok))
    assert want[1][:3] == LENGTH_CHECK  # too small: the mapping
    assert want[3][0] == -3 and want[3][2] == "incorrect length check"  # too large: the decoder's own
    assert want[7][0] != 1
    # room for the three blocks as the headers size them (a stream whose out_cap the claimed ISIZE passes gives the block
    # no room and reports the capacity outcome, as in _members)
    caps = [640]
    for _, _, _, t in cases:
        caps += [cap4(500 + (t[1] if t else 700) + 300), 640]
    got, _, trusted = dec(engine, streams, caps)
    assert got == want, [(g[:3], w[:3]) for g, w in zip(got, want)]
    # ... through the device entry: the same fields, every neighbour and every canary untouched
    dgot, _, dtrusted = _device(engine, streams, caps, "bgzf")
    assert dgot == want and dtrusted == trusted


def test_python_sizes_the_output_from_the_headers(engine):
    t = truthful()
    names = [k for k in t if bc.chain(t[k])[0]]
    assert len(names) == len(t) - 2  # all but the mixed chain and the BSIZE 0 file
    streams = [t[k] for k in names]
    assert engine.decompress_batch(streams, "gzip", members="bgzf") == [mc.walk(s)[1] for s in streams]
    assert engine.last_bgzf_trusted() == sum(headers_trusted(s) for s in streams)
    with pytest.raises(ValueError, match="stream 1 is not BGZF throughout: give out_caps"):
        engine.decompress_batch([BGZF_EOF, t["mixed BGZF / plain / FNAME"]], "gzip", members="bgzf")
    # members=True keeps its rule
    with pytest.raises(ValueError):
        engine.decompress_batch([BGZF_EOF], "gzip", members=True)
