"""GPU tests of the decode of multi-member gzip files (zs_inflate_batch_members*, inflate_members.hip,
DESIGN 4.14): members=True decodes every member and concatenates the outputs, as Python's zlib does when a
decompressobj(31) is restarted on unused_data (memberscases.walk); a failing stream reports what the plain
entry with inflate_ref_wrap = 0 reports for the failing member's bytes.  The smallest shapes at which the
scan, the sizing lanes, the plan, the two output routes and the stitch can go wrong."""
import ctypes
import zlib

import pytest

import corpus
import memberscases as mc
from memberscases import BGZF_EOF, CAPACITY, cap4, good, member, text

pytestmark = pytest.mark.gpu


def dec(engine, streams, caps):
    got = engine.decompress_batch_detailed(streams, "gzip", out_caps=caps, members=True)
    return got, engine.last_members()


def plain(engine, streams, caps):
    try:
        engine.set_option("inflate_ref_wrap", 0)
        return engine.decompress_batch_detailed(streams, "gzip", out_caps=caps)
    finally:
        engine.set_option("inflate_ref_wrap", 1)


def failed(engine, s, cap):
    """the fields of a stream whose member k fails: the plain entry's status, phase and message for s[start_k:]
    with the room that is left, the complete members' bytes, consumed = start_k, check 0"""
    idx, out, at, ok = mc.walk(s)
    assert not ok
    (st, ph, msg, _, _, _), = plain(engine, [s[at:]], [cap - len(out)])
    assert st != 1
    return (st, ph, msg, out, at, 0)


def all_good(engine, streams, slack=8):
    caps = [len(mc.walk(s)[1]) + slack for s in streams]
    got, idx = dec(engine, streams, caps)
    for k, (s, g, i) in enumerate(zip(streams, got, idx)):
        assert g == good(s), (k, g[:3], g[4:], len(g[3]))
        assert i == mc.walk(s)[0], k
    return got


def test_more_candidates_than_the_list_holds_at_first(engine):
    """a stored member whose data is 1f 8b 08 00 five thousand times: the candidates outgrow the list a context starts
    with (1,024 and one per 2 KiB of input), so the emit pass and the sizing run once more over the grown list; every
    false start is an ERROR lane, the true member takes a tail round, the member behind it is found"""
    s = member(b"\x1f\x8b\x08\x00" * 5000, 0) + member(b"tail")
    assert len(mc.candidates(s)) == 5001
    (g,), = [all_good(engine, [s], 0)]
    assert g[3] == b"\x1f\x8b\x08\x00" * 5000 + b"tail"


def test_empty_members_and_the_empty_input(engine):
    e, a = member(b""), member(b"abc")
    streams = [a + e, e + a + member(b"de"), a + e + member(b"de"), a + member(b"de") + e, BGZF_EOF, e, e + e + e]
    for slack in (0, 8):
        all_good(engine, streams, slack)
    # an input of length 0: the plain entry's outcome
    got, idx = dec(engine, [b"", a + e], [8, 3])
    assert got[0] == plain(engine, [b""], [8])[0] and got[0][0] != 1 and got[1] == good(a + e)
    assert idx == [[(0, 0)], mc.walk(a + e)[0]]


@pytest.mark.parametrize("slack", [0, 8])
def test_member_lengths_on_the_staged_and_the_in_place_route(engine, slack):
    staged = b"".join(member(text(n, n)) for n in range(1, 8))  # every out_pos mod 4
    in_place = b"".join(member(text(n, n)) for n in (4, 8, 12))
    all_good(engine, [staged], slack)
    all_good(engine, [in_place], slack)
    all_good(engine, [in_place, in_place + member(b"xyz")], slack)  # (a last member of any length stays in place)
    all_good(engine, [in_place, staged, member(b"q")], slack)


def test_a_hand_built_header_on_a_member_that_is_not_the_first(engine):
    h = mc.hand_member(text(777, 3), extra=mc.bc_extra(0x1234) + b"XY\x03\x00abc", name=b"a name.txt", comment=b"a comment", fhcrc=True)
    all_good(engine, [member(text(100)) + h + member(b"tail"), h + h])


@pytest.mark.parametrize("d", [-3, -2, -1, 0, 1])
def test_the_pattern_across_the_scans_first_tile_boundary(engine, d):
    """one stream in the call, so it starts at an aligned address and its first tile ends at byte 4096: a level-0
    first member sized so that the second member's 1f 8b 08 xx starts at 4096 + d"""
    n = 4096 + d - (10 + 5 + 8)  # header, one stored block's 5 bytes, trailer
    s = member(corpus.rand(21, n), 0) + member(text(100, 2))
    assert s[4096 + d:4096 + d + 3] == b"\x1f\x8b\x08" and mc.walk(s)[0][1][0] == 4096 + d
    all_good(engine, [s])


def test_130_tiny_members_in_one_stream(engine):
    s = b"".join(member(bytes([65 + k % 26]) * (1 + k % 3)) for k in range(130))
    (g,), = [all_good(engine, [s], 0)]
    assert len(mc.walk(s)[0]) == 130 and len(g[3]) == sum(1 + k % 3 for k in range(130))


def test_two_large_members_with_a_tiny_one_between(engine):
    big = [corpus.rand(k, 40000) + text(150000, k) for k in (1, 2)]
    m = [member(b) for b in big]
    assert all(len(x) > 65536 for x in m)  # over inflate_wave_min (32,768) in mid-stream
    all_good(engine, [m[0] + member(b"12345") + m[1]])


def test_stored_gz_files_inside_a_member(engine):
    s12, d12, _ = mc.stored_gz_case(12)
    s3, d3, _ = mc.stored_gz_case(3, seed=40)
    got = all_good(engine, [s12, s3])
    assert [g[3] for g in got] == [d12, d3]
    try:
        engine.set_option("sync_pass", 1)
        assert [g[3] for g in all_good(engine, [s3, s12, member(b"x")])] == [d3, d12, b"x"]
    finally:
        engine.set_option("sync_pass", 8)


def test_trailing_bytes(engine):
    base = member(text(40)) + member(b"xy")
    # ignored: zeros, noise, a start that fails the four-byte test (too short; a reserved flag bit), consumed at the last trailer
    tails = [b"\x00" * 37, corpus.rand(5, 50), b"\x1f\x8b\x08", b"\x1f\x8b\x08\xe0\x00", b"\x1f\x8b"]
    got = all_good(engine, [base + t for t in tails])
    assert [g[4] for g in got] == [len(base)] * len(tails)
    # 1f 8b 08 00 + garbage IS a member and fails the stream, with the plain entry's fields; so is 1f 8b 08 + a valid
    # flag byte + one byte: a member cut inside its header
    bad = [base + b"\x1f\x8b\x08\x00" + b"\x55" * 30, base + b"\x1f\x8b\x08\x00\x00"]
    got, idx = dec(engine, bad + [base], [64, 64, 64])
    assert got[:2] == [failed(engine, s, 64) for s in bad] and got[2] == good(base)
    assert [g[3] for g in got[:2]] == [text(40) + b"xy"] * 2 and [g[4] for g in got[:2]] == [len(base)] * 2
    assert [len(i) for i in idx] == [3, 3, 2]


@pytest.mark.parametrize("which", ["crc", "isize"])
def test_a_flipped_trailer_byte_in_member_2_of_3(engine, which):
    parts = [member(text(500, 1)), member(text(700, 2)), member(text(300, 3))]
    flip = bytearray(parts[1])
    flip[-8 if which == "crc" else -4] ^= 0x10
    s = parts[0] + bytes(flip) + parts[2]
    ok = b"".join(parts)
    got, idx = dec(engine, [ok, s, ok], [1508, 1508, 1500])
    want = failed(engine, s, 1508)
    assert got[1] == want and want[0] == -3 and want[3] == text(500, 1) and want[4] == len(parts[0]) and want[5] == 0
    assert got[0] == got[2] == good(ok)  # the neighbours are untouched


def test_the_last_member_truncated(engine):
    a, b = member(text(40)), mc.hand_member(text(900, 2), name=b"file")
    cuts = (7, 12, len(b) // 2, len(b) - 8, len(b) - 1)  # inside the header, the name, the data, the trailer (twice)
    streams = [a + b[:c] for c in cuts]
    got, _ = dec(engine, streams, [1000] * len(cuts))
    assert got == [failed(engine, s, 1000) for s in streams]
    assert all(g[3] == text(40) and g[4] == len(a) for g in got)


def test_capacity(engine):
    lens = (4, 5, 2, 0, 9)
    datas = [text(n, n + 1) for n in lens]
    s = b"".join(member(d) for d in datas)
    starts = [a for a, _ in mc.walk(s)[0]]
    whole = b"".join(datas)
    cases = [(20, None), (19, 4), (11, 4), (10, 2), (8, 1), (3, 0), (0, 0)]  # (capacity, the first member that does not fit)
    got, _ = dec(engine, [s] * len(cases), [c for c, _ in cases])
    for (cap, k), g in zip(cases, got):
        if k is None:
            assert g == good(s), cap
        else:
            # the first member that does not fit is given no room: the plain entry's capacity outcome
            fit = sum(lens[:k])
            assert g == CAPACITY + (whole[:fit], starts[k], 0), (cap, g[:3], g[4:])
            assert plain(engine, [s[starts[k]:]], [0])[0][:3] == CAPACITY


def _device(engine, streams, caps, in_offs, blob, guard=64):
    """the device entry over `blob`: (statuses, lengths, consumed, checks, the regions' bytes, the whole output, its
    offsets), regions `guard` bytes apart"""
    import torch

    n = len(streams)
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
                             d_check=d_chk.data_ptr(), members=True)
    torch.cuda.synchronize()
    assert bytes(d_in.cpu().numpy()) == bytes(blob)  # the input is only read
    out = bytes(d_out.cpu().numpy())
    lens = d_len.tolist()
    return (d_st.tolist(), lens, d_cons.tolist(), [x & 0xffffffff for x in d_chk.tolist()],
            [out[a:a + l] for a, l in zip(out_off, lens)], out, out_off)


def test_the_device_entry_keeps_inside_its_regions(engine):
    """inputs at odd offsets in one blob, 64-byte 0x5a guards between the regions: staged and in-place shapes, a
    stream that fails in its second member and one that runs out of capacity"""
    staged = b"".join(member(text(n, n)) for n in range(1, 8))
    in_place = b"".join(member(text(n, n)) for n in (4, 8, 12))
    broken = bytearray(member(text(500, 1)) + member(text(700, 2)))
    broken[-8] ^= 1
    streams = [staged, in_place, bytes(broken), staged, BGZF_EOF, member(text(5000, 9)) + member(text(3001, 8))]
    caps = [cap4(28), 24, 1200, 12, 0, 8004]
    blob, in_offs = bytearray(b"\x1f\x8b\x08\x00" * 4), []
    for k, s in enumerate(streams):
        blob += b"\x1f\x8b\x08\x00"[: 1 + k % 3]  # (odd offsets; the filler would pass the scan's test)
        in_offs.append(len(blob))
        blob += s
    blob += b"\x1f\x8b\x08\x00" * 4
    st, lens, cons, chk, outs, out, out_off = _device(engine, streams, caps, in_offs, blob)
    full = b"".join(text(n, n) for n in range(1, 8))
    assert st == [1, 1, -3, -5, 1, 1]
    assert outs == [full, mc.walk(in_place)[1], text(500, 1), full[:10], b"", text(5000, 9) + text(3001, 8)]
    assert cons == [len(staged), len(in_place), len(member(text(500, 1))), mc.walk(staged)[0][4][0], 28, len(streams[5])]
    assert chk == [zlib.crc32(full), zlib.crc32(mc.walk(in_place)[1]), 0, 0, 0, zlib.crc32(outs[5])]
    # no store leaves [out_off, out_off + cap rounded up to 4): every guard byte is as it was
    keep = bytearray(b"\x01" * len(out))
    for a, c in zip(out_off, caps):
        keep[a:a + cap4(c)] = b"\x00" * cap4(c)
    assert all(b == 0x5a for b, k in zip(out, keep) if k)
    assert engine.last_members() == [mc.walk(s)[0][:n] for s, n in zip(streams, (7, 3, 2, 5, 1, 2))]


def test_a_batch_of_five_streams_field_for_field(engine):
    counts = (1, 2, 40, 1, 3)
    parts = [[text(37 * (k + 1) + 11 * j, 10 * k + j) for j in range(c)] for k, c in enumerate(counts)]
    streams = [b"".join(member(d, (j + k) % 10) for j, d in enumerate(ds)) for k, ds in enumerate(parts)]
    caps = [len(b"".join(ds)) for ds in parts]
    got, idx = dec(engine, streams, caps)
    assert got == [good(s) for s in streams] and idx == [mc.walk(s)[0] for s in streams]
    assert [len(i) for i in idx] == list(counts)
    # the single-member streams are field for field the plain entry's
    p = plain(engine, [streams[0], streams[3]], [caps[0], caps[3]])
    assert [got[0], got[3]] == p
    # check = zlib's crc32 of the whole output = zs_crc32_combine over the members' values
    import zsamd

    for ds, g in zip(parts, got):
        c = 0
        for d in ds:
            c = zsamd.crc32_combine(c, zlib.crc32(d), len(d))
        assert g[5] == c == zlib.crc32(b"".join(ds))


def test_the_pool_decodes_members_too(engine):
    import zsamd

    streams = [b"".join(member(text(100 + 7 * j + k, j + k)) for j in range(k + 1)) for k in range(6)] + [BGZF_EOF]
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        got = pool.decompress_batch_detailed(streams, "gzip", out_caps=[len(mc.walk(s)[1]) for s in streams], members=True)
        assert got == [good(s) for s in streams]
    finally:
        pool.close()


def test_a_bgzf_shaped_file(engine):
    data = text(4 * 65280, 12)
    s = mc.bgzf(data)
    (g,), idx = dec(engine, [s], [len(data)])
    assert g == (1, 0, "", data, len(s), zlib.crc32(data))
    assert len(idx[0]) == 5 and [o for _, o in idx[0]] == [0, 65280, 2 * 65280, 3 * 65280, 4 * 65280]
    assert engine.last_host_chunks() == 1
