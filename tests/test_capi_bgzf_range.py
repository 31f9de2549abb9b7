"""CPU-side checks of the BGZF range entries: libzsgpu.so exports them, include/zs_gpu.h declares them
with the _bgzf entries' arguments plus the two arrays of virtual offsets behind in_len, every refusal is decided
before the context is looked at and in the stated order, zs_bgzf_range_out_len and zs_bgzf_voffset are host
arithmetic that agrees with a walk of the headers in Python, and the Python binding carries ranges=."""
import ctypes
import inspect
import os
import re

import pytest

import bgzfrangecases as rc
from bgzfrangecases import voff
from memberscases import BGZF_EOF, member, text

bc = rc.bc
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("zs_inflate_batch_bgzf_range_device", "zs_inflate_batch_bgzf_device"),
         ("zs_inflate_batch_bgzf_range", "zs_inflate_batch_bgzf"),
         ("zs_pool_inflate_batch_bgzf_range", "zs_pool_inflate_batch_bgzf")]
GZIP_ONLY = "members are a gzip notion (use windowBits 31)"
CAPS = "members are found with given capacities only"
ALIGN = "output offsets/capacities must be multiples of 4"
ARRAYS = "null virtual offset arrays"
ORDER = "a range's begin lies behind its end"
PAST = "a range's end lies past the stream's input"
MESSAGE = b"virtual offsets do not follow a chain of BGZF blocks"


def test_library_exports_the_symbols():
    import zsamd

    L = zsamd.lib()
    assert [s for s in [a for a, _ in PAIRS] + ["zs_bgzf_range_out_len", "zs_bgzf_voffset"] if not hasattr(L, s)] == []


def test_header_declares_them_with_the_bgzf_arguments_and_the_offsets_behind_in_len():
    src = open(os.path.join(ROOT, "include", "zs_gpu.h")).read()

    def args(name):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        return " ".join(m.group(1).split())

    for new, old in PAIRS:
        want = args(old).replace("const uint32_t *in_len,",
                                 "const uint32_t *in_len, const uint64_t *voff_begin, const uint64_t *voff_end,")
        assert args(new) == want, new
    assert ("int zs_bgzf_range_out_len(const uint8_t *in, uint32_t in_len, uint64_t voff_begin, uint64_t voff_end, "
            "uint64_t *total);") in src
    assert ("int zs_bgzf_voffset(const uint32_t *block_in, const uint32_t *block_out, uint64_t count, uint64_t upos, "
            "uint64_t *voff);") in src
    flat = " ".join(src.replace("*", " ").split())
    for t in ("coffset << 16 | uoffset", "SEVERAL STREAMS MAY NAME THE SAME INPUT BYTES", '"%s"' % MESSAGE.decode(),
              '"bgzf_range_place"', "must land on ce exactly", '"%s"' % ARRAYS, '"%s"' % ORDER, '"%s"' % PAST,
              "de-duplicating blocks shared by overlapping ranges"):
        assert t in flat, t
    # the range is no longer listed as not built
    for line in flat.split(" - "):
        if line.startswith("Not built"):
            assert "a seek by virtual offset" not in line, line


def test_the_message_has_its_index_behind_the_existing_ones():
    import zsamd

    L = zsamd.lib()
    assert L.zs_inflate_message(21) == b"restart points do not decode the stream"
    assert L.zs_inflate_message(22) == b""  # (kept empty: the restart entries' test pins it)
    assert L.zs_inflate_message(23) == MESSAGE
    assert L.zs_inflate_message(24) == b""


def test_every_refusal_is_decided_before_the_context_and_in_order():
    import zsamd

    L = zsamd.lib()
    u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    i32 = lambda: (ctypes.c_int32 * 2)()
    out = ctypes.create_string_buffer(64)
    OK = (u64(0, 0), u64(32 << 16, 5 << 16))

    def call(wbits, n, out_off=u64(0, 16), out_cap=u32(16, 16), vb=OK[0], ve=OK[1]):
        res = [i32(), i32(), i32(), u32(0, 0), u32(0, 0), u32(0, 0)]
        host = (wbits, n, b"x" * 64, u64(0, 32), u32(32, 32), vb, ve, out, out_off, out_cap, *res)
        got = []
        for fn in (L.zs_inflate_batch_bgzf_range, L.zs_pool_inflate_batch_bgzf_range):
            r = fn(None, *host)
            got.append((r, L.zs_last_error().decode()))
        r = L.zs_inflate_batch_bgzf_range_device(None, wbits, n, None, u64(0, 32), u32(32, 32), vb, ve, None, out_off,
                                                 out_cap, None, None, None, None, None, None, None)
        got.append((r, L.zs_last_error().decode()))
        return got

    # the _bgzf entries' refusals, in their order, whatever the offsets are
    bad = {"vb": None, "ve": u64(1, (33 << 16))}
    for wbits in (-15, 15, -16, 0, 30):
        assert call(wbits, 2, out_off=u64(2, 16), out_cap=None, **bad) == [(-2, GZIP_ONLY)] * 3, wbits
        assert call(wbits, 0) == [(-2, GZIP_ONLY)] * 3, wbits
    assert call(31, 2, out_cap=None, **bad) == [(-2, CAPS)] * 3
    got = call(31, 2, out_off=u64(2, 16), **bad)
    assert got[2] == (-2, ALIGN) and got[0] == got[1] == (-2, ARRAYS)  # (the host entries have no alignment rule)
    # then the offsets': the arrays, the order, the end -- stream by stream
    assert call(31, 2, vb=None) == [(-2, ARRAYS)] * 3 and call(31, 2, ve=None) == [(-2, ARRAYS)] * 3
    assert call(31, 2, vb=u64(0, (5 << 16) | 1)) == [(-2, ORDER)] * 3
    assert call(31, 2, vb=u64(0, (5 << 16) | 1), ve=u64(33 << 16, 5 << 16)) == [(-2, PAST)] * 3  # stream 0 first
    assert call(31, 2, ve=u64(32 << 16, 33 << 16)) == [(-2, PAST)] * 3
    assert call(31, 2, ve=u64((32 << 16) | 0xffff, 32 << 16)) == [(-2, "null context"), (-2, "null pool"), (-2, "null context")]
    # nothing to refuse: then the context is looked at
    assert call(31, 2) == [(-2, "null context"), (-2, "null pool"), (-2, "null context")]


def five():
    """five data blocks of 1, 3, 300, 64 and 200 bytes and the end-of-file block"""
    return b"".join(bc.block(text(n, k)) for k, n in enumerate((1, 3, 300, 64, 200))) + BGZF_EOF


def test_range_out_len_against_a_walk_of_the_headers():
    import zsamd

    L = zsamd.lib()

    def out_len(s, vb, ve):
        total = ctypes.c_uint64(77)
        r = L.zs_bgzf_range_out_len(s, len(s), vb, ve, ctypes.byref(total))
        assert zsamd.bgzf_range_out_len(s, vb, ve) == (total.value if r else None)
        return r, total.value

    s = five()
    b = rc.blocks(s)
    assert [x[2] for x in b] == [1, 3, 300, 64, 200, 0] and b[-1][1] == len(s)
    # every pair of (block start, uoffset in {0, 1, ISIZE - 1, ISIZE}), the end of the file included as a start
    offs = sorted({voff(st, u) for st, _, isize in b for u in (0, 1, max(isize - 1, 0), isize)} | {voff(len(s), 0)})
    seen = {0: 0, 1: 0}
    for vb in offs:
        for ve in offs:
            if vb > ve:
                assert out_len(s, vb, ve) == (0, 0)
                continue
            want = rc.out_len(s, vb, ve)
            assert out_len(s, vb, ve) == want, (hex(vb), hex(ve))
            seen[want[0]] += 1
            if want[0]:
                data, idx = rc.whole(s)
                upos = lambda v: dict(idx)[v >> 16] + (v & 0xffff)
                assert want[1] == upos(ve) - upos(vb)
    assert seen[0] >= 20 and seen[1] >= 200  # (uoffset 1 of the end-of-file block lies above its ISIZE)
    # the other header failures, a range past the input, a null input
    for (vb, ve), _ in rc.header_failures(s).values():
        assert out_len(s, vb, ve) == (0, 0)
    assert out_len(s, 0, voff(len(s) + 1, 0)) == (0, 0)
    assert out_len(member(b"abc"), 0, voff(len(member(b"abc")), 0)) == (0, 0)
    assert L.zs_bgzf_range_out_len(None, 5, 0, 0, None) == 0
    # a header that lies is followed as it stands
    lie = bc.block(text(40), isize=41) + BGZF_EOF
    assert out_len(lie, voff(0, 3), voff(0, 41)) == (1, 38)


def test_voffset_against_the_same_walk():
    import zsamd

    L = zsamd.lib()
    big = bc.block(bytes(65536), level=1)  # a block of 65,536 bytes: more than a BGZF writer makes, legal to read
    assert bc.trusted(big, 0) == (len(big), 65536)
    for s in (five(), big + bc.block(text(10)) + BGZF_EOF):
        data, idx = rc.whole(s)
        for upos in sorted({0, 1, len(data) - 1, len(data), len(data) + 1} | {o + d for _, o in idx for d in (-1, 0, 1)}):
            if upos < 0:
                continue
            want = rc.voffset(idx, upos)
            assert zsamd.bgzf_voffset(idx, upos) == want, upos
            if want is not None and upos < len(data):
                # the offset names that byte: the range from it of one byte is data[upos]
                nxt = rc.voffset(idx, upos + 1)
                assert rc.expect(s, want, nxt)[3] == data[upos:upos + 1], upos
        assert zsamd.bgzf_voffset(idx, len(data)) == voff(len(s), 0)  # the end entry
        assert zsamd.bgzf_voffset(idx[:-1], idx[-2][1]) == voff(idx[-2][0], 0)  # without it: the last block's start
        assert zsamd.bgzf_voffset(idx[:-1], len(data) + 1) is None
    _, idx = rc.whole(big + bc.block(text(10)) + BGZF_EOF)
    assert zsamd.bgzf_voffset(idx, 65535) == voff(0, 65535) and zsamd.bgzf_voffset(idx, 65536) == voff(len(big), 0)
    # a difference that does not fit 16 bits: a plain gzip member of 70,000 bytes in a members index
    assert zsamd.bgzf_voffset([(0, 0), (900, 70000)], 65535) == voff(0, 65535)
    assert zsamd.bgzf_voffset([(0, 0), (900, 70000)], 65536) is None
    assert zsamd.bgzf_voffset([], 0) is None
    # a writer's list (last_bgzf_blocks) has the uncompressed side first
    assert zsamd.bgzf_voffset([(0, 0), (300, 210), (600, 400)], 301, written=True) == voff(210, 1)
    assert zsamd.bgzf_voffset([(0, 0), (300, 210), (600, 400)], 601, written=True) is None
    v = ctypes.c_uint64(9)
    assert L.zs_bgzf_voffset(None, None, 0, 0, ctypes.byref(v)) == 0 and v.value == 0


def test_python_carries_the_keyword():
    import zsamd

    s = five()
    for cls in (zsamd.Engine, zsamd.Pool):
        for fn in ("decompress_batch", "decompress_batch_raw", "decompress_batch_detailed"):
            assert "ranges" in inspect.signature(getattr(cls, fn)).parameters, (cls, fn)
    assert "ranges" in inspect.signature(zsamd.Engine.decompress_device).parameters
    assert zsamd.decompress_ranges(None, False, 3) is None
    vb, ve = zsamd.decompress_ranges([(1, 2), (3, 1 << 40)], "bgzf", 2)
    assert list(vb) == [1, 3] and list(ve) == [2, 1 << 40]
    for members in (False, True, "BGZF"):
        with pytest.raises(ValueError, match='ranges need members="bgzf"'):
            zsamd.decompress_ranges([(0, 0)], members, 1)
    with pytest.raises(ValueError):
        zsamd.decompress_ranges([(0, 0)], "bgzf", 2)
    b = rc.blocks(s)
    assert zsamd.bgzf_range_out_caps([s, s], [(voff(b[2][0], 1), voff(b[3][0], 2)), (0, 0)]) == [304, 0]
    with pytest.raises(ValueError, match="stream 1: the virtual offsets do not follow a chain of BGZF blocks"):
        zsamd.bgzf_range_out_caps([s, s], [(0, 0), (voff(3, 0), voff(b[1][0], 0))])
