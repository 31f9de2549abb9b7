"""CPU-side checks of the restart-point entries: libzsgpu.so exports them, include/zs_gpu.h declares
them with the reference citation, the Python binding carries the keyword, every refusal is decided
before the context is looked at (a null context still gets the refusal's text), the new message has
its index, and zs_wrapper_header_len parses the wrappers' headers."""
import ctypes
import gzip
import inspect
import io
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_inflate_batch_restart_device", "zs_inflate_batch_restart", "zs_pool_inflate_batch_restart"]
SEG_MAX = 67108863


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_restart_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES + ["zs_wrapper_header_len", "zs_last_flush_index"] if not hasattr(L, s)] == []


def test_header_declares_them_with_the_reference_citation():
    src = header()
    for name in ENTRIES:
        m = re.search(r"/\*([^/]*?)\*/\s*int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        assert "inflate.ts:1267-1337" in m.group(1), name
        args = " ".join(m.group(2).split())
        assert args.endswith("const uint64_t *restart_first, const uint32_t *restart_in, const uint32_t *restart_out"), name
    assert re.search(r"uint32_t zs_wrapper_header_len\(int wbits, const uint8_t \*in, uint32_t in_len\);", src)
    assert re.search(r"uint64_t zs_last_flush_index\(zs_ctx \*ctx, uint32_t \*in_pos, uint64_t cap\);", src)
    flat = " ".join(src.replace("*", " ").split())
    for text in ('"restart points do not decode the stream"', "67,108,863 segments", "whatever the context's option says",
                 "FHCRC is skipped, not verified", "A raw stream has no trailer", "no _dict or _auto forms",
                 "Not offered on the pool", "inflate.ts:1285-1337", "inffast.ts:133-147"):
        assert text in flat, text


def test_python_signatures():
    import zsamd

    for cls in (zsamd.Engine, zsamd.Pool):
        for meth in ("decompress_batch", "decompress_batch_raw", "decompress_batch_detailed"):
            assert inspect.signature(getattr(cls, meth)).parameters["restart"].default is None, (cls, meth)
    assert inspect.signature(zsamd.Engine.decompress_device).parameters["restart"].default is None
    assert callable(zsamd.Engine.last_flush_index) and callable(zsamd.wrapper_header_len)
    assert not hasattr(zsamd.Pool, "last_flush_index")


def test_the_keyword_prepends_the_start_and_needs_capacities():
    import zsamd

    g = gzip_header(name=b"a.txt") + b"\x03\x00" + bytes(8)
    first, rin, rout = zsamd.decompress_restart([g, g], "gzip", [[(30, 4), (40, 9)], None], [16, 16])
    assert (list(first), list(rin)[:4], list(rout)[:4]) == ([0, 3, 4], [16, 30, 40, 16], [0, 4, 9, 0])
    first, rin, rout = zsamd.decompress_restart([b"xx"], "deflate", [[]], [16])
    assert (list(first), rin[0], rout[0]) == ([0, 1], 2, 0)
    assert zsamd.decompress_restart([b"xx"], "deflate-raw", [[(7, 1)]], [16])[1][0] == 0
    with pytest.raises(ValueError):
        zsamd.decompress_restart([b"xx"], "deflate", [[]], None)
    with pytest.raises(ValueError):
        zsamd.decompress_restart([b"xx"], "deflate", [[]], [16], zdict=b"d")
    with pytest.raises(ValueError):
        zsamd.decompress_restart([b"xx"], "deflate", [[], []], [16])
    with pytest.raises(ValueError):
        zsamd.decompress_restart([b"xx"], "deflate", [[(1, -1)]], [16])


def test_every_refusal_is_decided_before_the_context():
    import zsamd

    L = zsamd.lib()
    u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    i32 = lambda: (ctypes.c_int32 * 2)()
    out = ctypes.create_string_buffer(64)

    def call(wbits, n, in_len, first, rin, rout, out_off=u64(0, 0), out_cap=u32(16, 16)):
        res = [i32(), i32(), i32(), u32(0, 0), u32(0, 0), u32(0, 0)]
        host = (wbits, n, b"x" * 64, u64(0, 0), in_len, out, out_off, out_cap, *res, first, rin, rout)
        got = []
        for fn, ctx in ((L.zs_inflate_batch_restart, None), (L.zs_pool_inflate_batch_restart, None)):
            r = fn(ctx, *host)
            got.append((r, L.zs_last_error().decode()))
        r = L.zs_inflate_batch_restart_device(None, wbits, n, None, u64(0, 0), in_len, None, out_off, out_cap, None, None,
                                              None, None, None, None, None, first, rin, rout)
        got.append((r, L.zs_last_error().decode()))
        return got

    def refused(text, *a, **kw):
        got = call(*a, **kw)
        assert got == [(-2, text)] * 3, (text, got)

    ln = u32(40, 40)
    refused("deflate64 has no restart points", -16, 1, ln, None, None, None)
    refused("unsupported windowBits (use -15, 15 or 31)", 14, 1, ln, None, None, None)
    refused("null restart arrays", 15, 1, ln, None, u32(2), u32(0))
    refused("null restart arrays", 15, 1, ln, u64(0, 1), None, u32(0))
    refused("null restart arrays", 15, 1, ln, u64(0, 1), u32(2), None)
    refused("a stream without its first point", 15, 2, ln, u64(0, 1, 1), u32(2), u32(0))
    refused("too many restart points (more than 67,108,863 segments in one call)", 15, 1, ln, u64(0, SEG_MAX + 1), u32(2),
            u32(0))
    refused("the first point's out_pos must be 0", 15, 1, ln, u64(0, 1), u32(2), u32(1))
    refused("restart in_pos must increase by at least 5", 15, 1, ln, u64(0, 2), u32(2, 6), u32(0, 9))
    refused("restart in_pos must increase by at least 5", 15, 1, ln, u64(0, 3), u32(2, 10, 9), u32(0, 9, 9))
    refused("restart out_pos must not decrease", 15, 1, ln, u64(0, 3), u32(2, 10, 20), u32(0, 9, 8))
    refused("restart in_pos past the stream's input", 15, 1, ln, u64(0, 2), u32(2, 41), u32(0, 9))
    # the device entry's alignment rule comes last; the host entries take any offset and capacity
    ok = (15, 1, ln, u64(0, 2), u32(2, 40), u32(0, 9))
    for kw in ({"out_off": u64(2, 0)}, {"out_cap": u32(18, 16)}):
        got = call(*ok, **kw)
        assert got[2] == (-2, "output offsets/capacities must be multiples of 4")
        assert got[0] == (-2, "null context") and got[1] == (-2, "null pool")
    # nothing to refuse: then the context is looked at
    assert call(*ok) == [(-2, "null context"), (-2, "null pool"), (-2, "null context")]


def test_the_new_message_has_its_index_and_the_old_ones_keep_theirs():
    import zsamd

    L = zsamd.lib()
    old = ["", "incorrect header check", "unknown compression method", "invalid window size", "unknown header flags set",
           "header crc mismatch", "invalid block type", "invalid stored block lengths",
           "too many length or distance symbols", "too many length", "invalid code lengths set",
           "invalid bit length repeat", "invalid code -- missing end-of-block", "invalid literal/lengths set",
           "invalid distances set", "invalid literal/length code", "invalid distance code",
           "invalid distance too far back", "incorrect data check", "incorrect length check", "output capacity exceeded"]
    assert [L.zs_inflate_message(i).decode() for i in range(len(old))] == old
    assert L.zs_inflate_message(len(old)) == b"restart points do not decode the stream"
    assert L.zs_inflate_message(len(old) + 1) == b""


def gzip_header(name=None, extra=None, comment=None, hcrc=False):
    flg = (8 if name is not None else 0) | (4 if extra is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + bytes(4) + b"\x00\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc:
        h += b"\xab\xcd"
    return h


def test_wrapper_header_len():
    import zsamd

    f = zsamd.wrapper_header_len
    assert f(b"", "deflate-raw") == 0 and f(b"anything", "deflate-raw") == 0
    assert f(b"\x78\x9c", "deflate") == 2 and f(b"", "deflate") == 2
    headers = [gzip_header(), gzip_header(name=b"file.txt"), gzip_header(extra=b"\x01\x02\x03\x04\x05"),
               gzip_header(extra=b""), gzip_header(comment=b"a comment"), gzip_header(hcrc=True),
               gzip_header(name=b"n", extra=b"ex\x00tra", comment=b"c", hcrc=True), gzip_header(name=b"", comment=b"")]
    b = io.BytesIO()
    with gzip.GzipFile(filename="data.bin", fileobj=b, mode="wb", mtime=1) as fh:
        fh.write(b"hello")
    py = b.getvalue()
    assert py[3] & 8
    assert f(py, "gzip") == 10 + len(b"data.bin") + 1
    headers.append(py[:19])
    assert [len(h) for h in headers[:2]] == [10, 19]
    for h in headers:
        assert f(h, "gzip") == len(h), h
        assert f(h + b"\x03\x00" + bytes(8), "gzip") == len(h), h
        for k in range(len(h)):  # every truncation
            assert f(h[:k], "gzip") == 0, (h, k)
    # malformed: the magic, the method, a reserved flag
    good = gzip_header(name=b"x")
    for at, v in ((0, 0x1e), (1, 0x8c), (2, 7), (3, 0x28), (3, 0x48), (3, 0x88)):
        bad = bytearray(good)
        bad[at] = v
        assert f(bytes(bad), "gzip") == 0, (at, v)
