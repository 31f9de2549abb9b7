"""CPU-side checks of the entries that decode every member of multi-member gzip files: libzsgpu.so exports
them, include/zs_gpu.h declares them with exactly their plain counterparts' arguments, every refusal is
decided before the context is looked at (a null context still gets the refusal's text) and in its order,
and the Python binding carries members=True."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("zs_inflate_batch_members_device", "zs_inflate_batch_device_ex"), ("zs_inflate_batch_members", "zs_inflate_batch_ex"),
         ("zs_pool_inflate_batch_members", "zs_pool_inflate_batch")]
GZIP_ONLY = "members are a gzip notion (use windowBits 31)"
CAPS = "members are found with given capacities only"
ALIGN = "output offsets/capacities must be multiples of 4"


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_four_symbols():
    import zsamd

    L = zsamd.lib()
    assert [s for s in [a for a, _ in PAIRS] + ["zs_last_members"] if not hasattr(L, s)] == []


def test_header_declares_them_with_their_counterparts_arguments():
    src = header()

    def args(name):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        return " ".join(m.group(1).split())

    for new, old in PAIRS:
        assert args(new) == args(old), new
    assert re.search(r"uint64_t zs_last_members\(zs_ctx \*ctx, uint64_t \*member_first, uint32_t \*member_in, "
                     r"uint32_t \*member_out,\s*uint64_t cap\);", src)
    flat = " ".join(src.replace("*", " ").split())
    for text in ("members are a gzip notion", "zs_last_host_chunks = 1", '"members_scan", "members_size" and "members_stitch"',
                 "67,108,863 candidates plus streams", "once more per tail round", "following BSIZE", "restart points inside members",
                 'zlib or raw "members"', "decoding a range of members (a seek)", "zs_last_members on the pool"):
        assert text in flat, text


def test_every_refusal_is_decided_before_the_context_and_in_its_order():
    import zsamd

    L = zsamd.lib()
    u64 = lambda *v: (ctypes.c_uint64 * len(v))(*v)
    u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)
    i32 = lambda: (ctypes.c_int32 * 2)()
    out = ctypes.create_string_buffer(64)

    def call(wbits, n, out_off=u64(0, 16), out_cap=u32(16, 16)):
        res = [i32(), i32(), i32(), u32(0, 0), u32(0, 0), u32(0, 0)]
        host = (wbits, n, b"x" * 64, u64(0, 32), u32(32, 32), out, out_off, out_cap, *res)
        got = []
        for fn in (L.zs_inflate_batch_members, L.zs_pool_inflate_batch_members):
            r = fn(None, *host)
            got.append((r, L.zs_last_error().decode()))
        r = L.zs_inflate_batch_members_device(None, wbits, n, None, u64(0, 32), u32(32, 32), None, out_off, out_cap, None,
                                              None, None, None, None, None, None)
        got.append((r, L.zs_last_error().decode()))
        return got

    # 1. the format, even of an empty batch and whatever else is wrong
    for wbits in (-15, 15, -16, 0, 30):
        assert call(wbits, 2, out_off=u64(2, 16), out_cap=None) == [(-2, GZIP_ONLY)] * 3, wbits
        assert call(wbits, 0) == [(-2, GZIP_ONLY)] * 3, wbits
    # 2. the capacities must be given, whatever the offsets are
    assert call(31, 2, out_cap=None) == [(-2, CAPS)] * 3
    assert call(31, 2, out_off=u64(2, 16), out_cap=None) == [(-2, CAPS)] * 3
    # 3. the device entry's alignment rule last; the host entries take any offset and capacity
    for kw in ({"out_off": u64(2, 16)}, {"out_cap": u32(18, 16)}):
        got = call(31, 2, **kw)
        assert got[2] == (-2, ALIGN)
        assert got[0] == (-2, "null context") and got[1] == (-2, "null pool")
    # nothing to refuse: then the context is looked at
    assert call(31, 2) == [(-2, "null context"), (-2, "null pool"), (-2, "null context")]
    # no context, no record: the query answers 0
    assert L.zs_last_members(None, None, None, None, 0) == 0


def test_python_carries_the_keyword():
    import zsamd

    assert zsamd.decompress_members(True, "gzip", [16]) is True
    assert zsamd.decompress_members(False, "deflate", None) is False and zsamd.decompress_members(None, "gzip", None) is False
    for args in (("deflate", [16]), ("deflate-raw", [16]), ("gzip", None)):
        with pytest.raises(ValueError):
            zsamd.decompress_members(True, *args)
    with pytest.raises(ValueError):
        zsamd.decompress_members(True, "gzip", [16], zdict=b"d")
    with pytest.raises(ValueError):
        zsamd.decompress_members(True, "gzip", [16], restart="scan")
    for cls in (zsamd.Engine, zsamd.Pool):
        for fn in ("decompress_batch", "decompress_batch_raw", "decompress_batch_detailed"):
            assert "members" in inspect.signature(getattr(cls, fn)).parameters, (cls, fn)
    assert "members" in inspect.signature(zsamd.Engine.decompress_device).parameters
    assert callable(zsamd.Engine.last_members) and not hasattr(zsamd.Pool, "last_members")
