"""CPU-side checks of the entries that find their restart points: libzsgpu.so exports them,
include/zs_gpu.h declares them with exactly their plain counterparts' arguments, every refusal is
decided before the context is looked at (a null context still gets the refusal's text), the Python
binding carries restart="scan", and option sync_pass is declared with its range."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("zs_inflate_batch_sync_device", "zs_inflate_batch_device_ex"), ("zs_inflate_batch_sync", "zs_inflate_batch_ex"),
         ("zs_pool_inflate_batch_sync", "zs_pool_inflate_batch")]


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in [a for a, _ in PAIRS] + ["zs_last_restart_points"] if not hasattr(L, s)] == []


def test_header_declares_them_with_their_counterparts_arguments():
    src = header()

    def args(name):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        return " ".join(m.group(1).split())

    for new, old in PAIRS:
        assert args(new) == args(old), new
    assert re.search(r"uint64_t zs_last_restart_points\(zs_ctx \*ctx, uint64_t \*restart_first, uint32_t \*restart_in, "
                     r"uint32_t \*restart_out,\s*uint64_t cap\);", src)
    flat = " ".join(src.replace("*", " ").split())
    for text in ("inflate.ts:1267-1283", "synchronises hip_stream once in the middle", "zs_last_host_chunks = 1",
                 '"sync_scan", "sync_size"', '"sync_pass", 1 .. 64, default 8', "67,108,863 candidates plus streams",
                 "multi-member gzip files", "a seek", "Not offered on the pool"):
        assert text in flat, text


def test_python_carries_the_keyword():
    import zsamd

    assert zsamd.decompress_scan("scan", [16]) is True
    assert zsamd.decompress_scan(None, None) is False and zsamd.decompress_scan([[]], [16]) is False
    with pytest.raises(ValueError):
        zsamd.decompress_scan("scan", None)  # the capacities must be given
    with pytest.raises(ValueError):
        zsamd.decompress_scan("scan", [16], zdict=b"d")
    assert callable(zsamd.Engine.last_restart_points) and not hasattr(zsamd.Pool, "last_restart_points")
    assert "headers" in inspect.signature(zsamd.Engine.decompress_device).parameters


def test_every_refusal_is_decided_before_the_context():
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
        for fn in (L.zs_inflate_batch_sync, L.zs_pool_inflate_batch_sync):
            r = fn(None, *host)
            got.append((r, L.zs_last_error().decode()))
        r = L.zs_inflate_batch_sync_device(None, wbits, n, None, u64(0, 32), u32(32, 32), None, out_off, out_cap, None, None,
                                           None, None, None, None, None)
        got.append((r, L.zs_last_error().decode()))
        return got

    # the format first, even of an empty batch and whatever else is wrong
    assert call(-16, 2, out_cap=None) == [(-2, "deflate64 has no restart points")] * 3
    assert call(-16, 0) == [(-2, "deflate64 has no restart points")] * 3
    assert call(14, 2, out_cap=None) == [(-2, "unsupported windowBits (use -15, 15 or 31)")] * 3
    assert call(0, 2) == [(-2, "unsupported windowBits (use -15, 15 or 31)")] * 3
    # the capacities must be given (there is no _auto form)
    assert call(31, 2, out_cap=None) == [(-2, "restart points are found with given capacities only")] * 3
    assert call(31, 2, out_off=u64(2, 16), out_cap=None) == [(-2, "restart points are found with given capacities only")] * 3
    # the device entry's alignment rule last; the host entries take any offset and capacity
    for kw in ({"out_off": u64(2, 16)}, {"out_cap": u32(18, 16)}):
        got = call(15, 2, **kw)
        assert got[2] == (-2, "output offsets/capacities must be multiples of 4")
        assert got[0] == (-2, "null context") and got[1] == (-2, "null pool")
    # nothing to refuse: then the context is looked at
    for wbits in (-15, 15, 31):
        assert call(wbits, 2) == [(-2, "null context"), (-2, "null pool"), (-2, "null context")]
    # no context, no record: the query answers 0
    assert L.zs_last_restart_points(None, None, None, None, 0) == 0


def test_the_sync_pass_options_range():
    """zs_set_option needs a context, so the range is checked where it is declared: the option's table entry
    and the pure predicate it calls (tests/test_plan_sync.py runs the predicate)"""
    capi = open(os.path.join(ROOT, "zlib-streams-ts_amd", "csrc", "capi.cpp")).read()
    assert re.search(r'OPT_INT\("sync_pass", o\.sync_pass, zs_sync_pass_ok\(v\), "sync_pass must be 1 \.\. 64"\)', capi)
    plan = open(os.path.join(ROOT, "zlib-streams-ts_amd", "csrc", "zs_plan.h")).read()
    assert re.search(r"zs_sync_pass_ok\(int v\) \{ return v >= 1 && v <= 64; \}", plan)
    assert re.search(r"uint32_t sync_pass = 8;", plan)
