"""CPU-side checks of the compression-strategy entries: libzsgpu.so exports them,
include/zs_gpu.h declares them with the constants and the reference citations, the
Python binding carries the constants, and the argument checks that need no GPU answer
as deflateInit2_ does (deflate.ts:289-290: Z_STREAM_ERROR, "init failed: -2")."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_deflate_batch_strategy_device", "zs_deflate_batch_strategy", "zs_pool_deflate_batch_strategy"]
CONSTANTS = {"ZS_DEFAULT_STRATEGY": 0, "ZS_FILTERED": 1, "ZS_HUFFMAN_ONLY": 2, "ZS_RLE": 3, "ZS_FIXED": 4}


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_strategy_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES if not hasattr(L, s)] == []


def test_header_declares_them_with_the_reference_citations():
    src = header()
    for name in ENTRIES:
        m = re.search(r"/\*([^/]*?)\*/\s*int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        assert "deflate.ts:289-290" in m.group(1) and ":923-931" in m.group(1), name
        assert re.search(r"int level, int strategy, int wbits, uint32_t n_streams,", m.group(2)), name
        assert re.search(r"uint32_t \*(d_)?check(, void \*hip_stream)?$", m.group(2)), name  # the counterpart's arguments
    for name, value in CONSTANTS.items():
        m = re.search(r"#define %s (\d+)\s*/\*(.*?)\*/" % name, src, re.S)
        assert m and int(m.group(1)) == value, name
        assert re.search(r"(deflate|trees)\.ts:\d+", m.group(2)), name
    assert "no _dict forms" in src and '"rle_ref"' in src


def test_python_constants():
    import zsamd

    assert (zsamd.Z_DEFAULT_STRATEGY, zsamd.Z_FILTERED, zsamd.Z_HUFFMAN_ONLY, zsamd.Z_RLE, zsamd.Z_FIXED) == (0, 1, 2, 3, 4)
    for cls in (zsamd.Engine, zsamd.Pool):
        for meth in ("compress_batch", "compress_batch_raw", "compress_batch_detailed"):
            assert inspect.signature(getattr(cls, meth)).parameters["strategy"].default == 0, (cls, meth)
    for meth in ("compress_device", "compress_host"):
        assert inspect.signature(getattr(zsamd.Engine, meth)).parameters["strategy"].default == 0, meth


@pytest.mark.parametrize("bad", [-1, 5, 100, 2.0, "2", None, True])
def test_an_invalid_strategy_is_init_failed_minus_2(bad):
    import zsamd

    with pytest.raises(zsamd.ZsError) as e:
        zsamd.compress_strategy(bad)
    assert str(e.value) == "init failed: -2" and e.value.status == zsamd.Z_STREAM_ERROR
    assert e.value.phase == zsamd.PHASE_INIT


def test_a_strategy_with_a_dictionary_is_refused_before_any_call():
    import zsamd

    for s in (1, 2, 3, 4):
        with pytest.raises(ValueError):
            zsamd.compress_strategy(s, b"dictionary")
    assert zsamd.compress_strategy(0, b"dictionary") == 0
    assert [zsamd.compress_strategy(s) for s in range(5)] == [0, 1, 2, 3, 4]
    # the methods check before they touch the context (none here)
    eng = object.__new__(zsamd.Engine)
    with pytest.raises(ValueError):
        eng.compress_batch([b"x"], "deflate", 6, zdict=b"d", strategy=zsamd.Z_RLE)
    with pytest.raises(zsamd.ZsError, match="init failed: -2"):
        eng.compress_batch([b"x"], "deflate", 6, strategy=9)


@pytest.mark.parametrize("strategy", [-1, 5, 1 << 20])
def test_the_c_entries_validate_the_strategy_first(strategy):
    import zsamd

    L = zsamd.lib()
    n = 1
    off, ln, cap = (ctypes.c_uint64 * n)(0), (ctypes.c_uint32 * n)(1), (ctypes.c_uint32 * n)(64)
    st, ol, ck = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    out = ctypes.create_string_buffer(64)
    # (null context and pool: the strategy is refused before either is looked at)
    assert L.zs_deflate_batch_strategy(None, 6, strategy, -15, n, b"x", off, ln, out, off, cap, st, ol, ck) == -2
    assert L.zs_last_error() == b"invalid strategy"
    assert L.zs_pool_deflate_batch_strategy(None, 6, strategy, -15, n, b"x", off, ln, out, off, cap, st, ol, ck) == -2
    assert L.zs_last_error() == b"invalid strategy"
    assert L.zs_deflate_batch_strategy_device(None, 6, strategy, -15, n, None, off, ln, None, off, cap, None, None, None,
                                              None) == -2
    assert L.zs_last_error() == b"invalid strategy"


def test_a_valid_strategy_without_a_context_is_still_an_error():
    import zsamd

    L = zsamd.lib()
    n = 1
    off, ln, cap = (ctypes.c_uint64 * n)(0), (ctypes.c_uint32 * n)(1), (ctypes.c_uint32 * n)(64)
    st, ol, ck = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    out = ctypes.create_string_buffer(64)
    assert L.zs_deflate_batch_strategy(None, 6, 2, -15, n, b"x", off, ln, out, off, cap, st, ol, ck) == -2
    assert L.zs_last_error() == b"null context"
