"""CPU-side checks of the windowBits / memLevel entries: libzsgpu.so exports them,
include/zs_gpu.h declares them with the reference citation, the Python binding carries the
keywords and the validator, the argument checks that need no GPU answer as deflateInit2_
does (deflate.ts:281-294: Z_STREAM_ERROR, "init failed: -2"), and zs_deflate_bound_params
is deflateBound (deflate.ts:619-673)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_deflate_batch_params_device", "zs_deflate_batch_params", "zs_pool_deflate_batch_params"]


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_params_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES + ["zs_deflate_bound_params"] if not hasattr(L, s)] == []


def test_header_declares_them_with_the_reference_citation():
    src = header()
    for name in ENTRIES:
        m = re.search(r"/\*([^/]*?)\*/\s*int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        assert "deflate.ts:253-343" in m.group(1), name
        assert re.search(r"int level, int wbits, int mem_level, uint32_t n_streams,", m.group(2)), name
        assert re.search(r"uint32_t \*(d_)?check(, void \*hip_stream)?$", m.group(2)), name  # the counterpart's arguments
    m = re.search(r"/\*((?:[^*]|\*(?!/))*)\*/\s*uint64_t zs_deflate_bound_params\(uint64_t source_len, int wbits, "
                  r"int mem_level, int level\);", src, re.S)
    assert m and "deflate.ts:619-673" in m.group(1)
    flat = " ".join(src.replace("*", " ").split())  # (comment line breaks aside)
    assert "no _dict or _strategy forms" in flat
    assert '"invalid window bits"' in flat and '"invalid memLevel"' in flat


def test_python_signatures():
    import zsamd

    for cls in (zsamd.Engine, zsamd.Pool):
        for meth in ("compress_batch", "compress_batch_raw", "compress_batch_detailed"):
            p = inspect.signature(getattr(cls, meth)).parameters
            assert p["window_bits"].default is None and p["mem_level"].default == 8, (cls, meth)
    for meth in ("compress_device", "compress_host"):
        p = inspect.signature(getattr(zsamd.Engine, meth)).parameters
        assert p["window_bits"].default is None and p["mem_level"].default == 8, meth


def test_the_validator_returns_the_windowbits_code():
    import zsamd

    assert zsamd.compress_params("deflate-raw", None, 8) == -15
    assert zsamd.compress_params("deflate", None, 8) == 15 and zsamd.compress_params("gzip", None, 8) == 31
    assert [zsamd.compress_params("deflate", wb, 1) for wb in range(8, 16)] == list(range(8, 16))
    assert [zsamd.compress_params("deflate-raw", wb, 9) for wb in range(9, 16)] == [-wb for wb in range(9, 16)]
    assert [zsamd.compress_params("gzip", wb, 4) for wb in range(9, 16)] == [wb + 16 for wb in range(9, 16)]
    # the default parameters go with a dictionary or a strategy as before
    assert zsamd.compress_params("deflate", 15, 8, zdict=b"d") == 15 and zsamd.compress_params("gzip", None, 8, strategy=2) == 31


@pytest.mark.parametrize("fmt,wb,ml", [("deflate", 7, 8), ("deflate", 16, 8), ("deflate-raw", 8, 8), ("gzip", 8, 8),
                                       ("deflate", 12.0, 8), ("deflate", "12", 8), ("deflate", True, 8),
                                       ("deflate", 12, 0), ("deflate", 12, 10), ("deflate", 12, 8.0),
                                       ("deflate", 12, None), ("deflate", 12, True), ("deflate", -12, 8)])
def test_invalid_parameters_are_init_failed_minus_2(fmt, wb, ml):
    import zsamd

    with pytest.raises(zsamd.ZsError) as e:
        zsamd.compress_params(fmt, wb, ml)
    assert str(e.value) == "init failed: -2" and e.value.status == zsamd.Z_STREAM_ERROR
    assert e.value.phase == zsamd.PHASE_INIT
    # the methods check before they touch the context (none here)
    with pytest.raises(zsamd.ZsError, match="init failed: -2"):
        object.__new__(zsamd.Engine).compress_batch([b"x"], fmt, 6, window_bits=wb, mem_level=ml)
    with pytest.raises(zsamd.ZsError, match="init failed: -2"):
        object.__new__(zsamd.Pool).compress_batch([b"x"], fmt, 6, window_bits=wb, mem_level=ml)


def test_non_default_parameters_with_a_dictionary_or_a_strategy_are_refused_before_any_call():
    import zsamd

    for wb, ml in ((12, 8), (None, 4), (15, 9), (8, 8)):
        with pytest.raises(ValueError):
            zsamd.compress_params("deflate", wb, ml, zdict=b"dictionary")
        with pytest.raises(ValueError):
            zsamd.compress_params("deflate", wb, ml, strategy=zsamd.Z_FIXED)
        eng = object.__new__(zsamd.Engine)
        with pytest.raises(ValueError):
            eng.compress_batch([b"x"], "deflate", 6, zdict=b"d", window_bits=wb, mem_level=ml)
        with pytest.raises(ValueError):
            eng.compress_batch([b"x"], "deflate", 6, strategy=zsamd.Z_RLE, window_bits=wb, mem_level=ml)


def _args(n=1):
    off, ln, cap = (ctypes.c_uint64 * n)(0), (ctypes.c_uint32 * n)(1), (ctypes.c_uint32 * n)(64)
    st, ol, ck = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    return off, ln, cap, st, ol, ck, ctypes.create_string_buffer(64)


@pytest.mark.parametrize("wbits,ml,msg", [(-8, 8, b"invalid window bits"), (24, 8, b"invalid window bits"),
                                          (7, 8, b"invalid window bits"), (16, 8, b"invalid window bits"),
                                          (32, 8, b"invalid window bits"), (12, 0, b"invalid memLevel"),
                                          (12, 10, b"invalid memLevel")])
def test_the_c_entries_validate_the_parameters_first(wbits, ml, msg):
    import zsamd

    L = zsamd.lib()
    off, ln, cap, st, ol, ck, out = _args()
    # (null context and pool: the parameters are refused before either is looked at)
    assert L.zs_deflate_batch_params(None, 6, wbits, ml, 1, b"x", off, ln, out, off, cap, st, ol, ck) == -2
    assert L.zs_last_error() == msg
    assert L.zs_pool_deflate_batch_params(None, 6, wbits, ml, 1, b"x", off, ln, out, off, cap, st, ol, ck) == -2
    assert L.zs_last_error() == msg
    assert L.zs_deflate_batch_params_device(None, 6, wbits, ml, 1, None, off, ln, None, off, cap, None, None, None,
                                            None) == -2
    assert L.zs_last_error() == msg


@pytest.mark.parametrize("wbits,ml", [(-9, 1), (8, 8), (12, 4), (31, 9), (15, 8)])
def test_valid_parameters_without_a_context_are_still_an_error(wbits, ml):
    import zsamd

    L = zsamd.lib()
    off, ln, cap, st, ol, ck, out = _args()
    assert L.zs_deflate_batch_params(None, 6, wbits, ml, 1, b"x", off, ln, out, off, cap, st, ol, ck) == -2
    assert L.zs_last_error() == b"null context"
    assert L.zs_deflate_batch_params_device(None, 6, wbits, ml, 1, None, off, ln, None, off, cap, None, None, None,
                                            None) == -2
    assert L.zs_last_error() == b"null context"
    assert L.zs_pool_deflate_batch_params(None, 6, wbits, ml, 1, b"x", off, ln, out, off, cap, st, ol, ck) == -2
    assert L.zs_last_error() == b"null pool"


def test_the_bound_is_deflateBound():
    import zsamd

    L = zsamd.lib()
    wrap = {"deflate-raw": 0, "deflate": 6, "gzip": 18}
    code = lambda fmt, wb: -wb if fmt == "deflate-raw" else wb + 16 if fmt == "gzip" else wb
    for n in (0, 1, 100, 40000, 65536, 1 << 20, (1 << 32) - 1):
        fixedlen = n + (n >> 3) + (n >> 8) + (n >> 9) + 4
        storelen = n + (n >> 5) + (n >> 7) + (n >> 11) + 7
        for fmt in wrap:
            for wb in range(8 if fmt == "deflate" else 9, 16):
                for ml in range(1, 10):
                    for level in (0, 1, 6, 9):
                        got = L.zs_deflate_bound_params(n, code(fmt, wb), ml, level)
                        if (max(wb, 9), ml + 7) == (15, 15):  # the default branch is zs_deflate_bound
                            assert got == L.zs_deflate_bound(n, code(fmt, 15)), (n, fmt, wb, ml, level)
                        else:  # deflate.ts:669-671
                            want = (fixedlen if max(wb, 9) <= ml + 7 and level else storelen) + wrap[fmt]
                            assert got == want, (n, fmt, wb, ml, level)
    assert L.zs_deflate_bound_params(40000, -9, 1, 6) == 41588
    assert L.zs_deflate_bound_params(100, -8, 8, 6) == 0 and L.zs_deflate_bound_params(100, 12, 10, 6) == 0
