"""CPU-side checks of the primed-pieces entries: libzsgpu.so exports them, include/zs_gpu.h
declares them (the _flush entries' arguments without `int flush`) and says what sizes their
outputs, the Python binding carries the keyword and refuses it up front where it is not built,
and what the entries answer before a context is looked at.  The refusals that need a context
(positions, level 0, the count, windowBits, level) are in test_gpu_deflate_primed.py; their order
is zs_plan.h's, pinned in test_plan_primed.py."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_deflate_batch_primed_device", "zs_deflate_batch_primed", "zs_pool_deflate_batch_primed"]


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_primed_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES if not hasattr(L, s)] == []


def test_header_declares_them_as_the_flush_entries_without_the_flush_argument():
    src = header()
    for name in ENTRIES:
        m = re.search(r"int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        args = " ".join(m.group(1).split())
        flush = " ".join(re.search(r"int %s\(([^;]*)\);" % name.replace("primed", "flush"), src, re.S).group(1).split())
        assert args == flush.replace("int flush, ", ""), name
        assert args.endswith("const uint64_t *flush_first, const uint32_t *flush_pos") and "int flush" not in args, name
    flat = " ".join(src.replace("*", " ").split())  # (comment line breaks aside)
    for text in ("pigz's construction", "no FDICT", "deflateSetDictionary(in[max(0, a - 32768), a))", "Z_SYNC_FLUSH",
                 "size outputs with zs_deflate_bound_flush", "a raw piece with a dictionary adds no bytes",
                 "a call whose streams have no point is the _ex call", "zs_last_flush_index returns the offsets behind the markers",
                 "level 0 with a point", "streams + points above 65,535"):
        assert text in flat, text
    assert "pigz-identical" not in flat and "identical to pigz" not in flat


def test_python_signatures():
    import zsamd

    for cls in (zsamd.Engine, zsamd.Pool):
        for meth in ("compress_batch", "compress_batch_raw", "compress_batch_detailed"):
            assert inspect.signature(getattr(cls, meth)).parameters["primed"].default is False, (cls, meth)
    assert inspect.signature(zsamd.Engine.compress_device).parameters["primed"].default is False


def test_primed_needs_positions_and_is_refused_with_the_other_features_before_any_call():
    import zsamd

    f = zsamd.compress_primed
    assert f(False) is False and f(None) is False and f(False, flush_every=5) is False
    assert f(True, flush_at=[5]) is True and f(True, flush_every=5) is True and f(True, flush_at=[]) is True
    with pytest.raises(ValueError):
        f(True)  # no positions
    with pytest.raises(ValueError):
        f(True, flush_every=5, bgzf=True)
    one = [b"0123456789"]
    for cls in (zsamd.Engine, zsamd.Pool):  # the methods check before they touch the context (none here)
        for meth in ("compress_batch", "compress_batch_raw", "compress_batch_detailed"):
            with pytest.raises(ValueError):
                getattr(object.__new__(cls), meth)(one, "deflate", 6, primed=True)
            with pytest.raises(ValueError):
                getattr(object.__new__(cls), meth)(one, "gzip", 6, primed=True, flush_every=5, bgzf=True)
            for kw in ({"zdict": b"dictionary"}, {"strategy": zsamd.Z_FIXED}, {"window_bits": 12}, {"mem_level": 4}):
                with pytest.raises(ValueError):
                    getattr(object.__new__(cls), meth)(one, "deflate", 6, primed=True, flush_every=5, **kw)
    ln, off = (ctypes.c_uint32 * 1)(10), (ctypes.c_uint64 * 1)(0)
    with pytest.raises(ValueError):
        object.__new__(zsamd.Engine).compress_device(6, "deflate", 1, 0, off, ln, 0, off, ln, 0, 0, primed=True)
    with pytest.raises(ValueError):
        object.__new__(zsamd.Engine).compress_device(6, "deflate", 1, 0, off, ln, 0, off, ln, 0, 0, primed=True,
                                                     flush_at=[5], window_bits=12)


def _args(n=1):
    off, ln, cap = (ctypes.c_uint64 * n)(0), (ctypes.c_uint32 * n)(1), (ctypes.c_uint32 * n)(64)
    st, ol, ck = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    first, pos = (ctypes.c_uint64 * (n + 1))(0, 1), (ctypes.c_uint32 * 1)(0)
    return off, ln, cap, st, ol, ck, ctypes.create_string_buffer(64), first, pos


def test_what_the_entries_answer_before_a_context_is_looked_at():
    """no `flush` argument, so nothing of the request is refused before the context: a null context or pool is
    named first, whatever else is wrong; the pool names null arrays before it looks at itself, as the _flush form"""
    import zsamd

    L = zsamd.lib()
    off, ln, cap, st, ol, ck, out, first, pos = _args()
    for level, wbits in ((6, -15), (99, 7), (0, 31)):
        assert L.zs_deflate_batch_primed(None, level, wbits, 1, b"x", off, ln, out, off, cap, st, ol, ck, first, pos) == -2
        assert L.zs_last_error() == b"null context"
        assert L.zs_deflate_batch_primed_device(None, level, wbits, 1, None, off, ln, None, off, cap, None, None, None,
                                                None, first, pos) == -2
        assert L.zs_last_error() == b"null context"
        assert L.zs_pool_deflate_batch_primed(None, level, wbits, 1, b"x", off, ln, out, off, cap, st, ol, ck, first,
                                              pos) == -2
        assert L.zs_last_error() == b"null pool"
        assert L.zs_pool_deflate_batch_primed(None, level, wbits, 1, b"x", off, ln, out, off, cap, st, ol, ck, None,
                                              pos) == -2
        assert L.zs_last_error() == b"null flush arrays"
    # an empty batch through the pool form needs no arrays
    assert L.zs_pool_deflate_batch_primed(None, 6, -15, 0, b"", off, ln, out, off, cap, st, ol, ck, None, None) == -2
    assert L.zs_last_error() == b"null pool"


def test_every_committed_case_stays_within_the_flush_bound():
    import primedcases
    import zsamd

    L = zsamd.lib()
    g = primedcases.golden()
    for name, data, level, fmt, pos in primedcases.all_cases():
        b = L.zs_deflate_bound_flush(len(data), primedcases.WBITS[fmt], len(pos))
        assert b == primedcases.bound(len(data), fmt, len(pos)) and g[name][0] <= b, name
