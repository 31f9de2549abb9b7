"""CPU-side checks of the Z_FULL_FLUSH entries: libzsgpu.so exports them, include/zs_gpu.h
declares them with the reference citation, the Python binding carries the keywords, the flush
argument is refused before the context is looked at (deflate.ts:720: Z_STREAM_ERROR), and
zs_deflate_bound_flush is zs_deflate_bound + 12 per flush point."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_deflate_batch_flush_device", "zs_deflate_batch_flush", "zs_pool_deflate_batch_flush"]


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_flush_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES + ["zs_deflate_bound_flush"] if not hasattr(L, s)] == []


def test_header_declares_them_with_the_reference_citation():
    src = header()
    for name in ENTRIES:
        m = re.search(r"/\*([^/]*?)\*/\s*int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        assert "deflate.ts:923-961" in m.group(1), name
        assert re.search(r"int level, int wbits, uint32_t n_streams,", m.group(2)), name
        args = " ".join(m.group(2).split())
        assert args.endswith("int flush, const uint64_t *flush_first, const uint32_t *flush_pos"), name
    assert re.search(r"#define ZS_FULL_FLUSH 3\b", src)
    assert re.search(r"uint64_t zs_deflate_bound_flush\(uint64_t source_len, int wbits, uint64_t n_flush\);", src)
    flat = " ".join(src.replace("*", " ").split())  # (comment line breaks aside)
    assert "no _dict, _strategy or _params forms" in flat
    for text in ('"flush mode not built"', '"invalid flush"', '"invalid flush positions"', '"null flush arrays"',
                 "level 0 with any flush point", "deflate.ts:923-961", "deflate.ts:720"):
        assert text in flat, text
    assert "take any inflate capacity" not in flat  # both host entries take exact capacities


def test_python_signatures():
    import zsamd

    for cls in (zsamd.Engine, zsamd.Pool):
        for meth in ("compress_batch", "compress_batch_raw", "compress_batch_detailed"):
            p = inspect.signature(getattr(cls, meth)).parameters
            assert p["flush_at"].default is None and p["flush_every"].default is None, (cls, meth)
    p = inspect.signature(zsamd.Engine.compress_device).parameters
    assert p["flush_at"].default is None and p["flush_every"].default is None
    assert inspect.signature(zsamd.deflate_bound).parameters["n_flush"].default == 0
    assert zsamd.Z_FULL_FLUSH == 3


def test_the_keywords_become_position_lists():
    import zsamd

    f = zsamd.compress_flush
    assert f([10, 20]) is None
    assert f([10, 20, 0, 8, 9], flush_every=8) == [[8], [8, 16], [], [], [8]]  # N, 2N, ... below the length
    assert f([10, 20], flush_at=[0, 5]) == [[0, 5], [0, 5]]                    # one list for all streams
    assert f([10, 20], flush_at=[[1], None]) == [[1], []]                      # one list per stream
    assert f([10, 20], flush_at=[]) == [[], []] and f([10, 20], flush_at=[[], (3, 4)]) == [[], [3, 4]]
    first, pos = zsamd._flush_arrays([[1], [], [3, 4]])
    assert list(first) == [0, 1, 1, 3] and list(pos)[:3] == [1, 3, 4]


def test_the_keywords_are_refused_with_the_other_features_before_any_call():
    import zsamd

    for kw in ({"zdict": b"dictionary"}, {"strategy": zsamd.Z_FIXED}, {"window_bits": 12}, {"mem_level": 4}):
        with pytest.raises(ValueError):
            zsamd.compress_flush([10], flush_at=[5], **kw)
        for cls in (zsamd.Engine, zsamd.Pool):  # the methods check before they touch the context (none here)
            with pytest.raises(ValueError):
                object.__new__(cls).compress_batch([b"0123456789"], "deflate", 6, flush_every=5, **kw)
    for kw in ({"flush_at": [5], "flush_every": 5}, {"flush_every": 0}, {"flush_every": -1}, {"flush_every": 2.0},
               {"flush_every": True}, {"flush_at": [[1], [2]]}, {"flush_at": [[1.5]]}, {"flush_at": [[-1]]},
               {"flush_at": [[1 << 32]]}):
        with pytest.raises(ValueError):
            zsamd.compress_flush([10], **kw)
    with pytest.raises(ValueError):
        zsamd.deflate_bound(100, "deflate", dict_len=4, n_flush=1)
    # the default parameters go with flush points
    assert zsamd.compress_flush([10], flush_at=[5], window_bits=15, mem_level=8, strategy=0) == [[5]]


def _args(n=1):
    off, ln, cap = (ctypes.c_uint64 * n)(0), (ctypes.c_uint32 * n)(1), (ctypes.c_uint32 * n)(64)
    st, ol, ck = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    first, pos = (ctypes.c_uint64 * (n + 1))(0, 1), (ctypes.c_uint32 * 1)(0)
    return off, ln, cap, st, ol, ck, ctypes.create_string_buffer(64), first, pos


@pytest.mark.parametrize("flush,msg", [(1, b"flush mode not built"), (2, b"flush mode not built"),
                                       (5, b"flush mode not built"), (0, b"invalid flush"), (4, b"invalid flush"),
                                       (6, b"invalid flush"), (-1, b"invalid flush")])
def test_the_c_entries_validate_the_flush_mode_first(flush, msg):
    import zsamd

    L = zsamd.lib()
    off, ln, cap, st, ol, ck, out, first, pos = _args()
    # (null context and pool, and an invalid level: the flush mode is refused before any of them is looked at)
    assert L.zs_deflate_batch_flush(None, 99, -15, 1, b"x", off, ln, out, off, cap, st, ol, ck, flush, first, pos) == -2
    assert L.zs_last_error() == msg
    assert L.zs_pool_deflate_batch_flush(None, 99, -15, 1, b"x", off, ln, out, off, cap, st, ol, ck, flush, first,
                                         pos) == -2
    assert L.zs_last_error() == msg
    assert L.zs_deflate_batch_flush_device(None, 99, -15, 1, None, off, ln, None, off, cap, None, None, None, None,
                                           flush, first, pos) == -2
    assert L.zs_last_error() == msg


def test_a_valid_flush_mode_without_a_context_is_still_an_error():
    import zsamd

    L = zsamd.lib()
    off, ln, cap, st, ol, ck, out, first, pos = _args()
    assert L.zs_deflate_batch_flush(None, 6, -15, 1, b"x", off, ln, out, off, cap, st, ol, ck, 3, first, pos) == -2
    assert L.zs_last_error() == b"null context"
    assert L.zs_deflate_batch_flush_device(None, 6, -15, 1, None, off, ln, None, off, cap, None, None, None, None, 3,
                                           first, pos) == -2
    assert L.zs_last_error() == b"null context"
    assert L.zs_pool_deflate_batch_flush(None, 6, -15, 1, b"x", off, ln, out, off, cap, st, ol, ck, 3, first, pos) == -2
    assert L.zs_last_error() == b"null pool"
    assert L.zs_pool_deflate_batch_flush(None, 6, -15, 1, b"x", off, ln, out, off, cap, st, ol, ck, 3, None, pos) == -2
    assert L.zs_last_error() == b"null flush arrays"


def test_the_bound_is_the_plain_bound_and_12_per_flush_point():
    import flushcases
    import zsamd

    L = zsamd.lib()
    for n in (0, 1, 100, 40000, 65536, 1 << 20, (1 << 32) - 1):
        for fmt, wbits in flushcases.WBITS.items():
            for k in (0, 1, 7, 4096, 1 << 20):
                assert L.zs_deflate_bound_flush(n, wbits, k) == L.zs_deflate_bound(n, wbits) + 12 * k
                assert L.zs_deflate_bound_flush(n, wbits, k) == flushcases.bound(n, fmt, k)
    assert zsamd.deflate_bound(1000, "gzip", n_flush=3) == zsamd.deflate_bound(1000, "gzip") + 36
    # every committed case stays within it; the closest one by how much
    g = flushcases.golden()
    room = [flushcases.bound(len(c[1]), c[3], len(c[4])) - g[c[0]][0] for c in flushcases.all_cases()]
    assert min(room) >= 0
