"""CPU-side checks of the BGZF write entries: libzsgpu.so exports them, include/zs_gpu.h declares them and
states the bytes, the Python binding carries the keyword, the level, the block size, the arrays and the count are
refused before the context is looked at and in that order, and zs_deflate_bound_bgzf is the sum over the blocks."""
import ctypes
import inspect
import os
import re

import pytest

import bgzfwritecases as w

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_deflate_batch_bgzf_device", "zs_deflate_batch_bgzf", "zs_pool_deflate_batch_bgzf"]


def header():
    return open(os.path.join(ROOT, "include", "zs_gpu.h")).read()


def test_library_exports_the_bgzf_write_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES + ["zs_deflate_bound_bgzf", "zs_last_bgzf_blocks"] if not hasattr(L, s)] == []


def test_header_declares_them_and_states_the_bytes():
    src = header()
    for name in ENTRIES:
        m = re.search(r"int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        args = " ".join(m.group(1).split())
        assert re.search(r"int level, uint32_t n_streams,", args), name  # no wbits
        assert args.endswith("uint32_t block_bytes"), name
    assert re.search(r"#define ZS_BGZF_BLOCK 65280\b", src)
    assert re.search(r"uint64_t zs_deflate_bound_bgzf\(uint64_t source_len, uint32_t block_bytes\);", src)
    assert re.search(r"uint64_t zs_last_bgzf_blocks\(zs_ctx \*ctx, uint64_t \*block_first, uint32_t \*block_in, "
                     r"uint32_t \*block_out,\s+uint64_t cap\);", src)
    flat = " ".join(src.replace("*", " ").split())  # (comment line breaks aside)
    for text in ("SAM specification 4.1", "1f 8b 08 04 | 00 00 00 00 | 00 | ff | 06 00 | 42 43 02 00 | BSIZE",
                 "1f8b08040000000000ff0600424302001b0003000000000000000000", "XFL 0 at every level",
                 "01 | LEN | ~LEN | the piece", '"invalid BGZF block size"', '"null arrays"',
                 '"too many BGZF blocks (streams + blocks above 65,535 in one call)"',
                 "zs_deflate_bound(65280, -15) + 26 = 65,331 <= 65,536", "no _dict, _strategy or _params forms",
                 "keeps its trailing empty static block", "bgzip built against zlib 1.2.11",
                 "the contract is the bytes above"):
        assert text in flat, text


def test_python_signatures():
    import zsamd

    for cls in (zsamd.Engine, zsamd.Pool):
        for meth in ("compress_batch", "compress_batch_raw", "compress_batch_detailed"):
            assert inspect.signature(getattr(cls, meth)).parameters["bgzf"].default is None, (cls, meth)
    for meth in ("compress_device", "compress_host"):
        assert inspect.signature(getattr(zsamd.Engine, meth)).parameters["bgzf"].default is None, meth
    assert inspect.signature(zsamd.deflate_bound).parameters["bgzf"].default is None
    assert hasattr(zsamd.Engine, "last_bgzf_blocks") and zsamd.BGZF_BLOCK == 65280


def test_the_keyword_becomes_the_block_size():
    import zsamd

    f = zsamd.compress_bgzf
    assert f(None) is None and f(False) is None
    assert f(True) == 0 and f(65280) == 65280 and f(1) == 1 and f(7, "gzip", window_bits=15, mem_level=8) == 7
    assert f(65281) == 65281  # (the engine refuses it: "invalid BGZF block size")
    for bad in (0, -1, 2.0, "64k", 1 << 32):
        with pytest.raises(ValueError):
            f(bad)


def test_the_keyword_is_refused_with_the_other_features_before_any_call():
    import zsamd

    for fmt in ("deflate-raw", "deflate"):
        with pytest.raises(ValueError):
            zsamd.compress_bgzf(True, fmt)
    for kw in ({"zdict": b"dictionary"}, {"strategy": zsamd.Z_FIXED}, {"window_bits": 12}, {"mem_level": 4},
               {"flush_at": [5]}, {"flush_every": 5}):
        with pytest.raises(ValueError):
            zsamd.compress_bgzf(True, "gzip", **kw)
        for cls in (zsamd.Engine, zsamd.Pool):  # the methods check before they touch the context (none here)
            with pytest.raises(ValueError):
                object.__new__(cls).compress_batch([b"0123456789"], "gzip", 6, bgzf=True, **kw)
    with pytest.raises(ValueError):
        object.__new__(zsamd.Engine).compress_batch([b"0123456789"], "deflate", 6, bgzf=True)
    for kw in ({"dict_len": 4}, {"n_flush": 1}):
        with pytest.raises(ValueError):
            zsamd.deflate_bound(100, "gzip", bgzf=True, **kw)
    with pytest.raises(ValueError):
        zsamd.deflate_bound(100, "deflate", bgzf=True)
    with pytest.raises(ValueError):
        zsamd.deflate_bound(100, "gzip", bgzf=65281)


def _args(n=1, length=1):
    off, ln, cap = (ctypes.c_uint64 * n)(0), (ctypes.c_uint32 * n)(length), (ctypes.c_uint32 * n)(64)
    st, ol, ck = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    return off, ln, cap, st, ol, ck, ctypes.create_string_buffer(64)


def calls(level, block, n=1, length=1, null=False):
    """the three entries with a null context / pool: [(return code, zs_last_error())]"""
    import zsamd

    L = zsamd.lib()
    off, ln, cap, st, ol, ck, out = _args(max(n, 1), length)
    a_off, a_ln, a_cap = (None, None, None) if null else (off, ln, cap)
    res = []
    r = L.zs_deflate_batch_bgzf_device(None, level, n, None, a_off, a_ln, None, a_off, a_cap, None, None, None, None, block)
    res.append((r, L.zs_last_error()))
    r = L.zs_deflate_batch_bgzf(None, level, n, b"x", a_off, a_ln, out, a_off, a_cap, st, ol, ck, block)
    res.append((r, L.zs_last_error()))
    r = L.zs_pool_deflate_batch_bgzf(None, level, n, b"x", a_off, a_ln, out, a_off, a_cap, st, ol, ck, block)
    res.append((r, L.zs_last_error()))
    return res


def test_the_c_entries_refuse_in_order_before_the_context_is_looked_at():
    # the level first, whatever else is wrong (a block size out of range, null arrays, a null context)
    for level in (-2, 10, 99):
        assert calls(level, 65281, null=True) == [(-2, b"invalid level")] * 3
    # then the block size
    for block in (65281, 1 << 20, 0xffffffff):
        assert calls(6, block, null=True) == [(-2, b"invalid BGZF block size")] * 3
    # then the arrays
    for level in (-1, 0, 9):
        assert calls(level, 0, null=True) == [(-2, b"null arrays")] * 3
    # then, for the one device call, streams + data blocks: 1 + 65,535 refused, 1 + 65,534 taken (up to the context)
    many = b"too many BGZF blocks (streams + blocks above 65,535 in one call)"
    assert calls(6, 1, length=65535)[0] == (-2, many)
    assert calls(6, 7, length=7 * 65534 + 1)[0] == (-2, many)
    assert calls(6, 1, length=65534)[0] == (-2, b"null context")
    assert calls(6, 7, length=7 * 65534)[0] == (-2, b"null context")


def test_a_valid_call_without_a_context_is_still_an_error():
    for level, block in ((-1, 0), (0, 1), (9, 65280)):
        assert calls(level, block) == [(-2, b"null context"), (-2, b"null context"), (-2, b"null pool")]


def test_last_bgzf_blocks_without_a_context_is_empty():
    import zsamd

    assert zsamd.lib().zs_last_bgzf_blocks(None, None, None, None, 0) == 0


def test_the_bound_is_the_sum_over_the_blocks():
    import zsamd

    L = zsamd.lib()
    for block in (0, 1, 7, 256, 4096, 65279, 65280):
        bb = block or 65280
        for n in (0, 1, bb - 1, bb, bb + 1, 2 * bb + 1, 1000003):
            if n // bb > 300000:
                continue
            want = sum(L.zs_deflate_bound(min(bb, n - a), -15) + 26 for a in range(0, n, bb)) + 28
            assert L.zs_deflate_bound_bgzf(n, block) == want == w.bound(n, bb), (n, block)
    assert L.zs_deflate_bound_bgzf(65280, 0) == 65331 + 28 and L.zs_deflate_bound_bgzf(0, 0) == 28
    assert L.zs_deflate_bound_bgzf(1 << 32, 0) == w.bound(1 << 32)  # (closed form: no loop over the blocks)
    assert L.zs_deflate_bound_bgzf(100, 65281) == 0
    assert zsamd.deflate_bound(1000, "gzip", bgzf=True) == w.bound(1000)
    assert zsamd.deflate_bound(1000, "gzip", bgzf=7) == w.bound(1000, 7)
    # every committed case stays within it
    g = w.golden()
    assert min(w.bound(len(c[1]), c[3]) - g[c[0]][0] for c in w.all_cases()) >= 0
    # level 0's stored form is smaller than the bound at every length
    for n in (1, 7, 4095, 4096, 65280):
        assert n + 5 + 26 + 28 <= w.bound(n)
