"""CPU-side checks of the BGZF entries: libzsgpu.so exports them, include/zs_gpu.h declares them with exactly the
_members entries' arguments, every refusal is decided before the context is looked at and in the members' order,
zs_bgzf_out_len is host arithmetic that agrees with a walk of the headers in Python, and the Python binding carries
members="bgzf"."""
import ctypes
import inspect
import os
import re

import pytest

import bgzfcases as bc
import memberscases as mc
from memberscases import BGZF_EOF, member, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("zs_inflate_batch_bgzf_device", "zs_inflate_batch_members_device"), ("zs_inflate_batch_bgzf", "zs_inflate_batch_members"),
         ("zs_pool_inflate_batch_bgzf", "zs_pool_inflate_batch_members")]
GZIP_ONLY = "members are a gzip notion (use windowBits 31)"
CAPS = "members are found with given capacities only"
ALIGN = "output offsets/capacities must be multiples of 4"


def test_library_exports_the_symbols():
    import zsamd

    L = zsamd.lib()
    assert [s for s in [a for a, _ in PAIRS] + ["zs_last_bgzf_trusted", "zs_bgzf_out_len"] if not hasattr(L, s)] == []


def test_header_declares_them_with_the_members_entries_arguments():
    src = open(os.path.join(ROOT, "include", "zs_gpu.h")).read()

    def args(name):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        return " ".join(m.group(1).split())

    for new, old in PAIRS:
        assert args(new) == args(old), new
    assert "uint64_t zs_last_bgzf_trusted(zs_ctx *ctx);" in src
    assert "int zs_bgzf_out_len(const uint8_t *in, uint32_t in_len, uint64_t *total);" in src
    flat = " ".join(src.replace("*", " ").split())
    for t in ("FLG exactly 4", "p + total <= n", "<= 65536", '"incorrect length check"', '"bgzf_size"', "a BGZF writer",
              "a seek by virtual offset", "NOT verified"):
        assert t in flat, t


def test_every_refusal_is_decided_before_the_context_and_in_the_members_order():
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
        for fn in (L.zs_inflate_batch_bgzf, L.zs_pool_inflate_batch_bgzf):
            r = fn(None, *host)
            got.append((r, L.zs_last_error().decode()))
        r = L.zs_inflate_batch_bgzf_device(None, wbits, n, None, u64(0, 32), u32(32, 32), None, out_off, out_cap, None,
                                           None, None, None, None, None, None)
        got.append((r, L.zs_last_error().decode()))
        return got

    for wbits in (-15, 15, -16, 0, 30):
        assert call(wbits, 2, out_off=u64(2, 16), out_cap=None) == [(-2, GZIP_ONLY)] * 3, wbits
        assert call(wbits, 0) == [(-2, GZIP_ONLY)] * 3, wbits
    assert call(31, 2, out_cap=None) == [(-2, CAPS)] * 3
    assert call(31, 2, out_off=u64(2, 16), out_cap=None) == [(-2, CAPS)] * 3
    for kw in ({"out_off": u64(2, 16)}, {"out_cap": u32(18, 16)}):
        got = call(31, 2, **kw)
        assert got[2] == (-2, ALIGN)
        assert got[0] == (-2, "null context") and got[1] == (-2, "null pool")
    assert call(31, 2) == [(-2, "null context"), (-2, "null pool"), (-2, "null context")]
    assert L.zs_last_bgzf_trusted(None) == 0


def test_out_len_against_a_walk_of_the_headers():
    import zsamd

    L = zsamd.lib()

    def out_len(s):
        total = ctypes.c_uint64(77)
        r = L.zs_bgzf_out_len(s, len(s), ctypes.byref(total))
        assert zsamd.bgzf_out_len(s) == (total.value if r else None)
        return r, total.value

    a = bc.bgzf(text(300), 100)
    truthful = [a, bc.bgzf(text(70000, 3)), BGZF_EOF, a + b"\x00" * 37, a + b"\x1f\x8b\x08", bc.xy_block(text(50)) + a,
                bc.bgzf(text(90, 1), 30, eof=False)]
    for s in truthful:
        ok, total, idx = bc.chain(s)
        assert ok == 1 and idx == mc.walk(s)[0] and total == len(mc.walk(s)[1])
        assert out_len(s) == (1, total)
    mixed = bc.block(text(40)) + member(b"abc") + bc.block(text(30))
    cut = a[:-28][:-5]  # the last data block truncated: the magic holds, the size does not fit
    for s in (mixed, cut, member(b"abc"), mc.bgzf(text(300), block=100), b"", b"\x1f\x8b\x08\x04", a[:17]):
        assert bc.chain(s)[:2] == (0, 0)
        assert out_len(s) == (0, 0)
    # a header that lies is followed as it stands: host arithmetic, nothing is decoded
    lie = bc.block(text(40), isize=41) + BGZF_EOF
    assert out_len(lie) == (1, 41)
    assert L.zs_bgzf_out_len(None, 0, None) == 0


def test_python_carries_the_keyword():
    import zsamd

    assert zsamd.decompress_members("bgzf", "gzip", [16]) == "bgzf" and zsamd.decompress_members("bgzf", "gzip", None) == "bgzf"
    assert zsamd.decompress_members(True, "gzip", [16]) is True and zsamd.decompress_members(False, "gzip", None) is False
    for args in (("bgzf", "deflate", [16]), ("bgzf", "deflate-raw", None), ("BGZF", "gzip", [16]), ("scan", "gzip", [16])):
        with pytest.raises(ValueError):
            zsamd.decompress_members(*args)
    with pytest.raises(ValueError):
        zsamd.decompress_members("bgzf", "gzip", [16], zdict=b"d")
    with pytest.raises(ValueError):
        zsamd.decompress_members("bgzf", "gzip", [16], restart="scan")
    assert zsamd.bgzf_out_caps([bc.bgzf(text(301), 100), BGZF_EOF]) == [304, 0]
    with pytest.raises(ValueError, match="stream 1 is not BGZF throughout: give out_caps"):
        zsamd.bgzf_out_caps([BGZF_EOF, member(b"abc")])
    assert callable(zsamd.Engine.last_bgzf_trusted) and not hasattr(zsamd.Pool, "last_bgzf_trusted")
    assert "members" in inspect.signature(zsamd.Engine.decompress_device).parameters
