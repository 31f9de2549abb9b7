"""CPU-side checks of the dictionary-compression entries: libzsgpu.so exports them,
include/zs_gpu.h declares them and cites the reference, and zs_deflate_bound_dict
adds the four DICTID bytes of a zlib stream (deflate.ts:633)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_deflate_batch_dict_device", "zs_deflate_batch_dict", "zs_pool_deflate_batch_dict"]


def test_library_exports_the_dictionary_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES + ["zs_deflate_bound_dict"] if not hasattr(L, s)] == []


def test_header_declares_them_with_the_reference_citations():
    src = open(os.path.join(ROOT, "include", "zs_gpu.h")).read()
    for name in ENTRIES:
        m = re.search(r"/\*([^/]*?)\*/\s*int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        assert "deflate.ts:367-424" in m.group(1) and ":767-778" in m.group(1), name
        args = m.group(2)
        assert re.search(r"uint32_t \*(d_)?check,", args), name  # the _ex counterpart's arguments
        assert re.search(r"const uint8_t \*(d_)?dict,\s*const uint64_t \*dict_off,\s*const uint32_t \*dict_len$", args), name
    m = re.search(r"/\*([^/]*?)\*/\s*uint64_t zs_deflate_bound_dict\(uint64_t source_len, int wbits, uint64_t dict_len\);",
                  src, re.S)
    assert m and "deflate.ts:633" in m.group(1)


@pytest.mark.parametrize("n", [0, 1, 100, 65536, 1 << 30])
def test_bound(n):
    import zsamd

    L = zsamd.lib()
    for dl in (1, 257, 40000):
        assert L.zs_deflate_bound_dict(n, 15, dl) == L.zs_deflate_bound(n, 15) + 4
        assert L.zs_deflate_bound_dict(n, -15, dl) == L.zs_deflate_bound(n, -15)
    for wbits in (-15, 15, 31):
        assert L.zs_deflate_bound_dict(n, wbits, 0) == L.zs_deflate_bound(n, wbits)
    assert zsamd.deflate_bound(n, "deflate", 257) == zsamd.deflate_bound(n, "deflate") + 4
    assert zsamd.deflate_capacity(n, "deflate-raw", 257) == zsamd.deflate_capacity(n, "deflate-raw")
    assert zsamd.deflate_capacity(n, "deflate", 257) % 4 == 0
