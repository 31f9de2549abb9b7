"""CPU-side checks of the preset-dictionary entries: libzsgpu.so exports them,
include/zs_gpu.h declares them and cites the reference, and the Python binding
lays dictionaries out as the ABI takes them."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zs_inflate_batch_dict_device", "zs_inflate_batch_dict", "zs_inflate_batch_dict_auto",
           "zs_pool_inflate_batch_dict", "zs_pool_inflate_batch_dict_auto"]


def test_library_exports_the_dictionary_entries():
    import zsamd

    L = zsamd.lib()
    assert [s for s in ENTRIES if not hasattr(L, s)] == []


def test_header_declares_them_with_the_reference_citations():
    src = open(os.path.join(ROOT, "include", "zs_gpu.h")).read()
    for name in ENTRIES:
        m = re.search(r"/\*([^/]*?)\*/\s*int %s\(([^;]*)\);" % name, src, re.S)
        assert m, name
        assert "inflate.ts:1220-1249" in m.group(1) and ":594-597" in m.group(1), name
        args = m.group(2)
        assert re.search(r"const uint8_t \*(d_)?dict,\s*const uint64_t \*dict_off,\s*const uint32_t \*dict_len$", args), name


def test_binding_lays_dictionaries_out_once_each():
    import zsamd

    a, b = b"x" * 10, b"yz" * 7
    blob, offs, lens = zsamd._dict_layout([a, None, b, bytes(a), b"", b], 6)
    assert blob == a + b
    assert list(offs)[:6] == [0, 0, 10, 0, 0, 10] and list(lens)[:6] == [10, 0, 14, 10, 0, 14]
    blob, offs, lens = zsamd._dict_layout(a, 3)
    assert blob == a and list(offs)[:3] == [0, 0, 0] and list(lens)[:3] == [10, 10, 10]
    with pytest.raises(ValueError):
        zsamd._dict_layout([a], 2)
