"""The goldens of the dictionary-compression tests (tests/golden/deflate_dict.json):
one entry per case of tests/deflatedictcases.py, and -- where the running zlib is
the 1.2.11 they were written with -- regenerating them reproduces the file."""
import importlib.util
import os
import zlib

import pytest

import deflatedictcases as cases
import dictcases

HERE = os.path.dirname(os.path.abspath(__file__))


def generator():
    spec = importlib.util.spec_from_file_location("gen_deflate_dict", os.path.join(HERE, "golden", "gen_deflate_dict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_case_has_a_golden():
    names = [c[0] for c in cases.all_cases()]
    assert len(names) == len(set(names))
    g = cases.golden()
    assert sorted(names) == sorted(g)
    assert all(isinstance(v, list) and len(v) == 2 and len(v[1]) == 16 for v in g.values())


def test_case_list_covers_the_issue():
    names = {c[0] for c in cases.all_cases()}
    assert len(cases.small_inputs()) == 20 and [len(x) for x in cases.small_inputs()[16:]] == [0, 1, 2, 3]
    for L in dictcases.DICT_LENS:
        for level in range(1, 10):
            for fmt in ("deflate-raw", "deflate"):
                assert "s1/%s/l%d/d%d/i19" % (fmt, level, L) in names
    for level in (1, 3, 4, 6, 9):
        for L in (32768, 32767, 257):
            for n in (32506, 32507, 32606, 32767, 32768, 32769, 32770, 65536, 98604):
                assert "s2/l%d/d%d/text%d" % (level, L, n) in names
            for k in ("mixed200001", "zeros70000", "rand40000", "rand32767"):
                assert "s2/l%d/d%d/%s" % (level, L, k) in names
        for k in ("a3", "nil32768", "nil32767"):
            assert "s2/l%d/split/%s" % (level, k) in names
    (_, d, x), (_, d1, x1), (_, d2, x2) = cases.split_inputs()
    assert len(d) == 32768 and len(d + x) == 65536 and (d + x)[40000:40020] == (d + x)[7494:7514]
    assert len(d1 + x1) == 65374 and x1[65274 - 32768:65294 - 32768] == x1[:20]
    assert len(d2) == 32767 and d1[1:] == d2 and x1 == x2


def test_zlib_facts_the_design_rests_on():
    """(any zlib) the window keeps a dictionary's last 32,768 bytes, DICTID covers all of it"""
    d, x = dictcases.dictionary(40000), dictcases.record(3)
    assert dictcases.compress(x, 6, "deflate-raw", d) == dictcases.compress(x, 6, "deflate-raw", d[-32768:])
    z = dictcases.compress(x, 6, "deflate", d)
    assert z[:2] == b"\x78\xbb" and z[2:6] == zlib.adler32(d).to_bytes(4, "big")
    assert z != dictcases.compress(x, 6, "deflate", d[-32768:])
    assert z[-4:] == zlib.adler32(x).to_bytes(4, "big")
    with pytest.raises(ValueError):
        zlib.compressobj(6, zlib.DEFLATED, 31, 8, 0, d)


def test_regenerating_reproduces_the_file():
    gen = generator()
    if zlib.ZLIB_RUNTIME_VERSION != gen.WANT_ZLIB:
        pytest.skip("zlib %s is running; the goldens are zlib %s's" % (zlib.ZLIB_RUNTIME_VERSION, gen.WANT_ZLIB))
    assert gen.generate() == cases.golden()
