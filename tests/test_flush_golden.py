"""CPU: tests/golden/deflate_flush.json is what C zlib 1.2.11 produces for the cases of
tests/flushcases.py (gen_deflate_flush.py --check); every yardstick output inflates back to its
input, equals the concatenation of its independently compressed pieces -- the property the
engine's segments rest on -- and stays within zs_deflate_bound_flush.  Skips when the runtime
zlib is another version: the goldens are 1.2.11's."""
import os
import subprocess
import sys
import zlib

import pytest

import flushcases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(zlib.ZLIB_RUNTIME_VERSION != "1.2.11", reason="the goldens are zlib 1.2.11's")


def test_goldens_are_zlib_1_2_11():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_deflate_flush.py"), "--check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases match" % len(cases.all_cases()) in r.stdout


def test_every_case_has_a_golden_and_the_names_are_unique():
    names = [c[0] for c in cases.all_cases()]
    assert len(set(names)) == len(names) and set(names) == set(cases.golden())


def test_every_yardstick_output_inflates_back():
    for c in cases.all_cases():
        assert zlib.decompress(cases.yardstick(c), cases.WBITS[c[3]]) == c[1], c[0]


def test_every_case_is_the_concatenation_of_its_independent_pieces():
    for name, data, level, fmt, pos in cases.all_cases():
        y = cases.compress(data, level, fmt, pos)
        body = y[cases.HEADER[fmt]:len(y) - cases.TRAILER[fmt]]
        ps = cases.pieces(data, level, pos)
        assert body == b"".join(ps), name
        assert all(p.endswith(cases.MARKER) for p in ps[:-1]), name


def test_the_restart_offsets_are_behind_the_markers():
    g = cases.golden()
    for c in cases.all_cases():
        name, data, level, fmt, pos = c
        if fmt != "deflate-raw":
            continue
        y = cases.yardstick(c)
        assert len(g[name][2]) == len(pos), name
        for off, p in zip(g[name][2], pos):
            assert y[off - 4:off] == cases.MARKER and zlib.decompress(y[off:], -15) == data[p:], name


def test_every_case_stays_within_the_bound():
    worst = None
    for c in cases.all_cases():
        name, data, level, fmt, pos = c
        room = cases.bound(len(data), fmt, len(pos)) - cases.golden()[name][0]
        assert room >= 0, name
        worst = room if worst is None else min(worst, room)
    assert worst is not None


def test_the_cut_cases_are_what_they_say():
    """finished alone, filler(16383) at level 1 has a trailing empty static block; flushed, it has none;
    at level 6 the deferred literal keeps the block open and there is none either way"""
    import deflate_header

    def blocks(level, n, flush):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
        out = c.compress(cases.filler(n)) + (c.flush(zlib.Z_FULL_FLUSH) if flush else b"") + c.flush()
        return [(b.type, len(b.symbols)) for b in deflate_header.parse(out)]

    alone, flushed = blocks(1, 16383, False), blocks(1, 16383, True)
    assert len(alone) == 2 and alone[1][0] == 1  # the block of 16,383 literals, then an empty static one
    assert len(flushed) == 3 and flushed[0] == alone[0] and flushed[1][0] == 0  # ..., the marker, the final block
    assert len(blocks(6, 16383, False)) == 1 and len(blocks(6, 16383, True)) == 3
    assert len(blocks(1, 16382, False)) == 1 and len(blocks(1, 16382, True)) == 3
