"""CPU: tests/golden/deflate_primed.json is what C zlib 1.2.11 produces for the cases of
tests/primedcases.py (gen_deflate_primed.py --check, which also inflates every case back as ONE
stream, asserts zs_deflate_bound_flush, asserts that the 32,768-byte and the whole-piece feed
agree and shows that the cut cases hit their corner).  Skips when the runtime zlib is another
version: the goldens are 1.2.11's.  The checks that read the committed file alone run always."""
import os
import subprocess
import sys
import zlib

import pytest

import primedcases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
zlib_1_2_11 = pytest.mark.skipif(zlib.ZLIB_RUNTIME_VERSION != "1.2.11", reason="the goldens are zlib 1.2.11's")


@zlib_1_2_11
def test_goldens_are_zlib_1_2_11():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_deflate_primed.py"), "--check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases match" % len(cases.all_cases()) in r.stdout


def test_every_case_has_a_golden_and_the_names_are_unique():
    names = [c[0] for c in cases.all_cases()]
    assert len(set(names)) == len(names) and set(names) == set(cases.golden())


def test_every_long_case_is_smaller_primed_than_flushed_at_the_same_positions():
    """a condition the generator checked on the CPU and recorded: [.., .., offsets, [single, flushed]]"""
    g = cases.golden()
    long = cases.group("long")
    assert len(long) == 6
    for c in long:
        primed, (single, flushed) = g[c[0]][0], g[c[0]][3]
        assert primed < flushed and single < flushed, c[0]


@zlib_1_2_11
def test_the_flushed_sizes_recorded_are_the_flush_yardsticks():
    import flushcases

    c = cases.group("long")[0]
    name, data, level, fmt, pos = c
    assert cases.golden()[name][3] == [len(flushcases.compress(data, level, fmt, ())),
                                       len(flushcases.compress(data, level, fmt, pos))]


@zlib_1_2_11
def test_sync_and_full_flush_give_a_piece_the_same_bytes():
    for name, data, level, fmt, pos in cases.group("seams") + cases.group("stored"):
        edges = [0] + list(pos)
        for a, b in zip(edges, edges[1:]):
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0, data[max(0, a - cases.W):a]) if a else \
                zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
            full = c.compress(data[a:b]) + c.flush(zlib.Z_FULL_FLUSH)
            assert full == cases.piece(data, level, a, b, False), (name, a)
            assert full.endswith(cases.MARKER), (name, a)


@zlib_1_2_11
def test_the_offsets_are_behind_the_markers():
    g = cases.golden()
    for c in cases.group("tiny") + cases.group("seams") + cases.group("windows"):
        name, data, level, fmt, pos = c
        if fmt != "deflate-raw":
            continue
        y = cases.yardstick(c)
        assert len(g[name][2]) == len(pos), name
        for off in g[name][2]:
            assert y[off - 4:off] == cases.MARKER, name


@zlib_1_2_11
def test_the_cut_cases_are_what_they_say():
    assert cases.cut_shown()
