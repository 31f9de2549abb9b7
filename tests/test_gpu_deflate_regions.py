"""zs_deflate_batch_device_ex at levels 0 .. 9 through the harness of regioncases.py: every stream three
times in one batch -- with a capacity of exactly its output rounded up to 4, with zs_deflate_bound rounded
up, and 4 bytes short -- in regions at every 4-byte residue of 16 with one dword of canary between them at
the narrowest, the inputs at odd offsets between filler bytes.

The expected bytes are the oracle's (oracle.compress), so the capacities come from the reference and not
from the engine; level 0, which the oracle does not restate, takes the host entry's output (pinned to the
reference by test_gpu_deflate.py::test_level0_stored_layout_matches_reference_goldens).  A stream that fits
equals the expected one in bytes, status, length and check value; one that does not reports Z_BUF_ERROR and
length 0 and leaves its whole region as it was (zs_k_layout decides before any store; zs_k_stored at level
0) -- the rule test_gpu_boundary.py states for level 0, here at every level.  No byte outside the regions
and no input byte changes."""
import functools

import pytest

import corpus
import oracle
import regioncases as rc

pytestmark = pytest.mark.gpu

FORMATS = ["deflate-raw", "deflate", "gzip"]
LEVELS = [0, 1, 2, 3, 4, 6, 9]  # zs_k_stored; zs_k_fast's three instances; the sweep / parse / trees / emit path
# 0, 1 and 5 bytes; 4,095; one window's 65,536, a second window's first byte, 200,000 (several windows): text,
# mixed, random (the encoder's stored blocks) and zeros
MEMBERS = [("text", 0), ("rand", 1), ("text", 5), ("text", 4095), ("rand", 4095), ("zeros", 4095), ("text", 65536),
           ("mixed", 65536), ("mixed", 65537), ("zeros", 65537), ("rand", 65537), ("text", 200000), ("mixed", 200000),
           ("zeros", 200000), ("rand", 200000)]


@functools.lru_cache(maxsize=None)
def source(kind, n):
    return corpus.make({"kind": kind, "n": n, "seed": corpus.stream_seed(700 + n % 97)})


@functools.lru_cache(maxsize=None)
def reference(kind, n, level, fmt):
    st, out, _ = oracle.compress(source(kind, n), level, fmt)
    assert st == 1
    return out


def check_value(data, fmt):
    """strm.adler after the stream (zs_gpu.h): adler32 / crc32 of the input, 1 for deflate-raw"""
    return oracle.adler32(data) if fmt == "deflate" else oracle.crc32(data) if fmt == "gzip" else 1


def run_level(engine, level, fmt, kind):
    import zsamd

    datas = [source(k, n) for k, n in MEMBERS]
    if level == 0:
        want = [out for st, out in engine.compress_batch_raw(datas, fmt, 0) if st == 1]
        assert len(want) == len(datas)
    else:
        want = [reference(k, n, level, fmt) for k, n in MEMBERS]
    streams, caps, fits = [], [], []
    for d, w in zip(datas, want):
        bound = rc.cap4(zsamd.deflate_bound(len(d), fmt))
        assert bound >= rc.cap4(len(w)) >= 4
        for cap in (rc.cap4(len(w)), bound, rc.cap4(len(w)) - 4):
            streams.append(d)
            caps.append(cap)
            fits.append(w if cap >= len(w) else None)
    run = rc.deflate_run(engine, level, fmt, streams, caps, kind)
    assert not run.dirty, "level %d %s: bytes outside every region changed at %r" % (level, fmt, run.dirty)
    assert run.input_kept, (level, fmt)
    assert {o % 16 for o in run.offs} == {0, 4, 8, 12}
    for i, (d, w, (st, out, chk)) in enumerate(zip(streams, fits, run.rows)):
        where = (level, fmt, i, MEMBERS[i // 3], caps[i], st, run.out_len[i])
        if w is None:  # it does not fit: Z_BUF_ERROR, length 0, nothing written
            assert (st, run.out_len[i]) == (oracle.Z_BUF_ERROR, 0), where
            assert run.region(i) == bytes([rc.CANARY]) * caps[i], where
        else:
            assert st == 1 and out == w, where + (len(w),)
            assert chk == check_value(d, fmt), where
    return run


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("level", LEVELS)
def test_levels(engine, level, fmt):
    run_level(engine, level, fmt, rc.FILLERS[(level + FORMATS.index(fmt)) % 3])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("waves", [1, 2])
def test_level_6_with_one_and_two_parse_waves(engine, waves, fmt):
    """zs_k_parse and zs_k_parse_2w (the default below 2,048 streams is two)"""
    with rc.options(engine, parse_waves=waves):
        run_level(engine, 6, fmt, rc.FILLERS[waves])
