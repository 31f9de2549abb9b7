"""The cases of the Z_FULL_FLUSH tests (zs_deflate_batch_flush*): name -> (data, level, format,
flush positions).  The expected bytes are C zlib 1.2.11's -- zlib.compressobj(level, DEFLATED,
wbits, 8, 0); each piece between two positions goes in through 32,768-byte compress() calls, as
the reference's stream layer feeds deflate (streams.ts:7,78-84), flush(Z_FULL_FLUSH) follows at
each position and flush() ends the stream; the gzip OS byte is patched to 0xff.
tests/golden/gen_deflate_flush.py writes (length, sha256[:16]) per case into
tests/golden/deflate_flush.json -- for a deflate-raw case also the offsets behind its markers,
where a decoder can restart -- and the GPU tests compare against that file.

The groups are the smallest shapes at which the flushed layout can go wrong: see each *_cases
function."""
import functools
import hashlib
import itertools
import json
import os
import zlib

import corpus
from paramcases import filler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_flush.json")
FMTS = ["deflate-raw", "deflate", "gzip"]
WBITS = {"deflate-raw": -15, "deflate": 15, "gzip": 31}
HEADER = {"deflate-raw": 0, "deflate": 2, "gzip": 10}
TRAILER = {"deflate-raw": 0, "deflate": 4, "gzip": 8}
CHUNK = 32768  # the stream layer's input sub-chunk (streams.ts:7)
MARKER = b"\x00\x00\xff\xff"  # the empty stored block's LEN / NLEN, behind its three header bits and the padding


def parts(data, level, fmt, pos):
    """zlib's bytes, one part per flush position and the rest: part j ends with position j's marker"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], 8, 0)
    out, at = [], 0
    for p in list(pos) + [None]:
        end = len(data) if p is None else p
        got = [c.compress(data[i:min(i + CHUNK, end)]) for i in range(at, end, CHUNK)]
        got.append(c.flush() if p is None else c.flush(zlib.Z_FULL_FLUSH))
        out.append(b"".join(got))
        at = end
    return out


def compress(data, level, fmt, pos):
    """a gzip header's OS byte reads 0xff as the engine writes it (deflate.ts:799)"""
    out = b"".join(parts(data, level, fmt, pos))
    if fmt == "gzip":
        out = out[:9] + b"\xff" + out[10:]
    return out


def pieces(data, level, pos):
    """the pieces compressed independently, each a fresh raw stream ended by a full flush (the last by Z_FINISH)"""
    out, at = [], 0
    for p in list(pos) + [None]:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
        end = len(data) if p is None else p
        got = [c.compress(data[i:min(i + CHUNK, end)]) for i in range(at, end, CHUNK)]
        got.append(c.flush() if p is None else c.flush(zlib.Z_FULL_FLUSH))
        out.append(b"".join(got))
        at = end
    return out


def bound(n, fmt, n_flush):
    """zs_deflate_bound_flush"""
    return n + (n >> 12) + (n >> 14) + (n >> 25) + 13 - 6 + {"deflate-raw": 0, "deflate": 6, "gzip": 18}[fmt] + 12 * n_flush


def case(group, name, data, level, fmt, pos):
    return ("%s/%s/l%d/%s" % (group, fmt, level, name), data, level, fmt, tuple(pos))


def every(n, step):
    return tuple(range(step, n, step))


def tiny_cases():
    """b"abc" with every subset of the positions {0, 1, 2, 3}, and the empty input flushed at 0: the marker
    alone behind the header, the marker before the empty final block, pieces of one byte"""
    out = []
    for fmt in FMTS:
        for level in (1, 6):
            for k in range(5):
                for pos in itertools.combinations(range(4), k):
                    out.append(case("tiny", "abc@" + "".join(map(str, pos)), b"abc", level, fmt, pos))
            out.append(case("tiny", "empty@0", b"", level, fmt, (0,)))
            out.append(case("tiny", "empty@", b"", level, fmt, ()))
    return out


CUT_LENS = (16382, 16383, 16384, 32766)


def cut_cases():
    """filler(n) + b"tail" flushed at n, around the 16,383-symbol cut: at level 1 a piece of 16,383
    bytes without a match ends exactly on the cut, and finished alone it has a trailing empty static
    block which the flush does not write (`if (s.sym_next) FLUSH_BLOCK(s, 0)`); at level 6 the lazy
    parse's deferred literal keeps the block open"""
    out = []
    for level in (1, 6):
        for n in CUT_LENS:
            out.append(case("cut", "fill%d" % n, filler(n) + b"tail", level, "deflate-raw", (n,)))
    return out


def seam_inputs():
    a = corpus.text(corpus.stream_seed(6000), 820)  # pieces of 1 .. 40 bytes
    pa = tuple(itertools.accumulate(range(1, 41)))
    assert pa[-1] == len(a)
    b = corpus.text(corpus.stream_seed(6001), 300)  # 300 pieces of one byte
    return (("T1to40", a, pa), ("T300x1", b, tuple(range(1, 300))))


def seam_cases():
    """many short pieces: neighbouring segments share output words at every byte phase"""
    out = []
    for name, x, pos in seam_inputs():
        for level in (1, 6):
            for fmt in FMTS:
                out.append(case("seams", name, x, level, fmt, pos))
    return out


def stored_cases():
    """40,000 random bytes flushed at 10,000 and 20,001: stored blocks, byte-aligned inside their segments"""
    x = corpus.rand(6100, 40000)
    return [case("stored", "rand40000", x, level, fmt, (10000, 20001)) for level in (1, 6)
            for fmt in ("deflate-raw", "gzip")]


WINDOW_LEVELS = (1, 6, 9)


def window_cases():
    """200,000 bytes of text: flushed every 65,536 bytes (segments of one sweep window) and once at 70,000
    (a 130,000-byte segment of several sweep windows whose first starts inside the stream)"""
    x = corpus.text(corpus.stream_seed(6200), 200000)
    out = []
    for level in WINDOW_LEVELS:
        out.append(case("windows", "T200000every65536", x, level, "deflate-raw", every(len(x), 65536)))
        out.append(case("windows", "T200000at70000", x, level, "deflate-raw", (70000,)))
    out.append(case("windows", "T200000at70000", x, 6, "gzip", (70000,)))
    return out


def many_cases():
    """1 MiB flushed every 4,096 bytes: 256 segments, one more than a workgroup of the layout scan"""
    x = b"".join(corpus.text(corpus.stream_seed(6300 + i), 65536) for i in range(16))
    return [case("many", "T1Mevery4096", x, level, "deflate-raw", every(len(x), 4096)) for level in (1, 6)]


def mixed_cases():
    """streams with 0, 1 and 7 flush points and different lengths in one call"""
    out = []
    for fmt in FMTS:
        for level in (1, 6):
            for i, (n, pos) in enumerate(((5000, ()), (0, ()), (30000, (12345,)), (69999, every(69999, 8750)),
                                          (33, ()), (9000, (9000,)), (100, (0,)))):
                x = corpus.mixed(corpus.stream_seed(6400 + i), n)
                out.append(case("mixed", "M%d_%d" % (n, len(pos)), x, level, fmt, pos))
    return out


GROUPS = {"tiny": tiny_cases, "cut": cut_cases, "seams": seam_cases, "stored": stored_cases,
          "windows": window_cases, "many": many_cases, "mixed": mixed_cases}


@functools.lru_cache(maxsize=None)
def group(name):
    return tuple(GROUPS[name]())


def all_cases():
    return [c for g in GROUPS for c in group(g)]


def by_call(cases):
    """the cases in batches of one (level, format) each: one engine call"""
    calls = {}
    for c in cases:
        calls.setdefault(c[2:4], []).append(c)
    return list(calls.values())


def yardstick(c):
    name, data, level, fmt, pos = c
    return compress(data, level, fmt, pos)


def digest(b):
    return [len(b), hashlib.sha256(b).hexdigest()[:16]]


def entry(c):
    """a case's golden: the digest; for deflate-raw also the offsets behind the markers"""
    name, data, level, fmt, pos = c
    e = digest(yardstick(c))
    if fmt == "deflate-raw":
        e.append(list(itertools.accumulate(len(p) for p in parts(data, level, fmt, pos)[:-1])))
    return e


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)
