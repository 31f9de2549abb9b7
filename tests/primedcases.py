"""The cases of the primed-pieces tests (zs_deflate_batch_primed*; pigz's construction): name ->
(data, level, format, positions).  The expected bytes are C zlib 1.2.11's: the stream's ordinary
wrapper header (zlib: no FDICT; gzip: OS 255), then for every piece data[a:b] between two
positions the bytes of a raw stream of its own -- zlib.compressobj(level, DEFLATED, -15, 8, 0,
zdict=data[max(0, a - 32768):a]) (no zdict for a = 0), the piece in 32,768-byte compress() calls,
flush(Z_SYNC_FLUSH), or flush() for the last piece -- then the trailer over the whole input.
tests/golden/gen_deflate_primed.py writes (length, sha256[:16]) per case into
tests/golden/deflate_primed.json -- for a deflate-raw case also the offsets behind its markers,
for a *long* case also the single-stream and the flushed size -- and the GPU tests compare
against that file.

The groups are the smallest shapes at which a primed piece can go wrong: see each *_cases
function."""
import functools
import itertools
import json
import os
import struct
import zlib

import corpus
import flushcases
from paramcases import filler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_primed.json")
FMTS = flushcases.FMTS
WBITS = flushcases.WBITS
HEADER = flushcases.HEADER
TRAILER = flushcases.TRAILER
CHUNK = flushcases.CHUNK
MARKER = flushcases.MARKER
W = 32768  # the window: a prime's length at most
LEVELS = (1, 3, 4, 6, 9)

bound = flushcases.bound  # zs_deflate_bound_flush bounds a primed call too
case = flushcases.case
every = flushcases.every
by_call = flushcases.by_call
digest = flushcases.digest


def piece(data, level, a, b, last, feed=CHUNK, finish=None):
    """zlib's bytes for the piece data[a:b] primed with the 32 KiB in front of it; feed: the bytes
    per compress() call; finish: Z_FINISH or not, whatever the piece's place (the cut cases' proof)"""
    if a > 0:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0, data[max(0, a - W):a])
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
    got = [c.compress(data[i:min(i + feed, b)]) for i in range(a, b, feed)]
    got.append(c.flush() if (last if finish is None else finish) else c.flush(zlib.Z_SYNC_FLUSH))
    return b"".join(got)


def pieces(data, level, pos, feed=CHUNK):
    edges = [0] + list(pos) + [len(data)]
    return [piece(data, level, edges[j], edges[j + 1], j + 2 == len(edges), feed) for j in range(len(edges) - 1)]


def header(level, fmt):
    """the stream's ordinary wrapper header; gzip's OS byte reads 0xff as the engine writes it"""
    if fmt == "deflate-raw":
        return b""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], 8, 0)
    h = (c.compress(b"") + c.flush())[:HEADER[fmt]]
    return h[:9] + b"\xff" if fmt == "gzip" else h


def trailer(data, fmt):
    if fmt == "deflate":
        return struct.pack(">I", zlib.adler32(data))
    if fmt == "gzip":
        return struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)
    return b""


def compress(data, level, fmt, pos, feed=CHUNK):
    return header(level, fmt) + b"".join(pieces(data, level, pos, feed)) + trailer(data, fmt)


def tiny_cases():
    """b"abc" with every non-empty subset of the positions {0, 1, 2, 3}, and the empty input with a
    point at 0: the marker alone behind the header, primes of 1, 2 and 3 bytes, an empty last piece"""
    out = []
    for fmt in FMTS:
        for level in (1, 6):
            for k in range(1, 5):
                for pos in itertools.combinations(range(4), k):
                    out.append(case("tiny", "abc@" + "".join(map(str, pos)), b"abc", level, fmt, pos))
            out.append(case("tiny", "empty@0", b"", level, fmt, (0,)))
    return out


PRIME_AT = (1, 2, 3, 4, 258, 32505, 32506, 32507, 32767, 32768, 32769)


def prime_cases():
    """70,000 bytes of text with one position: a prime of 1 or 2 bytes (nothing insertable: the
    s.insert corner), the first insertable prime, MAX_DIST = 32,506 and lp saturating at 32,768"""
    x = corpus.text(corpus.stream_seed(7000), 70000)
    return [case("prime", "T70000at%d" % p, x, level, "deflate-raw", (p,)) for level in LEVELS for p in PRIME_AT]


def across_cases():
    """matches that reach back across a point: X || X, a 300-byte period with a point inside a
    258-byte match, and a run of one byte"""
    x = corpus.rand(7100, 1000)
    period = corpus.text(corpus.stream_seed(7101), 300) * 20
    out = []
    for level in LEVELS:
        for pos in ((999,), (1000,), (1001,), (999, 1000, 1001)):
            out.append(case("across", "XX@" + "_".join(map(str, pos)), x + x, level, "deflate-raw", pos))
        for pos in ((700,), (700, 3001)):
            out.append(case("across", "period300@" + "_".join(map(str, pos)), period, level, "deflate-raw", pos))
        for pos in ((1,), (2,), (3,), (2500,), (1, 2, 3, 2500)):
            out.append(case("across", "a5000@" + "_".join(map(str, pos)), b"a" * 5000, level, "deflate-raw", pos))
    return out


WINDOW_PIECES = (32768, 32769, 32770, 65536, 100000, 131072)


def window_cases():
    """a full prime and then a piece of n bytes: lp + n = 65,536, 65,537 (one sweep window) and
    65,538 (two); a slide with the prime in the window; three windows"""
    return [case("windows", "T32768+%d" % n, corpus.text(corpus.stream_seed(7200), W + n), level, "deflate-raw", (W,))
            for level in (1, 6, 9) for n in WINDOW_PIECES]


def stored_cases():
    """stored blocks behind a prime: their copy source lies behind the prime in the piece's window"""
    r = corpus.rand(7300, 40000)
    t = corpus.text(corpus.stream_seed(7301), 20000) + corpus.rand(7302, 20000) + corpus.text(corpus.stream_seed(7303), 20000)
    out = []
    for level in (1, 6):
        for fmt in ("deflate-raw", "gzip"):
            out.append(case("stored", "rand40000", r, level, fmt, (10000, 20001)))
            out.append(case("stored", "TRT60000", t, level, fmt, (20000, 40000)))
    return out


# The cut cases' prime: text (no zero byte), then b"z\xff".  Every three-byte string of filler(n),
# n <= 196,608, holds a zero byte, so none occurs in the prime; the two strings across the point are
# (z, 0xff, 0) and (0xff, 0, 0), and the first 32,766 bytes of filler hold (k, 0xff, 0) for k < 43
# alone and no (0xff, 0, 0): the piece has no match, as flushcases' cut input alone.
CUT_PRIME = corpus.text(corpus.stream_seed(7400), 998) + b"z\xff"


def cut_cases():
    """flushcases' cut input -- filler(n) + b"tail", a point at n -- behind CUT_PRIME: at level 1
    the primed piece of 16,383 bytes without a match ends exactly on the 16,383-symbol cut"""
    out = []
    for level in (1, 6):
        for n in flushcases.CUT_LENS:
            out.append(case("cut", "prime1000+fill%d" % n, CUT_PRIME + filler(n) + b"tail", level, "deflate-raw",
                            (len(CUT_PRIME), len(CUT_PRIME) + n)))
    return out


def cut_shown():
    """How the generator shows that the cut cases hit the corner, on the CPU: it parses zlib's blocks
    (deflate_header.parse) of the primed piece filler(16383) at level 1.  Finished alone (Z_FINISH), the
    piece is the block of 16,383 literals and then an empty static block; ended by the flush it is
    that block and the marker, no empty block between.  One byte less and neither form has it."""
    import deflate_header

    def blocks(level, n, finish):
        d = CUT_PRIME + filler(n)
        out = piece(d, level, len(CUT_PRIME), len(d), False, finish=finish)
        if not finish:  # (a parsable stream: the empty final block behind the marker)
            out += b"\x03\x00"
        return [(b.type, len(b.symbols)) for b in deflate_header.parse(out)]

    alone, flushed = blocks(1, 16383, True), blocks(1, 16383, False)
    assert len(alone) == 2 and alone[0][1] == 16383 and alone[1] == (1, 0), alone
    assert len(flushed) == 3 and flushed[0] == alone[0] and flushed[1][0] == 0, flushed
    assert len(blocks(1, 16382, True)) == 1 and len(blocks(1, 16382, False)) == 3
    assert len(blocks(6, 16383, True)) == 1 and len(blocks(6, 16383, False)) == 3
    return True


def seam_cases():
    """many short pieces: neighbouring segments share output words at every byte phase, and every
    prime is shorter than the window"""
    out = []
    for name, x, pos in flushcases.seam_inputs():
        for fmt in FMTS:
            out.append(case("seams", name, x, 6, fmt, pos))
        for level in (1, 9):
            out.append(case("seams", name, x, level, "deflate-raw", pos))
    return out


def many_cases():
    """1 MiB with a point every 4,096 bytes: 256 segments, two tiles of the layout scan"""
    x = b"".join(corpus.text(corpus.stream_seed(7500 + i), 65536) for i in range(16))
    return [case("many", "T1Mevery4096", x, level, "deflate-raw", every(len(x), 4096)) for level in (1, 6)]


def mixed_cases():
    """streams with 0, 1 and 7 points, an empty stream and odd lengths (odd input offsets) in one call"""
    out = []
    for fmt in FMTS:
        for level in (1, 6):
            for i, (n, pos) in enumerate(((5001, ()), (0, ()), (30001, (12345,)), (69999, every(69999, 8750)),
                                          (33, ()), (9000, (9000,)), (101, (0,)))):
                x = corpus.mixed(corpus.stream_seed(7600 + i), n)
                out.append(case("mixed", "M%d_%d" % (n, len(pos)), x, level, fmt, pos))
    return out


LONG_EVERY = 131072


def long_cases():
    """two streams of 400,000 bytes of text with a point every 131,072: the sizes DESIGN quotes"""
    out = []
    for level in (1, 6, 9):
        for k in range(2):
            x = corpus.text(corpus.stream_seed(7700 + k), 400000)
            out.append(case("long", "T400000_%d" % k, x, level, "deflate-raw", every(len(x), LONG_EVERY)))
    return out


GROUPS = {"tiny": tiny_cases, "prime": prime_cases, "across": across_cases, "windows": window_cases,
          "stored": stored_cases, "cut": cut_cases, "seams": seam_cases, "many": many_cases, "mixed": mixed_cases,
          "long": long_cases}


@functools.lru_cache(maxsize=None)
def group(name):
    return tuple(GROUPS[name]())


def all_cases():
    return [c for g in GROUPS for c in group(g)]


def yardstick(c):
    name, data, level, fmt, pos = c
    return compress(data, level, fmt, pos)


def sizes(c):
    """(single stream, flushed at the same positions): what the primed form is weighed against"""
    name, data, level, fmt, pos = c
    return [len(flushcases.compress(data, level, fmt, ())), len(flushcases.compress(data, level, fmt, pos))]


def entry(c):
    """a case's golden: the digest; for deflate-raw also the offsets behind the markers; for a long
    case also the single-stream and the flushed size"""
    name, data, level, fmt, pos = c
    e = digest(yardstick(c))
    if fmt == "deflate-raw":
        e.append(list(itertools.accumulate(len(p) for p in pieces(data, level, pos)[:-1])))
    if name.startswith("long/"):
        e.append(sizes(c))
    return e


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)
