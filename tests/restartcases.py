"""Inputs of the restart-point tests (test_gpu_inflate_restart.py): streams flushed with Python's zlib,
whose cumulative output lengths at the Z_FULL_FLUSH points are the index.  Any zlib serves: the expected
output of a decode is the source."""
import itertools
import zlib

import corpus

WBITS = {"deflate-raw": -15, "deflate": 15, "gzip": 31}
FORMATS = ("deflate-raw", "deflate", "gzip")
RESTART_MSG = "restart points do not decode the stream"
FAILED = (-3, 2, RESTART_MSG, b"", 0, 0)  # ZS_DATA_ERROR, ZS_PHASE_PROCESS, the message, no bytes, consumed, check


def flushed(data, points, fmt, level=6):
    """`data` compressed with a full flush at every position of `points` (increasing): the stream and
    its restart points [(in_pos, out_pos)], without the start."""
    co = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt])
    out, idx, at = b"", [], 0
    for p in points:
        out += co.compress(data[at:p]) + co.flush(zlib.Z_FULL_FLUSH)
        idx.append((len(out), p))
        at = p
    out += co.compress(data[at:]) + co.flush()
    return out, idx


def check_value(data, fmt):
    return zlib.adler32(data) if fmt == "deflate" else zlib.crc32(data) if fmt == "gzip" else 0


def subsets(positions):
    for k in range(len(positions) + 1):
        for c in itertools.combinations(positions, k):
            yield list(c)


def tiny_cases():
    """b"abc" with every subset of the positions {0, 1, 2, 3}, the empty input with {} and {0}"""
    return [(b"abc", ps) for ps in subsets([0, 1, 2, 3])] + [(b"", ps) for ps in subsets([0])]


def text(n, seed=7):
    return corpus.text(corpus.stream_seed(seed), n)


def cap4(n):
    return (n + 3) & ~3
