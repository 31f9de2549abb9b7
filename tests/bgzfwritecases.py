"""The cases of the BGZF writer's tests (zs_deflate_batch_bgzf*): (name, data, level, block_bytes), and the
framing of include/zs_gpu.h written out in Python.  A stream is cut every block_bytes; each piece becomes one
gzip member -- the 18-byte header with the BC subfield and BSIZE, the piece as a finished raw-deflate stream
(zlib.compressobj(level, DEFLATED, -15, 8, 0), all input, then flush()), crc32 and ISIZE -- and the 28-byte
end-of-file block ends the stream.  Level 0 is written by hand: one final stored block per piece.
tests/golden/gen_deflate_bgzf.py writes (length, sha256[:16]) per case into tests/golden/deflate_bgzf.json, and
the GPU tests compare against that file.

The groups are the smallest shapes at which the BGZF layout can go wrong: see each *_cases function."""
import functools
import hashlib
import json
import os
import struct
import zlib

import corpus
from paramcases import filler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_bgzf.json")
B = 65280  # ZS_BGZF_BLOCK
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")  # ... then BSIZE


def piece_raw(piece, level):
    """the deflate data of one block"""
    if level == 0:
        return b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xffff) + piece
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
    return c.compress(piece) + c.flush()


def member(piece, level):
    raw = piece_raw(piece, level)
    total = 18 + len(raw) + 8
    assert total <= 65536
    return HEADER + struct.pack("<H", total - 1) + raw + struct.pack("<II", zlib.crc32(piece), len(piece))


def pieces(data, block_bytes):
    return [data[a:a + block_bytes] for a in range(0, len(data), block_bytes)]


def compress(data, level, block_bytes=B):
    return b"".join(member(p, level) for p in pieces(data, block_bytes)) + EOF


def index(data, level, block_bytes=B):
    """[(in_pos, out_pos)] of every block, the end-of-file block's last: what zs_last_bgzf_blocks returns"""
    out, ip, op = [], 0, 0
    for p in pieces(data, block_bytes):
        out.append((ip, op))
        ip, op = ip + len(p), op + len(member(p, level))
    return out + [(ip, op)]


def bound(n, block_bytes=B):
    """zs_deflate_bound_bgzf: the sum over the blocks of zs_deflate_bound(piece, -15) + 26, plus 28"""
    raw = lambda k: k + (k >> 12) + (k >> 14) + (k >> 25) + 7
    return sum(raw(min(block_bytes, n - a)) + 26 for a in range(0, n, block_bytes)) + 28


def case(group, name, data, level, block_bytes=B):
    return ("%s/l%d/b%d/%s" % (group, level, block_bytes, name), data, level, block_bytes)


def empty_cases():
    """the empty input: the end-of-file block alone"""
    return [case("empty", "empty", b"", level) for level in (1, 6)]


EDGE_LENS = (1, B - 1, B, B + 1, 2 * B + 1)
EDGE_LEVELS = (1, 6, 9)


def edge_cases():
    """text of 1, B - 1, B, B + 1 (a one-byte last block) and 2B + 1 bytes"""
    x = corpus.text(corpus.stream_seed(7000), 2 * B + 1)
    return [case("edge", "T%d" % n, x[:n], level) for level in EDGE_LEVELS for n in EDGE_LENS]


def phase_cases():
    """300 blocks of one byte (29-byte members) and 143 of seven bytes: frames at every byte phase of a word"""
    a = corpus.text(corpus.stream_seed(7001), 300)
    b = corpus.text(corpus.stream_seed(7002), 1000)
    return [c for level in (1, 6) for c in (case("phases", "T300", a, level, 1), case("phases", "T1000", b, level, 7))]


CUT = 16383


def cut_cases():
    """filler(16,383) cut at 16,383 with a second piece behind it: at level 1 the first piece's symbols end
    exactly on the 16,383-symbol cut, and finished alone it keeps its trailing empty static block"""
    x = filler(CUT) + corpus.text(corpus.stream_seed(7003), 500)
    return [case("cut", "fill%d" % CUT, x, level, CUT) for level in (1, 6)]


def stored_cases():
    """65,280 random bytes: stored blocks inside a member, at the largest block the format meets"""
    x = corpus.rand(7100, B)
    return [case("stored", "rand%d" % B, x, level) for level in (1, 6, 9)]


def many_cases():
    """153,600 bytes in blocks of 256: 600 segments, three tiles of the layout scan"""
    x = corpus.text(corpus.stream_seed(7200), 153600)
    return [case("many", "T153600", x, level, 256) for level in (1, 6)]


MIXED_BLOCK = 5000


def mixed_cases():
    """streams of 1, 0 and 3 blocks in one call: the empty stream in the middle has no segment"""
    return [case("mixed", "M%d" % n, corpus.mixed(corpus.stream_seed(7300 + i), n), 6, MIXED_BLOCK)
            for i, n in enumerate((3000, 0, 2 * MIXED_BLOCK + 1))]


LEVEL0_LENS = (0, 1, B, B + 1)


def level0_cases():
    x = corpus.text(corpus.stream_seed(7400), B + 1)
    return [case("level0", "T%d" % n, x[:n], 0) for n in LEVEL0_LENS]


GROUPS = {"empty": empty_cases, "edge": edge_cases, "phases": phase_cases, "cut": cut_cases, "stored": stored_cases,
          "many": many_cases, "mixed": mixed_cases, "level0": level0_cases}


@functools.lru_cache(maxsize=None)
def group(name):
    return tuple(GROUPS[name]())


def all_cases():
    return [c for g in GROUPS for c in group(g)]


def by_call(cases):
    """the cases in batches of one (level, block_bytes) each: one engine call"""
    calls = {}
    for c in cases:
        calls.setdefault(c[2:4], []).append(c)
    return list(calls.values())


def yardstick(c):
    name, data, level, block_bytes = c
    return compress(data, level, block_bytes)


def digest(b):
    return [len(b), hashlib.sha256(b).hexdigest()[:16]]


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)
