"""The cases of the compression-strategy tests (zs_deflate_batch_strategy*): name ->
(data, level, format, strategy, rle_ref).  The expected bytes are C zlib 1.2.11's
(zlib.compressobj(level, DEFLATED, wbits, 8, strategy), one compress() + flush(), the
gzip OS byte patched to 0xff): tests/golden/gen_deflate_strategy.py writes (length,
sha256[:16]) per case into tests/golden/deflate_strategy.json and the GPU tests compare
against that file.  Z_RLE has two sets: rle_ref = 0 is zlib's Z_RLE; rle_ref = 1 (the
reference, whose deflate_rle finds no run, deflate.ts:1469-1481) is zlib's
Z_HUFFMAN_ONLY, bit for bit in every format (the wrappers test strategy >= 2)."""
import functools
import hashlib
import json
import os
import zlib

import corpus

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_strategy.json")
Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 1, 2, 3, 4
W = {"deflate-raw": -15, "deflate": 15, "gzip": 31}
FMTS = ["deflate-raw", "deflate", "gzip"]
SYM_END = 16383  # symbols per block (deflate.ts:336)

HUFF_LENS = [0, 1, 2, 3, 16382, 16383, 16384, 32766, 32767, 65537, 200000]
HUFF_LEVELS = [1, 6, 9]  # the wrapper bits (deflate.ts:757,798)
FILT_LEVELS = [4, 6, 9]
FILT_LENS = [4096, 65536, 200000]
FIXED_LEVELS = [1, 4, 9]
# the tally kernel's chunk boundaries: lane (every position), wave (64), workgroup tile (4096)
RLE_BOUNDARIES = [64, 4096, 8192]


def compress(data, level, fmt, strategy):
    """zlib's bytes; a gzip header's OS byte reads 0xff as the engine writes it (deflate.ts:799)"""
    c = zlib.compressobj(level, zlib.DEFLATED, W[fmt], 8, strategy)
    out = c.compress(data) + c.flush()
    if fmt == "gzip":
        out = out[:9] + b"\xff" + out[10:]
    return out


def norun(n, k=0):
    """n bytes without two equal neighbours"""
    return bytes(97 + (i + k) % 7 for i in range(n))


def runs(*parts):
    """bytes from (byte, length) pairs and literal byte strings"""
    out = bytearray()
    for p in parts:
        out += p if isinstance(p, bytes) else bytes([p[0]]) * p[1]
    return bytes(out)


def two_letter(seed, n, letters=b"ab"):
    r = corpus._xs(seed)
    return bytes(letters[next(r) % len(letters)] for _ in range(n))


@functools.lru_cache(maxsize=None)
def huff_inputs():
    """(name, data): texts of HUFF_LENS bytes, and random bytes (blocks the encoder stores)"""
    out = [("text%d" % n, corpus.text(corpus.stream_seed(4000 + i), n)) for i, n in enumerate(HUFF_LENS)]
    out.append(("rand40000", corpus.rand(4100, 40000)))
    return tuple(out)


RUN_LENS = [1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 517, 518, 519]


@functools.lru_cache(maxsize=None)
def rle_inputs():
    """(name, data) of the Z_RLE cases"""
    out = []
    for L in RUN_LENS:  # a run of L between bytes that differ from it
        out.append(("run%d" % L, runs(b"xy", (122, L), b"pq")))
    out.append(("all_lens", runs(*[p for L in RUN_LENS for p in ((65 + L % 20, L), b"-")])))
    out.append(("from0", runs((48, 300), b"end")))          # a run from position 0: its first byte is a literal
    out.append(("to_end", runs(b"start", (49, 777))))       # ... and one ending at the last byte
    out.append(("only_run3", runs((50, 3))))
    out.append(("only_run4", runs((50, 4))))
    out.append(("run70000", runs(b"ab", (51, 70000), b"cd")))
    out.append(("norun5000", norun(5000)))
    out.append(("norun40000", norun(40000)))
    # runs of several lengths across each chunk boundary of the tally kernel
    for B in RLE_BOUNDARIES:
        for L in (3, 4, 5, 259, 300, 600):
            for back in sorted({1, 2, L // 2, L - 1}):
                out.append(("straddle%d_%d_%d" % (B, L, back), runs(norun(B - back), (52, L), norun(300, 1))))
    # a run around a stream's 16,383rd symbol: the block cut falls before, on and behind its matches
    for lead in range(SYM_END - 4, SYM_END + 3):
        out.append(("cut%d" % lead, runs(norun(lead), (53, 600), norun(40, 2), (54, 9), norun(17000, 3))))
    out.append(("ab50000", two_letter(4200, 50000)))
    out.append(("abcd50000", two_letter(4201, 50000, b"abcd")))
    out.append(("ab_a200000", runs(two_letter(4202, 100000), (97, 40000), two_letter(4203, 60000))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def filtered_inputs():
    out = []
    for i, n in enumerate(FILT_LENS):
        out.append(("T%d" % n, corpus.text(corpus.stream_seed(4300 + i), n)))
        out.append(("M%d" % n, corpus.mixed(corpus.stream_seed(4310 + i), n)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fixed_inputs():
    return (("text20000", corpus.text(corpus.stream_seed(4400), 20000)), ("text100", corpus.text(corpus.stream_seed(4401), 100)),
            ("zeros20000", bytes(20000)), ("rand20000", corpus.rand(4402, 20000)), ("empty", b""))


def case(group, name, data, level, fmt, strategy, rle_ref=1):
    return ("%s/%s/l%d/%s%s" % (group, fmt, level, name, "" if strategy != Z_RLE else "/ref%d" % rle_ref), data, level, fmt,
            strategy, rle_ref)


def huff_cases(fmt, level):
    return [case("huff", name, x, level, fmt, Z_HUFFMAN_ONLY) for name, x in huff_inputs()]


def rle_cases(fmt, level, rle_ref):
    return [case("rle", name, x, level, fmt, Z_RLE, rle_ref) for name, x in rle_inputs()]


def filtered_cases(level):
    return [case("filtered", name, x, level, "deflate-raw", Z_FILTERED) for name, x in filtered_inputs()]


def filtered_fast_cases(level):
    """levels 1..3: deflate_fast has no filtered branch"""
    return [case("filtered", name, x, level, "deflate-raw", Z_FILTERED) for name, x in filtered_inputs()[:2]]


def fixed_cases(fmt, level):
    return [case("fixed", name, x, level, fmt, Z_FIXED) for name, x in fixed_inputs()]


def all_cases():
    out = []
    for fmt in FMTS:
        for level in HUFF_LEVELS:
            out += huff_cases(fmt, level)
    for rle_ref in (0, 1):
        out += rle_cases("deflate-raw", 6, rle_ref)
        for fmt in ("deflate", "gzip"):
            for level in (1, 9):
                out += rle_cases(fmt, level, rle_ref)[:16]
    for level in FILT_LEVELS:
        out += filtered_cases(level)
    for level in (1, 2, 3):
        out += filtered_fast_cases(level)
    for level in FIXED_LEVELS:
        out += fixed_cases("deflate-raw", level)
    for fmt in ("deflate", "gzip"):
        out += fixed_cases(fmt, 6)
    return out


def yardstick(c):
    """zlib's bytes for a case (rle_ref = 1: Z_HUFFMAN_ONLY's, see above)"""
    name, data, level, fmt, strategy, rle_ref = c
    return compress(data, level, fmt, Z_HUFFMAN_ONLY if strategy == Z_RLE and rle_ref else strategy)


def digest(b):
    return [len(b), hashlib.sha256(b).hexdigest()[:16]]


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)
