"""The cases of the windowBits / memLevel tests (zs_deflate_batch_params*): name ->
(data, level, format, window_bits, mem_level).  The expected bytes are C zlib 1.2.11's --
zlib.compressobj(level, DEFLATED, wbits, mem_level, 0) fed in 32,768-byte compress() calls
and then flush(), as the reference's stream layer feeds deflate (streams.ts:7,78-84), the
gzip OS byte patched to 0xff: tests/golden/gen_deflate_params.py writes (length,
sha256[:16]) per case into tests/golden/deflate_params.json and the GPU tests compare
against that file.

The groups are the smallest shapes at which a kernel that still assumed a 32 KiB window, a
15-bit hash or 16,383 symbols per block would go wrong: see each *_cases function."""
import functools
import hashlib
import json
import os
import zlib

import corpus

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_params.json")
FMTS = ["deflate-raw", "deflate", "gzip"]
CHUNK = 32768  # the stream layer's input sub-chunk (streams.ts:7)
MIN_LOOKAHEAD = 262


def wbits_code(fmt, window_bits):
    """deflateInit2_'s windowBits argument"""
    return -window_bits if fmt == "deflate-raw" else window_bits + 16 if fmt == "gzip" else window_bits


def compress(data, level, fmt, window_bits, mem_level):
    """zlib's bytes; a gzip header's OS byte reads 0xff as the engine writes it (deflate.ts:799)"""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits_code(fmt, window_bits), mem_level, 0)
    out = b"".join(c.compress(data[i:i + CHUNK]) for i in range(0, len(data), CHUNK)) + c.flush()
    if fmt == "gzip":
        out = out[:9] + b"\xff" + out[10:]
    return out


def bound(n, fmt, window_bits, mem_level, level):
    """deflateBound (deflate.ts:619-673) for these parameters"""
    w_bits, hash_bits = max(window_bits, 9), mem_level + 7
    wraplen = {"deflate-raw": 0, "deflate": 6, "gzip": 18}[fmt]
    if w_bits != 15 or hash_bits != 15:
        fixedlen = n + (n >> 3) + (n >> 8) + (n >> 9) + 4
        storelen = n + (n >> 5) + (n >> 7) + (n >> 11) + 7
        return (fixedlen if w_bits <= hash_bits and level else storelen) + wraplen
    return n + (n >> 12) + (n >> 14) + (n >> 25) + 13 - 6 + wraplen


@functools.lru_cache(maxsize=None)
def filler(n):
    """n bytes in which no three-byte string occurs twice (a prefix of the de Bruijn sequence
    B(256, 3) in its Lyndon-word order: no match anywhere, every byte a literal).  Below
    196,608 bytes every three-byte string in it holds a zero byte."""
    assert n <= 196608
    k, m = 256, 3
    a, seq = [0] * (k * m), []

    def db(t, p):
        if len(seq) >= n:
            return
        if t > m:
            if m % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            if len(seq) >= n:
                return
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return bytes(seq[:n])


MARKER = bytes([200, 201, 202])  # no zero byte: not in the filler


def marked(n, P, d):
    """the filler with the marker at P - d and at P: the match under test, at distance d (the bytes
    around a marker can add a stray short match at another distance; dist_found looks for d alone)"""
    x = bytearray(filler(n))
    assert P - d >= 1 and P + 3 <= n
    x[P - d:P - d + 3] = MARKER
    x[P:P + 3] = MARKER
    if x[P - 1] == x[P - d - 1]:  # keep the match from starting a byte early
        x[P - d - 1] = 251
    return bytes(x)


def case(group, name, data, level, fmt, window_bits, mem_level):
    return ("%s/%s/l%d/w%d/m%d/%s" % (group, fmt, level, window_bits, mem_level, name), data, level, fmt, window_bits,
            mem_level)


TINY_WINDOWS = {"deflate": range(8, 16), "gzip": range(9, 16), "deflate-raw": range(9, 16)}


def tiny_cases():
    """0..3 bytes in every format and window: the header bytes (CINFO, FCHECK), the empty final block"""
    out = []
    for fmt in FMTS:
        for wb in TINY_WINDOWS[fmt]:
            for n in range(4):
                out.append(case("tiny", "n%d" % n, b"abc"[:n], 6, fmt, wb, 8))
            out.append(case("tiny", "n3", b"abc", 1, fmt, wb, 1))
    return out


HASH_LEVELS = [1, 3, 4, 6, 9]


@functools.lru_cache(maxsize=None)
def hash_inputs():
    return (("T8192", corpus.text(corpus.stream_seed(5000), 8192)), ("M8192", corpus.mixed(corpus.stream_seed(5001), 8192)))


def hash_cases():
    """every hash width on 8 KiB: memLevel 9 at window 15 is the global-head instance at
    levels 1..3 and the two-pass link build at 4..9; memLevel 9 at window 12 the LDS-head one"""
    out = []
    for level in HASH_LEVELS:
        for ml in range(1, 10):
            for name, x in hash_inputs():
                out.append(case("hash", name, x, level, "deflate-raw", 15, ml))
        for name, x in hash_inputs():
            out.append(case("hash", name, x, level, "deflate-raw", 12, 9))
            out.append(case("hash", name, x, level, "deflate", 10, 3))
    return out


def cut_cases():
    """the block cut after lit_bufsize - 1 symbols: 127 at memLevel 1 (bytes without a match: one
    symbol each), 32,767 at memLevel 9 -- there a full block's literal/length tree totals 32,768"""
    out = []
    for level in (1, 6):
        for n in (126, 127, 128, 254, 255):
            out.append(case("cut", "fill%d" % n, filler(n), level, "deflate-raw", 15, 1))
            out.append(case("cut", "fill%d" % n, filler(n), level, "deflate-raw", 9, 1))
        for n in (32766, 32767, 32768, 32769):
            out.append(case("cut", "rand%d" % n, corpus.rand(5100, n), level, "deflate-raw", 15, 9))
            out.append(case("cut", "fill%d" % n, filler(n), level, "deflate-raw", 15, 9))
    return out


SLIDE_WINDOWS = [9, 12]


def slide_lens(w):
    return sorted(set(list(range(2 * w - 263, 2 * w - 259)) + [2 * w - 1, 2 * w, 2 * w + 1] +
                      [3 * w - 263, 3 * w - 262, 3 * w - 261] + [32767, 32768, 32769] + [65535, 65536, 65537, 65538]))


def slide_cases():
    """stream lengths around fill_window's slide positions (deflate.ts:180-190) for w = 512 and 4096"""
    out = []
    for wb in SLIDE_WINDOWS:
        for i, n in enumerate(slide_lens(1 << wb)):
            x = corpus.text(corpus.stream_seed(5200 + i), n)
            for level in (1, 6):
                out.append(case("slide", "T%d" % n, x, level, "deflate-raw", wb, 8))
    return out


def dist_cases():
    """one match at distance MAX_DIST - 1, MAX_DIST, MAX_DIST + 1 and w: away from any slide, and at a
    slide position P = 2 w - 262 + w, where with n - P < 262 the slide empties the head at exactly MAX_DIST
    (zs_parse.h: the NIL corner) and with n - P >= 262 it does not"""
    out = []
    for wb in SLIDE_WINDOWS:
        w = 1 << wb
        md = w - MIN_LOOKAHEAD
        for d in (md - 1, md, md + 1, w):
            for pname, P, tail in (("away", 5 * w + 77, 400), ("slide_end", 3 * w - MIN_LOOKAHEAD, 100),
                                   ("slide_more", 3 * w - MIN_LOOKAHEAD, 400)):
                x = marked(P + tail, P, d)
                for level in (1, 6):
                    out.append(case("dist", "%s_d%d" % (pname, d), x, level, "deflate-raw", wb, 8))
    return out


def dist_found(c, out):
    """(a copy at the case's distance is in the raw deflate stream `out`, it should be): the distance is in
    reach up to MAX_DIST, and at the slide position with the input ending inside the lookahead only below it"""
    import deflate_header

    name, _, _, _, wb, _ = c
    kind, d = name.rsplit("/", 1)[1].rsplit("_d", 1)
    d, md = int(d), (1 << wb) - MIN_LOOKAHEAD
    found = any(s[0] == "copy" and s[2] == d for b in deflate_header.parse(out) for s in b.symbols)
    return found, d < md if kind == "slide_end" else d <= md


def stored_cases():
    """40,000 random bytes: once a block's start has slid out of the window it cannot be stored
    (deflate.ts:1120-1124); at memLevel 1 the output comes close to deflateBound"""
    x = corpus.rand(5300, 40000)
    out = []
    for wb in (9, 12, 15):
        for ml in (8, 1):
            for level in (1, 6):
                out.append(case("stored", "rand40000", x, level, "deflate-raw", wb, ml))
    out.append(case("stored", "rand40000", x, 6, "deflate", 9, 8))
    out.append(case("stored", "rand40000", x, 6, "gzip", 12, 1))
    return out


LONG_PARAMS = [(9, 1), (12, 4), (15, 9)]


def long_cases():
    out = []
    for i, (wb, ml) in enumerate(LONG_PARAMS):
        x = corpus.text(corpus.stream_seed(5400 + i), 200000)
        for level in (1, 6, 9):
            out.append(case("long", "T200000", x, level, "deflate-raw", wb, ml))
    return out


GROUPS = {"tiny": tiny_cases, "hash": hash_cases, "cut": cut_cases, "slide": slide_cases, "dist": dist_cases,
          "stored": stored_cases, "long": long_cases}


@functools.lru_cache(maxsize=None)
def group(name):
    return tuple(GROUPS[name]())


def all_cases():
    return [c for g in GROUPS for c in group(g)]


def by_call(cases):
    """the cases in batches of one (level, format, window_bits, mem_level) each: one engine call"""
    calls = {}
    for c in cases:
        calls.setdefault(c[2:], []).append(c)
    return list(calls.values())


def yardstick(c):
    name, data, level, fmt, window_bits, mem_level = c
    return compress(data, level, fmt, window_bits, mem_level)


def digest(b):
    return [len(b), hashlib.sha256(b).hexdigest()[:16]]


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)
