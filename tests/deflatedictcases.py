"""The cases of the dictionary-compression tests (zs_deflate_batch_dict*): name ->
(data, dictionary or None, level, format).  The expected bytes are those of zlib
1.2.11's deflateSetDictionary, which deflate.ts:367-424 follows line for line:
tests/golden/gen_deflate_dict.py writes (length, sha256[:16]) of
zlib.compressobj(level, DEFLATED, wbits, 8, 0, zdict) per case into
tests/golden/deflate_dict.json, and the GPU tests compare against that file."""
import functools
import hashlib
import json
import os

import corpus
import dictcases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_dict.json")
FMTS = ["deflate-raw", "deflate"]
LEVELS = list(range(1, 10))
CORNER_LEVELS = [1, 3, 4, 6, 9]
CORNER_DICTS = [32768, 32767, 257]
MIXED_LEVELS = [1, 6]
# the text lengths around MAX_DIST, the window, the first slide and three windows
TEXT_LENS = [32506, 32507, 32606, 32767, 32768, 32769, 32770, 65536, 98604]


@functools.lru_cache(maxsize=None)
def small_inputs():
    """set 1: sixteen records and the inputs of 0, 1, 2 and 3 bytes"""
    return tuple(dictcases.record(i) for i in range(16)) + tuple(corpus.text(corpus.stream_seed(2000), k) for k in range(4))


@functools.lru_cache(maxsize=None)
def corner_inputs():
    """set 2: (name, data) run against each of CORNER_DICTS"""
    out = [("text%d" % n, corpus.text(corpus.stream_seed(3000 + i), n)) for i, n in enumerate(TEXT_LENS)]
    out.append(("mixed200001", corpus.mixed(corpus.stream_seed(3100), 200001)))
    out.append(("zeros70000", bytes(70000)))
    out.append(("rand40000", corpus.rand(3200, 40000)))  # stored blocks after a dictionary
    out.append(("rand32767", corpus.rand(3201, 2 * 16383 + 1)))  # ... and block cuts
    return tuple(out)


@functools.lru_cache(maxsize=None)
def split_inputs():
    """set 2: (name, dictionary, data) -- inputs cut into a dictionary and the data behind it"""
    x = bytearray(corpus.rand(77, 65536))  # a candidate at exactly MAX_DIST, in the dictionary
    x[40000:40020] = x[40000 - 32506:40000 - 32506 + 20]
    x = bytes(x)
    # the head slot a slide empties is the first data position, met < 262 bytes from the end
    y = bytearray(corpus.rand(78, 65374))
    y[65274:65294] = y[32768:32788]
    y = bytes(y)
    return (("a3", x[:32768], x[32768:]),
            ("nil32768", y[:32768], y[32768:]),
            ("nil32767", y[1:32768], y[32768:]))  # one window position lower: no slide is due there


@functools.lru_cache(maxsize=None)
def mixed_blob():
    return dictcases.dictionary(6000, 903)


MIXED_SLICES = [(1, 3001), (777, 2049)]  # (odd byte offset, length) into mixed_blob()


def mixed_dict(k):
    """set 3: stream k's dictionary; ("blob", offset, length) for a slice of the shared blob"""
    if k % 4 == 0:
        return None
    if k % 4 == 1:
        return dictcases.dictionary(257)
    if k % 4 == 2:
        return dictcases.dictionary(32768)
    return ("blob",) + MIXED_SLICES[(k // 4) % 2]


def mixed_dict_bytes(k):
    d = mixed_dict(k)
    if isinstance(d, tuple):
        return mixed_blob()[d[1]:d[1] + d[2]]
    return d


@functools.lru_cache(maxsize=None)
def mixed_inputs():
    return tuple(dictcases.record(k) for k in range(32))


def set1(fmt, level, L):
    d = dictcases.dictionary(L)
    return [("s1/%s/l%d/d%d/i%d" % (fmt, level, L, i), x, d, level, fmt) for i, x in enumerate(small_inputs())]


def set2(level):
    out = []
    for L in CORNER_DICTS:
        d = dictcases.dictionary(L)
        out += [("s2/l%d/d%d/%s" % (level, L, name), x, d, level, "deflate-raw") for name, x in corner_inputs()]
    out += [("s2/l%d/split/%s" % (level, name), x, d, level, "deflate-raw") for name, d, x in split_inputs()]
    return out


def set3(fmt, level):
    return [("s3/%s/l%d/k%d" % (fmt, level, k), x, mixed_dict_bytes(k), level, fmt)
            for k, x in enumerate(mixed_inputs())]


def all_cases():
    out = []
    for fmt in FMTS:
        for level in LEVELS:
            for L in dictcases.DICT_LENS:
                out += set1(fmt, level, L)
    for level in CORNER_LEVELS:
        out += set2(level)
    for fmt in FMTS:
        for level in MIXED_LEVELS:
            out += set3(fmt, level)
    return out


def digest(b):
    return [len(b), hashlib.sha256(b).hexdigest()[:16]]


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)
