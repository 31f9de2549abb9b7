"""Inputs of the preset-dictionary tests: members the system zlib writes against a
dictionary (zlib.compressobj(level, DEFLATED, wbits, 8, 0, zdict)), and hand-built
raw members (bitbuild) whose copies reach into the dictionary.  Every member here
is single-call (at most 32 KiB of input, 64 KiB of output), so the expected bytes
are the plaintext: the reference's one inflate() call copies from the window by
inflate_fast's contiguous branches only (inffast.ts:113-126,149-162)."""
import functools
import zlib

import bitbuild
import corpus

DICT_LENS = [1, 2, 3, 257, 32767, 32768, 40000]  # 40000: only the last 32,768 bytes count
LEVELS = [1, 6, 9]
W = {"deflate-raw": -15, "deflate": 15}


@functools.lru_cache(maxsize=None)
def dictionary(L, seed=900):
    return corpus.text(corpus.stream_seed(seed), L)


@functools.lru_cache(maxsize=None)
def record(i):
    return corpus.text(corpus.stream_seed(1000 + i), 100 + 61 * i)


def compress(data, level, fmt, zdict=None):
    if zdict:
        c = zlib.compressobj(level, zlib.DEFLATED, W[fmt], 8, 0, zdict)
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, W[fmt], 8, 0)
    return c.compress(data) + c.flush()


@functools.lru_cache(maxsize=None)
def members(L, fmt, n=64, seed=900):
    """[(compressed, plaintext)]: record i % 64 at level LEVELS[i % 3] against dictionary(L, seed)"""
    d = dictionary(L, seed)
    return tuple((compress(record(i % 64), LEVELS[i % 3], fmt, d), record(i % 64)) for i in range(n))


def inflate_ref(comp, fmt, zdict):
    """(bytes, consumed) by the system zlib"""
    d = zlib.decompressobj(W[fmt], zdict) if zdict else zlib.decompressobj(W[fmt])
    out = d.decompress(comp)
    assert d.eof
    return out, len(comp) - len(d.unused_data)


def cap4(n):
    """a capacity for n output bytes: n rounded up to 4 (at least 4)"""
    return max(4, (n + 3) & ~3)


def hand_built(L):
    """Raw members over dictionary(L), dl = min(L, 32768) bytes of it in the window:
    name -> (member, expected bytes or None where the distance is too far back)."""
    d = dictionary(L)
    dl = min(L, 32768)
    tail = d[-dl:]

    def expand(symbols):
        out = bytearray(tail)
        for s in symbols:
            if s[0] == "lit":
                out.append(s[1])
            else:
                for _ in range(s[1]):
                    out.append(out[-s[2]])
        return bytes(out[dl:])

    cases = {}
    # the first symbol a copy of length 258 at distance exactly dl (dl < 258: it crosses into the output)
    first = [("copy", 258, dl), ("lit", 65)]
    cases["first_copy_at_dl"] = (bitbuild.build(first, d64=False), expand(first))
    if dl >= 5:
        # length 258 at distance 5 at output position 0: crosses the boundary, then overlaps itself
        over = [("copy", 258, 5), ("lit", 66), ("copy", 20, 3)]
        cases["cross_with_overlap"] = (bitbuild.build(over, d64=False), expand(over))
    # a copy that ends exactly at the boundary (its last byte is the dictionary's last), after some output
    # (the shortest copy is 3 bytes: none lies within a shorter dictionary)
    if dl >= 3:
        k = min(dl, 37)
        edge = [("lit", 67), ("lit", 68), ("lit", 69), ("copy", k, k + 3), ("lit", 70)]
        cases["ends_at_boundary"] = (bitbuild.build(edge, d64=False), expand(edge))
    # distance dl + 1 at output position 0: one byte past the window (32,769 has no distance code)
    if dl + 1 <= 32768:
        cases["too_far"] = (bitbuild.build([("copy", 3, dl + 1), ("lit", 71)], d64=False), None)
    for name, (m, want) in cases.items():
        if want is not None:
            assert inflate_ref(m, "deflate-raw", d)[0] == want, name
    return cases
