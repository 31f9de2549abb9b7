"""zs_k_bucket's member array (zs_debug_fetch kind 7) against a host stable sort.

The members of a window are its inserted positions 0 .. m-1 sorted by (15-bit
hash, position), u16.  Checked for both instances of the kernel (lane_order 1:
the LDS atomics' lane order; 0: ranks by zs_wave_match) on one batch of short
streams whose lengths sit around the kernel's boundaries -- the 64 positions of
a claim instruction, the 2048 positions of a pass-2 chunk (m one below, on and
one past it, and twice that), the 65,535 positions of a window -- and whose
contents put everything into one bucket, into two, into two buckets that share
a count word, into about every bucket, and into few coarse hash ranges with many
buckets each.  The compressed bytes are checked against the oracle as well."""
import ctypes

import numpy as np
import pytest

import corpus
import oracle

CHUNK = 2048  # ZS_BK_CHUNK
FIRST = 65520  # ZS_SEG_FIRST: own positions of a long stream's first window


def _zeros(seed, n):
    return bytes(n)


def _abab(seed, n):
    return (b"ab" * (n // 2 + 1))[:n]


def _pair(seed, n):  # hashes of "aab" and "aac" differ in bit 0 only: the two buckets share a count word
    r = np.random.RandomState(seed).randint(0, 2, n // 3 + 1)
    return b"".join((b"aab", b"aac")[k] for k in r)[:n]


def _nibble(seed, n):  # 16 coarse hash ranges (h >> 9) of 256 buckets each, about n / 16 members per range
    return (np.random.RandomState(seed).randint(0, 16, n) + 0x20).astype(np.uint8).tobytes()


KINDS = {"zeros": _zeros, "abab": _abab, "pair": _pair, "nibble": _nibble, "rand": corpus.rand, "text": corpus.text}

SPECS = [("text", 3), ("rand", 4), ("zeros", 5), ("text", 66), ("pair", 67), ("abab", 130),
         ("text", CHUNK + 1), ("rand", CHUNK + 2), ("pair", CHUNK + 3), ("zeros", CHUNK + 2),
         ("abab", 2 * CHUNK + 1), ("text", 2 * CHUNK + 2), ("rand", 2 * CHUNK + 3), ("nibble", 2 * CHUNK + 3),
         ("text", 8192 + 2), ("zeros", 8192 + 3), ("rand", 8192 + 1), ("pair", 3 * 8192 + 2),
         ("zeros", 65535), ("text", 65535), ("rand", 65536), ("text", 65536), ("abab", 65536), ("pair", 65536),
         ("nibble", 65536), ("zeros", 65537), ("rand", 65537), ("text", 65537),
         ("text", 65538), ("rand", 98303)]  # the last two: windowed streams (their first windows are fetched)


def _members(d):
    """the first window's members: its inserted positions, stable-sorted by hash"""
    n = len(d)
    m = 0 if n < 3 else (n - 2 if n <= 65537 else FIRST)
    b = np.frombuffer(d, dtype=np.uint8)[:m + 2].astype(np.uint32)
    h = ((b[:m] << 10) ^ (b[1:m + 1] << 5) ^ b[2:m + 2]) & 0x7fff
    return np.argsort(h, kind="stable").astype(np.uint16)


@pytest.fixture(scope="module")
def streams():
    data = [KINDS[k](9900 + i, n) for i, (k, n) in enumerate(SPECS)]
    return data, [_members(d) for d in data], [oracle.compress(d, 6, "deflate-raw")[1] for d in data]


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 0])
def test_members_equal_host_stable_sort(engine, streams, order):
    data, want, ref = streams
    try:
        engine.set_option("lane_order", order)
        res = engine.compress_batch_raw(data, "deflate-raw", 6)
        got = [np.frombuffer(engine.bucket_members(i), dtype=np.uint16) for i in range(len(data))]
    finally:
        engine.set_option("lane_order", 1)
    for i, (k, n) in enumerate(SPECS):
        assert got[i].size == want[i].size and np.array_equal(got[i], want[i]), (k, n)
        assert res[i] == (1, ref[i]), (k, n)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 0])
def test_members_of_a_stream_at_an_odd_address(engine, order):
    """the packed input starts one byte into the buffer: the kernel's byte-wise loads"""
    import zsamd

    L = zsamd.lib()
    d = corpus.text(9950, 2 * CHUNK + 70)
    buf = b"\x55" + d
    out = ctypes.create_string_buffer(len(d) + 1024)
    st = (ctypes.c_int32 * 1)()
    ol = (ctypes.c_uint32 * 1)()
    try:
        engine.set_option("lane_order", order)
        r = L.zs_deflate_batch(engine.handle, 6, -15, 1, buf, (ctypes.c_uint64 * 1)(1), (ctypes.c_uint32 * 1)(len(d)),
                               out, (ctypes.c_uint64 * 1)(0), (ctypes.c_uint32 * 1)(len(d) + 1024), st, ol)
        got = np.frombuffer(engine.bucket_members(0), dtype=np.uint16)
    finally:
        engine.set_option("lane_order", 1)
    assert r == 0 and st[0] == 1
    assert np.array_equal(got, _members(d))
    assert out.raw[:ol[0]] == oracle.compress(d, 6, "deflate-raw")[1]
