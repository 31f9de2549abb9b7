"""GPU checks of the data checksums of long streams in parts (zs_k_checksum_parts +
zs_k_checksum_fold): the checksum entries, the deflate wrappers' check values and
the inflate trailer check give what one wave per stream gives, whatever "checksum_split" and
"checksum_part" say.  The small options (split 1, parts of 1024 bytes) cut small buffers into
many parts."""
import ctypes
import random
import zlib

import pytest

from test_gpu_checksum import ref_adler32

pytestmark = pytest.mark.gpu

PART = 1024
# 0 .. one part and a byte; 64 parts (a part per lane of the fold), 64 and a byte, 65, 200 and 7 bytes
LENS = [0, 1, 1023, 1024, 1025, 65536, 65537, 66560, 204807]
DEFAULT_SPLIT, DEFAULT_PART = 1 << 18, 65536


def parts_of(lens, part):
    return sum(max(1, -(-n // part)) for n in lens)


@pytest.fixture
def small(engine):
    """the engine with the small options; the defaults again afterwards"""
    engine.set_option("checksum_split", 1)
    engine.set_option("checksum_part", PART)
    yield engine
    engine.set_option("checksum_split", DEFAULT_SPLIT)
    engine.set_option("checksum_part", DEFAULT_PART)


@pytest.fixture(scope="module")
def bufs():
    rng = random.Random(31)
    return [rng.randbytes(n) for n in LENS]


def device_checksums(engine, kind, bufs, seeds):
    """through the device entry: the buffers packed behind a one-byte prefix (odd offsets)"""
    import torch

    blob = b"\xa5" + b"".join(bufs) + bytes(8)
    d = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    n = len(bufs)
    offs, o = [], 1
    for b in bufs:
        offs.append(o)
        o += len(b)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    sd = (ctypes.c_uint32 * n)(*seeds) if seeds is not None else None
    engine.checksum_device(kind, n, d.data_ptr(), (ctypes.c_uint64 * n)(*offs), (ctypes.c_uint32 * n)(*map(len, bufs)),
                           out.data_ptr(), seeds=sd)
    torch.cuda.synchronize()
    return [int(x) & 0xFFFFFFFF for x in out.cpu().tolist()]


@pytest.mark.parametrize("seed", [None, 0, 1, 0xFFFFFFFF, 0xFFF0FFF0, "random"])
def test_checksum_entries_in_parts(small, bufs, seed):
    rng = random.Random(32)
    n = len(bufs)
    seeds = None if seed is None else [rng.randrange(1 << 32) if seed == "random" else seed for _ in range(n)]
    want_crc = [zlib.crc32(b, 0 if seeds is None else seeds[i]) for i, b in enumerate(bufs)]
    want_adl = [ref_adler32(1 if seeds is None else seeds[i], b) for i, b in enumerate(bufs)]
    assert small.crc32(bufs, seeds) == want_crc
    assert small.last_checksum_parts() == parts_of(LENS, PART) == 401
    assert small.adler32(bufs, seeds) == want_adl
    assert small.last_checksum_parts() == 401
    assert device_checksums(small, "crc32", bufs, seeds) == want_crc
    assert device_checksums(small, "adler32", bufs, seeds) == want_adl
    assert small.last_checksum_parts() == 401
    # the same batch, one wave per stream
    small.set_option("checksum_split", 0)
    assert small.crc32(bufs, seeds) == want_crc and small.last_checksum_parts() == 0
    assert small.adler32(bufs, seeds) == want_adl and small.last_checksum_parts() == 0
    assert device_checksums(small, "adler32", bufs, seeds) == want_adl and small.last_checksum_parts() == 0


@pytest.mark.parametrize("part", [2048, 65536, 1 << 20])
def test_other_part_sizes(small, bufs, part):
    small.set_option("checksum_part", part)
    seeds = [7, 0, 1, 0xFFFFFFFF, 0xFFF0FFF0, 0x80000000, 0x12345678, 0xFFFF0000, 0x0000FFFF]
    assert small.crc32(bufs, seeds) == [zlib.crc32(b, s) for b, s in zip(bufs, seeds)]
    assert small.last_checksum_parts() == parts_of(LENS, part)
    assert small.adler32(bufs, seeds) == [ref_adler32(s, b) for b, s in zip(bufs, seeds)]


def test_default_options(engine):
    rng = random.Random(33)
    big = rng.randbytes((1 << 20) + 1)
    batch = [big] + [rng.randbytes(100) for _ in range(3)]
    assert engine.crc32(batch) == [zlib.crc32(b) for b in batch]
    assert engine.last_checksum_parts() == 17 + 3
    assert engine.adler32(batch) == [zlib.adler32(b) for b in batch]
    assert engine.last_checksum_parts() == 20
    assert engine.adler32(batch, [0xFFF0FFF0] * 4) == [ref_adler32(0xFFF0FFF0, b) for b in batch]
    # streams of at most 256 KiB (the threshold): one wave each; a byte more: parts
    quiet = [big[:262144], big[:1], b"", big[:65537]]
    assert engine.crc32(quiet) == [zlib.crc32(b) for b in quiet] and engine.last_checksum_parts() == 0
    assert engine.adler32([big[:262145]]) == [zlib.adler32(big[:262145])] and engine.last_checksum_parts() == 5


def test_option_values(engine):
    import zsamd

    for name, bad in (("checksum_split", [-1]), ("checksum_part", [0, 512, 1025, 3072, 1 << 21, -1024])):
        for v in bad:
            with pytest.raises(zsamd.ZsError):
                engine.set_option(name, v)
    # the refused values changed nothing
    x = bytes(range(256)) * 5000  # 1.28 MB
    assert engine.crc32([x]) == [zlib.crc32(x)] and engine.last_checksum_parts() == 20


@pytest.fixture(scope="module")
def text300():
    import zsamd

    return bytes(zsamd.corpus("text", 41, 1, 300 * 1024))


@pytest.mark.parametrize("fmt", ["gzip", "deflate"])
def test_deflate_flushed(small, text300, fmt):
    got = small.compress_batch_detailed([text300], fmt, 1, flush_every=4096)
    assert small.last_checksum_parts() == 300
    small.set_option("checksum_split", 0)
    assert small.compress_batch_detailed([text300], fmt, 1, flush_every=4096) == got
    assert small.last_checksum_parts() == 0
    st, out, check = got[0]
    assert st == 1 and zlib.decompress(out, 31 if fmt == "gzip" else 15) == text300
    assert check == (zlib.crc32(text300) if fmt == "gzip" else zlib.adler32(text300))


@pytest.mark.parametrize("level", [6, 0])
def test_deflate_gzip_unflushed(small, text300, level):
    batch = [text300, text300[:1025], b"", text300[:70001]]
    got = small.compress_batch_detailed(batch, "gzip", level)
    assert small.last_checksum_parts() == parts_of(map(len, batch), PART)
    small.set_option("checksum_split", 0)
    assert small.compress_batch_detailed(batch, "gzip", level) == got and small.last_checksum_parts() == 0
    for x, (st, out, check) in zip(batch, got):
        assert st == 1 and zlib.decompress(out, 31) == x and check == zlib.crc32(x)
    # a raw batch has no data checksum
    small.set_option("checksum_split", 1)
    small.compress_batch([text300], "deflate-raw", level)
    assert small.last_checksum_parts() == 0


@pytest.fixture(scope="module")
def members():
    import zsamd

    text = bytes(zsamd.corpus("text", 42, 1, 200 * 1024 + 13))
    out = {}
    for fmt, wbits in (("gzip", 31), ("deflate", 15)):
        c = zlib.compressobj(6, zlib.DEFLATED, wbits)
        out[fmt] = c.compress(text) + c.flush()
    return text, out


@pytest.mark.parametrize("fmt", ["gzip", "deflate"])
def test_inflate_trailer_check(small, members, fmt):
    text, comp = members
    good = comp[fmt]
    bad = bytearray(good)
    bad[-8 if fmt == "gzip" else -2] ^= 0x10  # a bit of the trailer's crc32 / adler32
    inputs = [good, good, bytes(bad), bytes(bad)]
    caps = [len(text), 4 * len(text)] * 2  # exact; and with empty parts past the decoded length
    got = small.decompress_batch_detailed(inputs, fmt, caps)
    assert small.last_checksum_parts() == parts_of(caps, PART)
    small.set_option("checksum_split", 0)
    assert small.decompress_batch_detailed(inputs, fmt, caps) == got and small.last_checksum_parts() == 0
    want = zlib.crc32(text) if fmt == "gzip" else zlib.adler32(text)
    for st, phase, msg, out, consumed, check in got[:2]:
        assert (st, out, consumed, check) == (1, text, len(good), want)
    for st, phase, msg, out, consumed, check in got[2:]:
        assert st == -3 and "data check" in msg
    assert got[2][:3] == got[3][:3]


def test_pool(engine, text300):
    """the pool's contexts inherit the parts at their default options: streams past 256 KiB"""
    import zsamd

    long = bytes(zsamd.corpus("text", 43, 1, (1 << 20) + 4097))
    batch = [long, text300, b"", long[:1 << 20]]
    want = engine.compress_batch_detailed(batch, "gzip", 6)
    assert engine.last_checksum_parts() == 17 + 5 + 1 + 16
    pool = zsamd.Pool([0, 0], repeat=True)
    try:
        assert pool.compress_batch_detailed(batch, "gzip", 6) == want
        assert pool.compress_batch_detailed(batch, "deflate", 1, flush_every=65536) == \
            engine.compress_batch_detailed(batch, "deflate", 1, flush_every=65536)
    finally:
        pool.close()
    for x, (st, out, check) in zip(batch, want):
        assert st == 1 and zlib.decompress(out, 31) == x and check == zlib.crc32(x)
