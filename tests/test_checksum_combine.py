"""zs_crc32_combine / zs_adler32_combine (host arithmetic of libzsgpu.so, no GPU) against Python's
zlib: the checksum of A + B from the pieces' checksums and len(B), through ctypes and through
the Python wrappers."""
import ctypes
import random
import zlib

import pytest

LENS = [0, 1, 2, 5551, 5552, 5553, 65521, 70000]


@pytest.fixture(scope="module")
def pieces():
    rng = random.Random(20)
    return {n: [rng.randbytes(n), rng.randbytes(n)] for n in LENS}


def c_entries():
    import zsamd

    L = zsamd.lib()
    return (lambda a, b, n: L.zs_crc32_combine(ctypes.c_uint32(a), ctypes.c_uint32(b), ctypes.c_uint64(n)),
            lambda a, b, n: L.zs_adler32_combine(ctypes.c_uint32(a), ctypes.c_uint32(b), ctypes.c_uint64(n)))


def py_entries():
    import zsamd

    return zsamd.crc32_combine, zsamd.adler32_combine


@pytest.mark.parametrize("entries", [c_entries, py_entries], ids=["ctypes", "python"])
def test_combine_is_the_checksum_of_the_joined_buffers(entries, pieces):
    crc_c, adl_c = entries()
    for na in LENS:
        for nb in LENS:
            a, b = pieces[na][0], pieces[nb][1]
            assert crc_c(zlib.crc32(a), zlib.crc32(b), nb) == zlib.crc32(a + b), (na, nb)
            assert adl_c(zlib.adler32(a), zlib.adler32(b), nb) == zlib.adler32(a + b), (na, nb)
    # a second piece without bytes: the first value, whatever the second argument
    assert crc_c(0x12345678, 0xdeadbeef, 0) == 0x12345678
    assert adl_c(0x12345678, 0x00010001, 0) == 0x12345678


@pytest.mark.parametrize("entries", [c_entries, py_entries], ids=["ctypes", "python"])
def test_combine_is_associative_past_4_gib(entries):
    crc_c, adl_c = entries()
    rng = random.Random(21)
    for lb, lc in [((1 << 32) - 5, 70000), (3 << 31, (1 << 33) + 12345), (1, 1 << 32), (65521 << 16, (1 << 32) - 1)]:
        assert lb + lc > 1 << 32
        for _ in range(4):
            a, b, c = (rng.randrange(1 << 32) for _ in range(3))
            assert crc_c(crc_c(a, b, lb), c, lc) == crc_c(a, crc_c(b, c, lc), lb + lc), (lb, lc)
            # adler32: reduced values, both halves below 65521
            a, b, c = ((rng.randrange(65521) << 16) | rng.randrange(65521) for _ in range(3))
            assert adl_c(adl_c(a, b, lb), c, lc) == adl_c(a, adl_c(b, c, lc), lb + lc), (lb, lc)
    # ... and agrees with a length that zlib can check: 2^32 + 3 zero bytes behind a piece, in two steps
    z = bytes(1 << 16)
    crc_z, adl_z, n = zlib.crc32(z), zlib.adler32(z), 1 << 16
    while n < (1 << 32):  # doubling: the checksums of 2^32 zero bytes
        crc_z, adl_z, n = crc_c(crc_z, crc_z, n), adl_c(adl_z, adl_z, n), 2 * n
    head = b"zs_gpu"
    want_crc = crc_c(crc_c(zlib.crc32(head), crc_z, n), zlib.crc32(bytes(3)), 3)
    assert crc_c(zlib.crc32(head), crc_c(crc_z, zlib.crc32(bytes(3)), 3), n + 3) == want_crc
    want_adl = adl_c(adl_c(zlib.adler32(head), adl_z, n), zlib.adler32(bytes(3)), 3)
    assert adl_c(zlib.adler32(head), adl_c(adl_z, zlib.adler32(bytes(3)), 3), n + 3) == want_adl
    # zero bytes leave adler32's low half alone and add len * A to the high half
    a0 = zlib.adler32(head) & 0xffff
    assert want_adl == ((((zlib.adler32(head) >> 16) + (n + 3) * a0) % 65521) << 16) | a0
