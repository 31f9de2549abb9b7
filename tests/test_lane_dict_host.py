"""The dictionary instances of the lane-per-member inflate kernel
(zs_k_inflate_lane<., false, true>, csrc/inflate_lane.hip) run on the CPU from the
kernel's own source (tools/lane_dict_host), checked against the system
zlib's decompressobj(wbits, zdict): bytes, consumed count and the wanted check
value of every member, for raw deflate and zlib, and clean members must not
bail.  Hand-built members (bitbuild) put copies on the dictionary / output
boundary.  The same program runs once more built with AddressSanitizer and
UBSan (a stand-alone program: the kernel's dictionary reads stay inside the
dictionary's words)."""
import os
import struct
import subprocess
import zlib

import pytest

import dictcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tools", "lane_dict_host")


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-s", "-C", HOST, "lane_dict_host"])
    return os.path.join(HOST, "lane_dict_host")


def run(exe, members, fmt, flags=1):
    """members: [(compressed, cap, dictionary)] -> [(bail, out_len, consumed, want, bytes)]"""
    data = struct.pack("<I", len(members)) + b"".join(
        struct.pack("<III", len(c), cap, len(d)) + c + d for c, cap, d in members)
    out = subprocess.run([exe, str(dictcases.W[fmt]), str(flags)], input=data, capture_output=True, check=True).stdout
    res, p = [], 0
    for _ in members:
        bail, olen, cons, want = struct.unpack_from("<4I", out, p)
        p += 16
        n = 0 if bail else olen
        res.append((bail, olen, cons, want, out[p:p + n]))
        p += n
    assert p == len(out)
    return res


def check_clean(exe, L, fmt, flags):
    d = dictcases.dictionary(L)
    ms = dictcases.members(L, fmt)
    res = run(exe, [(c, dictcases.cap4(len(s)), d) for c, s in ms], fmt, flags)
    for i, ((c, s), (bail, olen, cons, want, out)) in enumerate(zip(ms, res)):
        ref, rcons = dictcases.inflate_ref(c, fmt, d)
        assert ref == s
        assert not bail, (L, fmt, i)
        assert (out, olen, cons) == (s, len(s), rcons), (L, fmt, i)
        if fmt == "deflate":  # the trailer's adler32: of the output only (the check restarts after DICTID)
            assert want == zlib.adler32(s), (L, fmt, i)


@pytest.mark.parametrize("fmt", ["deflate-raw", "deflate"])
@pytest.mark.parametrize("L", dictcases.DICT_LENS)
def test_dictionary_members_decode_on_the_lane(host, L, fmt):
    check_clean(host, L, fmt, 1)


def test_zlib_members_compressed_against_the_dictionary_carry_fdict():
    for L in dictcases.DICT_LENS:
        c = dictcases.members(L, "deflate")[5][0]
        assert c[1] & 0x20 and struct.unpack(">I", c[2:6])[0] == zlib.adler32(dictcases.dictionary(L))


@pytest.mark.parametrize("L", dictcases.DICT_LENS)
def test_hand_built_copies_on_the_boundary(host, L):
    d = dictcases.dictionary(L)
    cases = dictcases.hand_built(L)
    names = sorted(cases)
    res = run(host, [(cases[k][0], dictcases.cap4(len(cases[k][1] or b"") + 8), d) for k in names], "deflate-raw")
    for k, (bail, olen, cons, want, out) in zip(names, res):
        m, exp = cases[k]
        if exp is None:
            assert bail, (L, k)  # distance dl + 1: the exact kernel reports "invalid distance too far back"
        else:
            assert not bail and out == exp and cons == len(m), (L, k)


def test_lane_leaves_these_to_the_exact_kernel(host):
    """wrong dictionary, FDICT without a dictionary, members past one inflate() call;
    an FDICT-clear member ignores its dictionary"""
    d, other = dictcases.dictionary(257), dictcases.dictionary(257, seed=901)
    s = dictcases.record(9)
    z = dictcases.compress(s, 6, "deflate", d)
    plain = dictcases.compress(s, 6, "deflate")
    cap = dictcases.cap4(len(s))
    res = run(host, [(z, cap, other), (z, cap, b""), (z, 65540, d), (plain, cap, d), (z, cap, d), (z, cap - 4, d)],
              "deflate")
    assert [r[0] for r in res] == [1, 1, 1, 0, 0, 1]
    assert res[3][4] == s and res[4][4] == s
    # raw: a member of more than 32 KiB of input takes the exact kernel
    import corpus
    big = corpus.rand(5, 40000)
    c = dictcases.compress(big, 1, "deflate-raw", d)
    assert len(c) > 32768
    assert run(host, [(c, 65536, d)], "deflate-raw")[0][0] == 1


def test_sanitized_build_of_the_dictionary_lane():
    """AddressSanitizer + UBSan over the same program (stand-alone, nothing preloaded):
    the dictionary's buffer ends with the word of its last byte, so a word read past
    it would be reported"""
    subprocess.check_call(["make", "-s", "-C", HOST, "lane_dict_host_san"])
    exe = os.path.join(HOST, "lane_dict_host_san")
    for L in (1, 3, 257, 32767, 40000):
        check_clean(exe, L, "deflate", 1)
        d = dictcases.dictionary(L)
        cases = dictcases.hand_built(L)
        run(exe, [(m, dictcases.cap4(len(exp or b"") + 8), d) for m, exp in cases.values()], "deflate-raw")
