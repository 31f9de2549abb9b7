"""CPU check of the Z_RLE arithmetic (csrc/zs_rle.h, the closed form zs_k_rle_tally
evaluates per position; host build tools/emu/emu_rle.cpp, plain g++).

Part 1: its symbols and block cuts against a sequential restatement of zlib 1.2.11's
deflate_rle loop, written below.  Part 2: against zlib itself -- the symbols, coded with
the fixed trees (bitbuild), inflate to the input, and they are the symbols of zlib's own
Z_RLE stream (read back with deflate_header; zlib cannot combine Z_FIXED with Z_RLE, so
its dynamic blocks are parsed).  The derivation of the closed form came from reading
deflate.c, not from a run: these tests are what confirm it."""
import random
import shutil
import subprocess
import zlib

import pytest

import bitbuild
import deflate_header
import strategycases as cases

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "emu", "emu_rle.cpp")
MAX_MATCH, MIN_MATCH = 258, 3


def deflate_rle(data):
    """zlib's deflate_rle (deflate.c 1.2.11), one symbol per iteration: [(position, length)], length 1 = a
    literal.  lookahead exceeds MAX_MATCH whenever input remains, so only the end of the input shortens a match."""
    n, p, out = len(data), 0, []
    while p < n:
        length = 0
        if n - p >= MIN_MATCH and p > 0:
            prev, scan = data[p - 1], p
            if prev == data[scan] and prev == data[scan + 1] and prev == data[scan + 2]:
                strend = p + MAX_MATCH
                scan += 2
                while True:  # (the unrolled scan of eight compares stops at the first difference or at strend)
                    scan += 1
                    if not (scan < strend and scan < n and data[scan] == prev):
                        break
                length = min(MAX_MATCH - (strend - scan), n - p)
        if length >= MIN_MATCH:
            out.append((p, length))
            p += length
        else:
            out.append((p, 1))
            p += 1
    return out


def blocks_of(symbols, n):
    """(sym_start, sym_count, in_start, in_end, last): a block closes after every 16,383rd symbol, the last one
    is final and may be empty"""
    out, nflush = [], len(symbols) // cases.SYM_END
    for b in range(nflush + 1):
        end = lambda g: symbols[g][0] + symbols[g][1]
        out.append((b * cases.SYM_END, cases.SYM_END if b < nflush else len(symbols) - nflush * cases.SYM_END,
                    0 if b == 0 else end(b * cases.SYM_END - 1), end((b + 1) * cases.SYM_END - 1) if b < nflush else n,
                    1 if b == nflush else 0))
    return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("emu_rle")
    exe = str(tmp / "emu_rle")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, SRC], check=True)

    def run(data):
        path = str(tmp / "in.bin")
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        syms, blocks = [], []
        for line in r.stdout.splitlines():
            f = line.split()
            if f[0] == "s":
                syms.append(int(f[1], 16))
            else:
                blocks.append(tuple(int(x) for x in f[1:]))
        return syms, blocks

    return run


def as_words(data, symbols):
    return [data[p] if n == 1 else 0x80000000 | (n - 3) << 16 | 1 for p, n in symbols]


def random_inputs():
    rng = random.Random(20240)
    out = [bytes(rng.choice(b"ab") for _ in range(n)) for n in (1, 2, 3, 4, 7, 300, 5000, 40000)]
    # runs of the listed lengths in random order, other bytes between some of them
    for _ in range(4):
        parts = []
        for L in rng.sample(cases.RUN_LENS * 3, len(cases.RUN_LENS) * 3):
            parts.append((rng.choice(b"ab") if not parts or isinstance(parts[-1], bytes) else 99 - (parts[-1][0] == 99), L))
            if rng.random() < 0.5:
                parts.append(b"-")
        out.append(cases.runs(*parts))
    return out


def inputs():
    return [x for _, x in cases.rle_inputs()] + random_inputs() + [b""]


def test_the_closed_form_is_the_sequential_loop(emu):
    for x in inputs():
        want = deflate_rle(x)
        syms, blocks = emu(x)
        assert syms == as_words(x, want), (len(x), x[:40])
        assert blocks == blocks_of(want, len(x)), (len(x), x[:40])


def test_block_cuts_fall_inside_and_around_a_run(emu):
    # the cases built for it: the 16,383rd symbol is a literal before the run, its first byte, one of its matches
    kinds = set()
    for name, x in cases.rle_inputs():
        if not name.startswith("cut"):
            continue
        want = deflate_rle(x)
        assert len(want) > cases.SYM_END
        kinds.add((want[cases.SYM_END - 1][1], want[cases.SYM_END][1]))
        assert emu(x)[1][0][3] == sum(n for _, n in want[:cases.SYM_END])
    assert {(1, 258), (258, 258), (258, 83), (83, 1), (1, 1)} <= kinds, kinds


def test_the_symbols_are_zlibs(emu):
    for x in inputs():
        syms, _ = emu(x)
        symbols = [("lit", v) if v < 256 else ("copy", ((v >> 16) & 0xff) + 3, v & 0xffff) for v in syms]
        # coded with the fixed trees they inflate to the input ...
        assert zlib.decompress(bitbuild.build(symbols, d64=False), -15) == x
        # ... and they are what zlib's own Z_RLE stream holds
        z = deflate_header.parse(cases.compress(x, 6, "deflate-raw", cases.Z_RLE))
        assert all(b.type != 0 for b in z)
        assert [s for b in z for s in b.symbols] == symbols, (len(x), x[:40])
        assert [len(b.symbols) for b in z] == [c for _, c, _, _, _ in blocks_of(deflate_rle(x), len(x))]
