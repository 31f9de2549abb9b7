"""GPU parity of zs_k_sweep at the edges of its group walk (deflate_sweep.hip,
SwWave::run8 at levels 5..9, SwWave::run at level 4): the opening group of
steps 1..8, each later group's first and last step, the chain >> 2 snapshots
(steps 4, 8, 32, 64 at levels 4..7), the 64-step blocks and the budgets.

Every stream has ONE hash bucket of exactly k members: k records "abc" + tail,
so the last record's chain is the k - 1 records before it, step t = the t-th
record back.  Tails share 0..2 bytes with the last record's (matches of 3..5
bytes) except where a family places a longer one:

  a  one strictly longer candidate (7 bytes) at step t*,
  b  two equally long ones (7 bytes), in one group or in adjacent groups: the first wins,
  c  long candidates (>= 10 bytes: the whole signature matches), one at a
     group's first or last step, or one on each side of a snapshot (11 bytes
     at step s, 13 at s + 1: the two budgets then differ).

The bytes around the records are filler whose trigrams are all different and
miss the bucket (trigrams that overlap the records' common bytes repeat by
construction).  Each stream is built from 7-bit bytes and again with one byte
>= 0x80, which selects the other signature form.  All of them go in one batch
with a 65,536-byte text stream.  The sweep's match table must equal the chain
walk's (option match_sweep = 0) at every position for both budgets, and the
bytes the oracle's.  test_streams_hit_their_edges checks the construction
itself without a GPU."""
import pytest

import corpus
import oracle

KS = [8, 9, 10, 16, 17, 24, 25, 32, 33, 34, 40, 41, 64, 65, 66, 72, 73, 128, 129, 130, 136, 137, 257]
LEVELS = [4, 5, 6, 7, 9]

MARK = b"abc"
TAIL = b"defghijklmnopqrs"  # the last record's tail; the others share a prefix of it
FILL0, FILLN = 0x20, 64  # filler alphabet 0x20..0x5f: no byte of MARK or TAIL


def _hash(b0, b1, b2):
    return ((b0 << 10) ^ (b1 << 5) ^ b2) & 0x7FFF


HM = _hash(*MARK)


def _filler(n, seed, seen):
    """n filler bytes whose trigrams are new (seen) and hash elsewhere than MARK's"""
    out = bytearray()
    x = seed
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        b = FILL0 + ((x >> 16) % FILLN)
        if len(out) >= 2:
            tri = (out[-2], out[-1], b)
            if tri in seen or _hash(*tri) == HM:
                continue
            seen.add(tri)
        out.append(b)
    return bytes(out)


def build(k, shared, high):
    """A stream whose MARK bucket has k members.  shared: {chain step of the
    last member: tail bytes it shares with that member}, default step % 3.
    Returns (data, position of the last member)."""
    seen = set()
    recs = bytearray()
    c = 0
    for j in range(k):
        t = k - 1 - j
        while True:
            sep = bytes([FILL0 + c % FILLN, FILL0 + c // FILLN])  # a counter: the trigrams through it are new
            c += 1
            r = MARK + (TAIL if t == 0 else TAIL[: shared.get(t, t % 3)]) + sep
            if all(_hash(*r[i : i + 3]) != HM for i in range(1, len(r) - 2)):
                break
        recs += r
    front = bytearray(_filler(max(2048 - len(recs) - 320, 64), 12345 + k, seen))
    if high:
        front[0] = 0xE9
    data = bytes(front) + bytes(recs) + _filler(320, 777 + k, seen)
    return data, len(front) + len(recs) - len(MARK + TAIL) - 2


def _group(k):
    """first and last step of the last whole group of a chain of k - 1 steps"""
    last = 8 * ((k - 1) // 8)
    return (last - 7, last) if last >= 8 else (1, k - 1)


def cases():
    """(family, k, {step: shared tail bytes}, {step: match length expected})"""
    out = []
    for k in KS:
        g0, g1 = _group(k)
        steps = sorted(t for t in {4, 5, 8, 9, 32, 33, 64, 65, g0, g1} if 1 <= t <= k - 1)
        for t in steps:  # a
            out.append(("a", k, {t: 4}, {t: 7}))
        pairs = [(g0, min(g0 + 2, k - 1))]  # b: one group
        if g0 >= 9:
            pairs.append((g0 - 1, g0))  # adjacent groups
        if k - 1 >= 9:
            pairs.append((8, 9))  # the opening group and the next
        for t1, t2 in sorted(set(pairs)):
            out.append(("b", k, {t1: 4, t2: 4}, {t1: 7, t2: 7}))
        for t in sorted({g0, g1}):  # c: a group's first and last step
            out.append(("c", k, {t: 9}, {t: 12}))
        for s in (4, 8, 32, 64):  # c: each side of a snapshot
            if s + 1 <= k - 1:
                out.append(("c", k, {s: 8, s + 1: 10}, {s: 11, s + 1: 13}))
    return out


@pytest.fixture(scope="module")
def streams():
    out = []
    for fam, k, shared, want in cases():
        for high in (False, True):
            data, p = build(k, shared, high)
            out.append((fam, k, want, high, data, p))
    return out


def test_streams_hit_their_edges(streams):
    """No GPU: each stream's bucket has exactly k members, and the last member's
    chain has the intended match lengths at the intended steps, 3..5 elsewhere."""
    assert {k for _, k, _, _, _, _ in streams} == set(KS)
    assert {f for f, _, _, _, _, _ in streams} == {"a", "b", "c"}
    for fam, k, want, high, d, p in streams:
        assert 2048 <= len(d) <= 8192, (fam, k, len(d))
        assert (max(d) >= 0x80) == high
        members = [i for i in range(len(d) - 2) if _hash(d[i], d[i + 1], d[i + 2]) == HM]
        assert len(members) == k and members[-1] == p, (fam, k, want, len(members))
        assert all(d[m : m + 3] == MARK for m in members)
        for t in range(1, k):
            q = members[k - 1 - t]
            n = 0
            while d[q + n] == d[p + n]:
                n += 1
            assert n == want.get(t, 3 + t % 3), (fam, k, want, t, n)
        if fam == "a":
            assert list(want.values()) == [7]
        if fam == "b":
            t1, t2 = sorted(want)
            assert want[t1] == want[t2] == 7 and ((t1 - 1) // 8 == (t2 - 1) // 8 or (t2 - 1) // 8 - (t1 - 1) // 8 == 1)
        if fam == "c":
            assert all(n >= 11 for n in want.values())


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_sweep_groups_match_table_equals_chain_walk(engine, streams, level):
    inputs = [s[4] for s in streams] + [corpus.text(4711, 65536)]
    tables, outs = [], []
    try:
        for sweep in (1, 0):
            engine.set_option("match_sweep", sweep)
            outs.append(engine.compress_batch_raw(inputs, "deflate-raw", level))
            tables.append([engine.debug_fetch(1, i, 8 * len(d)) for i, d in enumerate(inputs)])
    finally:
        engine.set_option("match_sweep", 1)
    for i, d in enumerate(inputs):
        tag = streams[i][:4] if i < len(streams) else "text"
        assert len(tables[0][i]) == 8 * len(d), (tag, len(d))
        assert tables[0][i] == tables[1][i], (tag, len(d))
        want = oracle.compress(d, level, "deflate-raw")[1]
        assert outs[0][i] == outs[1][i] and outs[0][i] == (1, want), (tag, len(d))
