"""Deterministic inputs that drive a deflate encoder's tree builder into its
rare branches (trees.ts:187-259: lengths over max_length and the overflow
repair; :305-316 with fewer than two used codes; :318-414 the run-length
header at its chunk limits).  Seeded, no files; tests/test_huffman_cases.py pins
on the oracle what each input reaches, tests/test_gpu_huffman.py runs them on
the GPU.

The skewed inputs start with 32 KiB of R-corpus bytes (no matches: they leave
as stored blocks) and go on with back-to-back copies of earlier bytes, each
with a chosen length and a chosen distance code.  A copy's source is a stretch
no earlier copy used, so its nearest occurrence is the intended one, and its
first byte differs from the byte after the previous copy's source, so the
previous match does not grow by chance.  The number of copies per code follows
chain(): ascending counts g with g[k+2] > slack * sum(g[:k+1]) + add, for which
the Huffman tree is a path -- its depth the number of codes less one -- with
room for the counts an encoder's parse shifts.  A copy that finds no unused
source in its code's range is left out (DROPPED counts them; up to a tenth of
the copies of the largest inputs): what an input reaches is what the oracle's
output shows, pinned case by case in tests/test_huffman_cases.py."""
import random

import corpus
from deflate_header import DBASE, DEXT, LBASE, LEXT

MAX_DIST = 32768 - 262  # deflate.ts MAX_DIST(s)
DROPPED = [0]  # copies left out so far for want of an unused source (the generators' own check)


def chain(n, slack=1.03, add=2, first=(1, 1)):
    """n ascending counts whose Huffman tree is a path."""
    g = list(first)
    while len(g) < n:
        g.append(int(slack * sum(g[:-1]) + add) + 1)
    return g[:n]


def len_of_code(c):
    """The shortest length that length code 257 + c stands for."""
    return LBASE[c]


def _copies(seed, plan, literals=b""):
    """32 KiB of R-corpus bytes, `literals`, then the copies of plan [(length, distance code)] in order.
    Returns (bytes, copies dropped for want of an unused source)."""
    rng = random.Random(seed)
    data = bytearray(corpus.rand(corpus.stream_seed(seed), 32768))
    data += literals
    used = bytearray(len(data))
    avoid, dropped = -1, 0
    for n, dc in plan:
        pos = len(data)
        if dc is None:  # any distance: a source may serve again (the encoder takes its nearest occurrence)
            lo, hi = n, min(MAX_DIST, pos)
        else:
            lo, hi = DBASE[dc], min(DBASE[dc] + (1 << DEXT[dc]) - 1, MAX_DIST, pos)
        a = -1
        if hi >= lo and (lo < n or dc is None):  # (a distance under the length: the copy repeats its own bytes)
            while a < 0 or data[a] == avoid:
                a = pos - rng.randrange(lo, hi + 1)
        elif hi >= lo:
            # the first unused stretch of n bytes from a random point of the code's range on, then from its start
            first, last = pos - hi, pos - lo  # source starts
            k = rng.randrange(first, last + 1)
            for s, e in ((k, last + n), (first, min(k + n, last + n))):
                while a < 0:
                    s = used.find(bytes(n), s, min(e, pos))
                    if s < 0:
                        break
                    if data[s] != avoid:
                        a = s
                    s += 1
        if a < 0:
            dropped += 1
            DROPPED[0] += 1
            continue
        for i in range(n):  # (byte by byte: a distance under the length repeats the copy's own bytes)
            data.append(data[a + i])
        used.extend(bytes(n))
        used[a:min(a + n, pos)] = b"\x01" * (min(a + n, pos) - a)
        avoid = data[a + n]
    return bytes(data), dropped


def _plan(seed, triples):
    plan = [(n, dc) for n, dc, count in triples for _ in range(count)]
    random.Random(seed ^ 0x5bd1e995).shuffle(plan)
    return plan


def dist_codes(n):
    """n distance codes, 29 downward, in ascending order of their range: the largest counts of a chain go to
    the codes with the widest choice of sources."""
    return list(range(30 - n, 30))


def skewed_matches(seed, len_counts, dist_counts):
    """len_counts [(length, count)] and dist_counts [(distance code, count)] with equal totals: every copy takes
    one length and one distance code, paired at random."""
    rng = random.Random(seed ^ 0x27d4eb2f)
    ls = [n for n, c in len_counts for _ in range(c)]
    ds = [d for d, c in dist_counts for _ in range(c)]
    assert len(ls) == len(ds)
    rng.shuffle(ls)
    rng.shuffle(ds)
    return _copies(seed, list(zip(ls, ds)))[0]


def skewed_dist(seed, ncodes, length=4, slack=1.03, add=2):
    """The distance tree a path of ncodes codes (29 downward), every copy `length` bytes long."""
    g = chain(ncodes, slack, add)
    return skewed_matches(seed, [(length, sum(g))], list(zip(dist_codes(ncodes), g)))


def skewed_len(seed, ncodes, slack=1.03, add=2):
    """The literal/length tree a path of ncodes length codes (258 upward: lengths 4, 5, ...), the rarest the
    longest; any distance."""
    g = chain(ncodes, slack, add)
    lens = [(len_of_code(1 + k), c) for k, c in zip(range(ncodes - 1, -1, -1), g)]
    return skewed_matches(seed, lens, [(None, sum(g))])


def paired(seed, triples):
    """[(length, distance code, count)]: both trees skewed at once, the k-th length tied to the k-th code."""
    return _copies(seed, _plan(seed, triples))[0]


def paired_chain(seed, ncodes, top_len=131, top_dist=29, slack=1.03, add=2):
    """paired() with one chain of counts for both trees: the rarest pair is (top_len, top_dist) -- 5 and 13 extra
    bits --, the others lengths 4, 5, ... with distance codes 30 - ncodes .. 28 less top_dist, most copies on the
    widest."""
    g = chain(ncodes, slack, add)
    dcs = [d for d in range(30 - ncodes, 30) if d != top_dist][-(ncodes - 1):]
    triples = [(top_len, top_dist, g[0])]
    for k in range(1, ncodes):
        triples.append((len_of_code(ncodes - k), dcs[k - 1], g[k]))
    return paired(seed, triples)


def debruijn(k, seed=1, alphabet=None):
    """A de Bruijn sequence of order 3 over k byte values (random ones, or `alphabet`) plus its first two bytes:
    every trigram once, so no match at any level; every value k * k times (the first two once more)."""
    if alphabet is None:
        alphabet = random.Random(seed * 1000 + k).sample(range(256), k)
    assert len(alphabet) == k
    n = 3
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    seq += seq[:2]
    return bytes(alphabet[i] for i in seq)


def every_code(seed):
    """All 256 literals, all 29 length codes and all 30 distance codes in one block (HLIT 286, HDIST 30): the
    literals twice in two orders, every length code with every distance code it can take, and 2,500 short
    copies so that the block is worth a dynamic header."""
    rng = random.Random(seed)
    lits = bytearray()
    for _ in range(2):
        p = list(range(256))
        rng.shuffle(p)
        lits += bytes(p)
    short = [(rng.choice([4, 5, 6]), rng.choice([24, 25, 26, 27, 28, 29])) for _ in range(2500)]
    plan = []
    for i in range(60):  # (first, while long unused stretches are plentiful; short copies between them, so that
        # the near distance codes find fresh bytes)
        plan.append((258 if i % 29 == 28 else LBASE[i % 29] + rng.randrange(1 << LEXT[i % 29]), i % 30))
        plan += [short.pop() for _ in range(4)]
    return _copies(seed, plan + short, bytes(lits))[0]


def header_runs(groups):
    """Literal-only input whose used byte values lie in `groups` [(first value, count)]: one de Bruijn sequence
    over all of them, so every value has the same frequency and -- with a power of two of them -- the same code
    length but for the one that pairs with the end of block; the unused values between the groups are runs of
    zero lengths of chosen size, the groups runs of equal lengths."""
    alphabet = [v + i for v, c in groups for i in range(c)]
    return debruijn(len(alphabet), alphabet=alphabet)


# 16 values each (4,098 bytes).  The oracle gives the 8th used value the odd length (it pairs with the end of
# block), so that value stands alone and the groups around it keep one length: zero runs of 3, 10, 11, 138 and 139
# and runs of 3, 6, 7 and 8 equal lengths; RUNS[4] takes two sequences (2 x 16 values): runs of 15, 9 and 7
RUNS = [
    [(0, 7), (10, 1), (21, 8)],
    [(0, 3), (14, 4), (30, 1), (40, 6), (50, 2)],
    [(0, 7), (145, 1), (150, 8)],
    [(0, 7), (146, 1), (150, 8)],
]
RUNS_TWO = ([(0, 16)], [(30, 9), (50, 7)])


def small_cases():
    """(name, bytes) of the odds and ends: inputs of a few bytes to 64 KiB around the tree builder's
    smallest cases and the header's run limits."""
    return [
        ("one_literal", b"a"),
        ("one_literal_twice", b"aa"),
        ("literal_and_match", b"a" * 259),
        ("one_match", b"abc" * 2),
        ("two_values", debruijn(2)),
    ] + [("runs_%d" % i, header_runs(g)) for i, g in enumerate(RUNS)] + [
        ("runs_4", header_runs(RUNS_TWO[0]) + header_runs(RUNS_TWO[1])),
    ]
