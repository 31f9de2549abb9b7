"""GPU parity of zs_k_sweep's long-candidate paths (deflate_sweep.hip, fold): a
candidate whose whole signature matches -- 10 bytes in the 7-bit form, 11 in
the 11-byte form -- is measured from the window; a lane's first long candidate
of a group is named by the group's maximum score, further ones of the same lane
in the same group are visited one by one.

One batch of small constructed streams in which occurrences of one trigram are
laid out so that a chosen position meets candidates of chosen lengths at chosen
chain steps.  A byte-wise model of the chains (below) first asserts that every
case the streams were built for really occurs at the level under test; then
the sweep's match table must equal the chain walk's (option match_sweep = 0) at
every position for both budgets, and the output the oracle's."""
import struct

import pytest

import corpus
import oracle

CHAIN = {4: 16, 5: 32, 6: 128, 7: 256, 9: 4096}  # max_chain_length, deflate.ts configuration_table
NICE = {4: 16, 5: 32, 6: 128, 7: 128, 9: 258}
T = b"q#Z"  # the trigram of every occurrence
S = 3  # a candidate sharing the trigram only


def _r7(seed, n):
    return bytes(x & 0x7F for x in corpus.rand(seed, n))


def _probe(seed, n=64):
    """A string starting with the trigram whose later bytes avoid the trigram's first byte."""
    return T + bytes(b if b != T[0] else 0x41 for b in _r7(seed, n - 3))


def _occ(P, lcp, seed):
    """An occurrence sharing exactly `lcp` bytes with P, then two bytes of filler."""
    f = bytes(b if b != T[0] else 0x42 for b in _r7(seed, 2))
    return P[:lcp] + bytes([P[lcp] ^ 1]) + f


def _steps(seed, lcps, P=None, cut=None):
    """A stream whose last occurrence P meets, at chain step t, a candidate sharing lcps[t - 1] bytes;
    cut: the stream ends `cut` bytes after P's start."""
    P = P or _probe(seed)
    out = [_r7(seed + 1, 40).replace(T[:1], b"A")]
    for i, l in enumerate(reversed(lcps)):
        out.append(_occ(P, l, seed + 2 + i))
    out.append(P if cut is None else P[:cut])
    return b"".join(out)


def _at(n, **steps):
    """lcps of n steps, S except the given ones (t5=13 -> step 5 shares 13 bytes)."""
    l = [S] * n
    for k, v in steps.items():
        l[int(k[1:]) - 1] = v
    return l


def _streams():
    s = {}
    s["one"] = _steps(100, _at(8, t7=13))
    s["two"] = _steps(200, _at(8, t6=12, t8=14))
    s["three"] = _steps(300, _at(8, t5=14, t7=13, t8=17))
    s["eight"] = _steps(400, _at(24, **{"t%d" % t: 11 + (t * 3) % 5 for t in range(5, 25)}))
    # two lanes of one chunk, one long candidate each at different steps of one group: X meets its copy at
    # step 7, Y its own at step 5
    X, Y = _probe(500), None
    Y = X[:5] + bytes([X[5] ^ 1]) + _probe(501)[6:]
    s["lanes"] = b"".join([_r7(502, 40).replace(T[:1], b"A"), _occ(X, 13, 503), _occ(Y, 13, 504)] +
                          [_occ(X, S, 505 + i) for i in range(4)] + [Y[:40], b"AB", X])
    # the head, steps 2..8, a group's last step and the next group's first (12 | 13 at level 4, 8 | 9 above)
    s["places"] = _steps(600, _at(17, t1=11, t3=12, t8=13, t9=14, t12=15, t13=17, t16=18, t17=19))
    # steps chain >> 2 and chain >> 2 + 1 of every level, the later one longer
    s["budgets"] = _steps(700, _at(1025, t4=11, t5=12, t8=13, t9=14, t32=15, t33=18, t64=19, t65=20, t1024=21,
                                   t1025=22))
    # 10: long in the 7-bit form only; 13: the record's extension bytes settle it; 14: the extension loop is
    # entered; 17, 18, 22: its first and second rounds in either form
    s["lengths"] = _steps(800, _at(16, t2=10, t3=13, t4=14, t6=17, t7=18, t10=22, t14=23))
    # nice - 1, nice, above nice in that order (levels 4 and 5), from step 2 and from step 4
    for lv in (4, 5):
        nc = NICE[lv]
        s["nice%d" % lv] = _steps(900 + lv, _at(8, t2=nc - 1, t3=nc, t4=40), P=_probe(900 + lv, 80))
        s["nice%db" % lv] = _steps(910 + lv, _at(8, t4=nc - 1, t5=nc, t6=40), P=_probe(910 + lv, 80))
    for cut in range(13, 21):  # the stream ends maxc bytes after the position
        s["end%d" % cut] = _steps(1000 + cut, _at(6, t2=30, t5=31), cut=cut)
    for k in list(s):  # the same with one byte >= 0x80: the 11-byte signature form
        s[k + "+hi"] = b"\xe9" + s[k]
    return s


def _groups(chain):
    """The sweep's groups of steps (first, last): steps 1..8 as one group where chain >> 2 >= 8, else the head and
    2..4; then eights (a four where fewer are left) cut at chain >> 2 and at 64-step blocks."""
    bs = chain >> 2
    g, first = ([(1, 8)], 9) if bs >= 8 else ([(1, 1), (2, 4)], 5)
    b = 0
    while chain > 4:
        t0, tb = (first if b == 0 else 64 * b + 1), min(64 * b + 64, chain)
        while t0 <= tb:
            t1 = t0 + 7 if t0 + 7 <= tb else t0 + 3
            if t0 <= bs < t1:
                t1 = bs
            g.append((t0, t1))
            t0 = t1 + 1
        if tb >= chain:
            break
        b += 1
    return g


def _lcp(d, p, q, maxc):
    k = 0
    while k < maxc and d[p + k] == d[q + k]:
        k += 1
    return k


def _model(d):
    """Per position with a candidate of >= 10 bytes: (p, member index, maxc, [(q, lcp) by chain step])."""
    n = len(d)
    buckets = {}
    for p in range(n - 2):
        h = ((d[p] << 10) ^ (d[p + 1] << 5) ^ d[p + 2]) & 0x7FFF
        buckets.setdefault(h, []).append(p)
    lanes, k0 = [], 0
    for h in sorted(buckets):
        ps = buckets[h]
        for i, p in enumerate(ps):
            maxc = min(258, n - p)
            c = [(q, _lcp(d, p, q, maxc)) for q in reversed(ps[max(0, i - 4096):i])]
            if any(l >= 10 for _, l in c):
                lanes.append((p, k0 + i, maxc, c))
        k0 += len(ps)
    return {"a7": max(d) < 0x80, "lanes": lanes}


def _best(c, budget, nice, maxc):
    """longest_match over the first `budget` candidates (deflate.ts:1082-1105): (length, candidate)."""
    bl, bq = 2, None
    for q, l in c[:budget]:
        if l > bl:
            bl, bq = l, q
            if l >= min(nice, maxc):
                break
    return bl, bq


@pytest.fixture(scope="module")
def streams():
    s = _streams()
    assert all(len(d) <= 8192 for d in s.values()), max(len(d) for d in s.values())
    return s


@pytest.fixture(scope="module")
def models(streams):
    return {k: _model(d) for k, d in streams.items()}


def _long_by_group(m, level):
    """(lane, group, [(step, lcp)]) for every swept lane and group holding long candidates."""
    lt = 10 if m["a7"] else 11
    out = []
    for lane in m["lanes"]:
        p, k, maxc, c = lane
        if maxc <= 12:  # the stream's last positions are walked exactly, not swept
            continue
        for t0, t1 in _groups(CHAIN[level]):
            if t0 > len(c):
                break
            lg = [(t, c[t - 1][1]) for t in range(t0, min(t1, len(c)) + 1) if c[t - 1][1] >= lt]
            if lg:
                out.append((lane, (t0, t1), lg))
    return out


@pytest.mark.parametrize("level", [4, 5, 6, 7, 9])
def test_constructed_cases_occur(streams, models, level):
    """The model finds every case the streams were built for, in both signature forms (no GPU needed)."""
    chain, nice = CHAIN[level], NICE[level]
    for hi in ("", "+hi"):
        L = {k: _long_by_group(models[k + hi], level) for k in streams if not k.endswith("+hi")}
        assert models["one" + hi]["a7"] == (hi == "")
        # exactly 1, 2, 3 and 8 long candidates of one lane inside one group
        for name, cnt in (("one", 1), ("two", 2), ("three", 3), ("eight", 8)):
            assert any(len(lg) == cnt for _, _, lg in L[name]), (name, hi)
        # two lanes of one chunk, one long candidate each, at different steps of one group
        single = [(lane[1] // 64, g, lg[0][0]) for lane, g, lg in L["lanes"] if len(lg) == 1]
        assert any(a[:2] == b[:2] and a[2] != b[2] for a in single for b in single), hi
        # the head, steps 2..8, a group's last step and the next group's first
        pl = L["places"]
        assert any(t == 1 for _, _, lg in pl for t, _ in lg) and any(2 <= t <= 8 for _, _, lg in pl for t, _ in lg), hi
        ends = {(lane[0], g[1]) for lane, g, lg in pl if lg[-1][0] == g[1]}
        assert any((lane[0], g[0] - 1) in ends for lane, g, lg in pl if lg[0][0] == g[0]), hi
        # steps chain >> 2 and chain >> 2 + 1, the later longer: the budgets' results differ
        bs = chain >> 2
        lane = max(models["budgets" + hi]["lanes"], key=lambda x: len(x[3]))
        c = lane[3]
        assert len(c) >= 1025 and c[bs][1] > c[bs - 1][1] >= 11, hi
        assert _best(c, chain, nice, lane[2]) != _best(c, bs, nice, lane[2]), hi
        assert _best(c, bs, nice, lane[2])[1] == c[bs - 1][0], hi
        # candidates of exactly 13, 14 and 17 bytes (and 18, 22: the extension loop's second round)
        got = {l for _, _, lg in L["lengths"] for _, l in lg}
        assert {13, 14, 17, 18, 22} <= got, (sorted(got), hi)
        assert (10 in got) == (hi == ""), hi
        # nice - 1, nice and above nice in chain order on one lane
        if level in (4, 5):
            for name in ("nice%d" % level, "nice%db" % level):
                seq = {}
                for lane, _, lg in L[name]:
                    seq.setdefault(lane[0], []).extend(l for _, l in lg)
                assert any(q[:3] == [nice - 1, nice, 40] for q in seq.values()), (name, seq, hi)
        # stream ends: a swept lane with maxc = 13..20 and a long candidate
        for cut in range(13, 21):
            assert any(lane[2] == cut for lane, _, _ in L["end%d" % cut]), (cut, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [4, 5, 6, 7, 9])
def test_sweep_long_match_table_equals_chain_walk(engine, streams, models, level):
    names = sorted(streams)
    inputs = [streams[k] for k in names]
    tables, outs = [], []
    try:
        for sweep in (1, 0):
            engine.set_option("match_sweep", sweep)
            outs.append(engine.compress_batch_raw(inputs, "deflate-raw", level))
            tables.append([engine.debug_fetch(1, i, 8 * len(d)) for i, d in enumerate(inputs)])
    finally:
        engine.set_option("match_sweep", 1)
    for i, d in enumerate(inputs):
        assert len(tables[0][i]) == 8 * len(d), (names[i], len(d))
        assert tables[0][i] == tables[1][i], names[i]
        want = oracle.compress(d, level, "deflate-raw")[1]
        assert outs[0][i] == outs[1][i] and outs[0][i] == (1, want), names[i]
    # the two budgets at the position built for them: the short one stops at step chain >> 2
    chain, nice = CHAIN[level], NICE[level]
    for name in ("budgets", "budgets+hi"):
        p, _, maxc, c = max(models[name]["lanes"], key=lambda x: len(x[3]))
        rx, ry = struct.unpack_from("<II", tables[0][names.index(name)], 8 * p)
        for got, budget in ((rx, chain), (ry, chain >> 2)):
            bl, bq = _best(c, budget, nice, maxc)
            assert (got >> 16, got & 0x7FFF) == (bl, p - bq), (name, budget)
        assert rx >> 16 > ry >> 16, name
