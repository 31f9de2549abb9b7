"""Streams built for zs_k_sweep's groups of chain steps in which a lane's chain ends
(csrc/zs_sweep_ends.h): a dead step -- a member of the neighbouring bucket, or an occurrence
more than MAX_DIST back -- that matches the lane's position better than every live step of its
group.  Shared by tests/test_sweep_ends_model.py (the host model must see every case occur)
and tests/test_gpu_sweep_ends.py (the kernel's bytes)."""
import corpus

MAX_DIST = 32506
# two trigrams whose 15-bit hashes differ by one (bit 0 of the third byte) and whose X -- the bits of the first
# two bytes that the hash loses -- is equal: T1's bucket follows T0's in the member array, and in the 7-bit
# signature form a T0 member's record equals a T1 member's wherever the following bytes agree
T0, T1 = b"q#Z", b"q#["
S = b"MATCHING-TAIL-BYTES!"  # what follows the trigram in a "long" occurrence (>= 10 bytes for either form)


def _hash(t):
    return ((t[0] << 10) ^ (t[1] << 5) ^ t[2]) & 0x7FFF


assert _hash(T1) == _hash(T0) + 1


def _r7(seed, n):
    """Filler: 7-bit bytes without any trigram's first byte."""
    return bytes(x & 0x7F for x in corpus.rand(seed, n)).replace(b"q", b"A").replace(b"w", b"B").replace(b"k", b"C")


def _foreign(seed, n0, n1, shared, live_shared):
    """n0 occurrences of T0 + S[:shared], then n1 of T1: every other one T1 + S[:shared] (its dead steps, the T0
    members, match `shared` bytes past the trigram), the rest T1 + S[:live_shared]."""
    out = [_r7(seed, 40)]
    for i in range(n0):
        out.append(T0 + S[:shared] + _r7(seed + 1 + i, 5))
    for i in range(n1):
        out.append(T1 + (S[:shared] if i & 1 else S[:live_shared]) + _r7(seed + 500 + i, 5))
    return b"".join(out)


def _window(seed, tri, near, hi_first=False):
    """A probe tri + S at a position whose chain holds `near` occurrences sharing one byte past the trigram inside
    the window and, behind them, twelve occurrences of tri + S more than MAX_DIST back."""
    out = [_r7(seed, 60)]
    for i in range(12):
        out.append(tri + S + _r7(seed + 1 + i, 30))
    far_end = sum(map(len, out))
    out.append(_r7(seed + 50, MAX_DIST + 200))  # every far occurrence is now out of every later position's reach
    for i in range(near):
        out.append(tri + S[:1] + _r7(seed + 100 + i, 20))
    out.append(tri + S + _r7(seed + 200, 40))
    d = b"".join(out)
    assert len(d) - 60 - far_end > MAX_DIST
    return d


def _head_edge(seed):
    """Head candidates at exactly MAX_DIST (live, and the only live step: an older, longer occurrence behind it is
    dead) and at MAX_DIST + 1 (no head: the position is never searched)."""
    b = bytearray(_r7(seed, 36000))
    e0, e1, e2 = b"w%Y" + S + b"-and-more", b"w%Y" + S + b"+less", b"k&X" + S
    b[1000:1000 + len(e0)] = e0
    b[1200:1200 + len(e1)] = e1
    p = 1200 + MAX_DIST
    b[p:p + len(e0)] = e0  # the head at exactly MAX_DIST shares S, the dead occurrence 200 further all of e0
    b[1500:1500 + len(e2)] = e2
    p2 = 1500 + MAX_DIST + 1
    b[p2:p2 + len(e2)] = e2
    return bytes(b)


def streams():
    s = {}
    # dead winner and dead long: the T0 members match T1's probes in the whole signature (7-bit form)
    s["foreign-long"] = _foreign(100, 24, 20, len(S), 1)
    # the dead steps match 5 bytes (of the signature's: the trigram's X and two more), the live ones 3..4
    s["foreign-short"] = _foreign(200, 24, 20, 2, 1)
    # a death inside a group behind step 8 (ten live steps), and inside steps 1..8 (three)
    s["window-late"] = _window(300, b"q#Z", 10)
    s["window-early"] = _window(400, b"q#Z", 3)
    s["head-edge"] = _head_edge(500)
    # a bucket of 100 that starts mid-chunk behind one of 40: the lanes die eight per group, every dead step long
    s["ramp"] = _foreign(600, 40, 100, len(S), len(S))
    # ... and behind unrelated members
    s["ramp-plain"] = _r7(700, 40) + b"".join(b"q#Z" + _r7(701 + i, 9) for i in range(100))
    for k in list(s):  # the same with one byte >= 0x80: the 11-byte signature form
        s[k + "+hi"] = b"\xe9" + s[k]
    assert all(len(d) <= 65536 for d in s.values())
    return s
