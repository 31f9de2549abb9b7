"""A plain-Python reader of raw deflate streams (RFC 1951) for the tests: what
each block's header says and what its symbols are, so that a test can state
which rare branches of the tree builder an encoder's output went through
(trees.ts:187-259 gen_bitlen's overflow repair, :318-414 scan_tree / send_tree)
and a byte mismatch can be named by block and field.

parse(data) returns one Block per block:

  type            0 stored, 1 fixed, 2 dynamic;  final, start / end (bit offsets)
  hlit hdist hclen   the header counts as coded (257.., 1.., 4..); None unless dynamic
  bl_lens         the 19 bit-length code lengths, in symbol order (not the permuted header order)
  lit_lens dist_lens   the code lengths (hlit and hdist of them; the fixed ones for a fixed block)
  ops             the header's run-length ops: (symbol 0..18, repeat count) -- count 1 for a plain length
  lit_freq dist_freq bl_freq   symbol frequencies in the block (286 / 30 / 19 counts; the end of block counted)
  symbols         ("lit", byte) | ("copy", length, distance), without the end of block
  widest          the widest symbol in bits: code + extra bits, length plus distance
  stored          a stored block's bytes

huffman_depth(freqs) is the depth of the Huffman tree of the non-zero
frequencies with no length limit; first_difference(a, b) names the first block
and field in which two streams differ.
"""
import heapq

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
         227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
         4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
BL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def length_code(n):
    """The length code (0 .. 28, symbol 257 + it) of a match length."""
    return 28 if n == 258 else max(i for i in range(28) if LBASE[i] <= n)


def distance_code(d):
    return max(i for i in range(30) if DBASE[i] <= d)


class Block:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "Block(type=%d, bits %d..%d, hlit=%s, hdist=%s, hclen=%s, %d symbols)" % (
            self.type, self.start, self.end, self.hlit, self.hdist, self.hclen, len(self.symbols))


class _Reader:
    def __init__(self, data):
        self.d, self.at, self.acc, self.n = bytes(data), 0, 0, 0

    def need(self, k):
        while self.n < k:
            if self.at >= len(self.d):
                raise ValueError("stream ends inside a block")
            self.acc |= self.d[self.at] << self.n
            self.at += 1
            self.n += 8

    def get(self, k):
        if k == 0:
            return 0
        self.need(k)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def pos(self):
        return 8 * self.at - self.n

    def sym(self, tab):
        """One Huffman symbol: (symbol, code length).  tab = (lookup, maxbits), lookup indexed by the next
        maxbits bits as they lie in the stream; the stream's zero padding serves a short last code."""
        look, m = tab
        while self.n < m and self.at < len(self.d):
            self.acc |= self.d[self.at] << self.n
            self.at += 1
            self.n += 8
        e = look[self.acc & ((1 << m) - 1)]
        if e is None:
            raise ValueError("a bit pattern that is no code")
        s, x = e
        if x > self.n:
            raise ValueError("stream ends inside a block")
        self.acc >>= x
        self.n -= x
        return s, x


def canonical_codes(lens):
    """{symbol: (code, length)} of the canonical Huffman code (RFC 1951 3.2.2)."""
    count = [0] * 16
    for x in lens:
        count[x] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, x in enumerate(lens):
        if x:
            out[s] = (nxt[x], x)
            nxt[x] += 1
    return out


def _table(lens):
    m = max(lens) if lens else 0
    if m == 0:
        return [None], 0
    look = [None] * (1 << m)
    for s, (c, x) in canonical_codes(lens).items():
        r = int(format(c, "0%db" % x)[::-1], 2)  # the code as its bits lie in the stream
        if r >= (1 << m):
            continue  # (an over-subscribed set: codes past the code space)
        for k in range(r, 1 << m, 1 << x):
            look[k] = (s, x)
    return look, m


def kraft(lens):
    """Sum of 2^-length over the used codes, as a fraction of 2^15 (32768 = complete)."""
    return sum(1 << (15 - x) for x in lens if x)


def parse(data, strict=True):
    """The blocks of a raw deflate stream.  A stream that is no valid deflate raises ValueError -- or, with strict
    False, ends the list with the block read so far, the reason in its `error`."""
    r, out = _Reader(data), []
    try:
        _blocks(r, out)
    except ValueError as e:
        if strict:
            raise
        out[-1].error = str(e)
    return out


def _blocks(r, out):
    while True:
        start = r.pos()
        final, typ = r.get(1), r.get(2)
        b = Block(type=typ, final=final, start=start, hlit=None, hdist=None, hclen=None, bl_lens=None,
                  lit_lens=None, dist_lens=None, ops=[], lit_freq=[0] * 286, dist_freq=[0] * 30,
                  bl_freq=[0] * 19, symbols=[], widest=0, stored=None, header_end=None, end=None, error=None)
        out.append(b)
        if typ == 3:
            raise ValueError("block type 3")
        if typ == 0:
            r.get(r.n & 7)
            n, nn = r.get(16), r.get(16)
            if n != nn ^ 0xFFFF:
                raise ValueError("stored block lengths")
            at = r.pos() >> 3
            if at + n > len(r.d):
                raise ValueError("stream ends inside a block")
            b.stored = r.d[at:at + n]
            r.at, r.acc, r.n = at + n, 0, 0
            b.header_end = 8 * at
        else:
            if typ == 1:
                b.lit_lens, b.dist_lens = list(FIXED_LIT), list(FIXED_DIST)
            else:
                _header(r, b)
            b.header_end = r.pos()
            _symbols(r, b)
        b.end = r.pos()
        if final:
            return


def _header(r, b):
    b.hlit, b.hdist, b.hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    b.bl_lens = [0] * 19
    for i in range(b.hclen):
        b.bl_lens[BL_ORDER[i]] = r.get(3)
    tab = _table(b.bl_lens)
    lens = []
    while len(lens) < b.hlit + b.hdist:
        s, _ = r.sym(tab)
        b.bl_freq[s] += 1
        if s < 16:
            b.ops.append((s, 1))
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise ValueError("repeat with no length before it")
            n, v = 3 + r.get(2), lens[-1]
        elif s == 17:
            n, v = 3 + r.get(3), 0
        else:
            n, v = 11 + r.get(7), 0
        b.ops.append((s, n))
        lens += [v] * n
    if len(lens) > b.hlit + b.hdist:
        raise ValueError("a repeat past the last length")
    b.lit_lens, b.dist_lens = lens[:b.hlit], lens[b.hlit:]


def _symbols(r, b):
    lt, dt = _table(b.lit_lens), _table(b.dist_lens)
    lf, df, syms, widest = b.lit_freq, b.dist_freq, b.symbols, 0
    while True:
        s, l1 = r.sym(lt)
        if s < 256:
            lf[s] += 1
            syms.append(("lit", s))
            if l1 > widest:
                widest = l1
            continue
        if s == 256:
            lf[256] += 1
            break
        if s > 285:
            raise ValueError("length symbol %d" % s)
        lf[s] += 1
        e1 = LEXT[s - 257]
        n = LBASE[s - 257] + r.get(e1)
        d, l2 = r.sym(dt)
        if d > 29:
            raise ValueError("distance symbol %d" % d)
        df[d] += 1
        e2 = DEXT[d]
        syms.append(("copy", n, DBASE[d] + r.get(e2)))
        if l1 + e1 + l2 + e2 > widest:
            widest = l1 + e1 + l2 + e2
    b.widest = widest


def expand(blocks):
    """The bytes the parsed blocks stand for (plain LZ77, no window limit)."""
    out = bytearray()
    for b in blocks:
        if b.type == 0:
            out += b.stored
            continue
        for s in b.symbols:
            if s[0] == "lit":
                out.append(s[1])
            else:
                _, n, d = s
                if d >= n:
                    out += out[len(out) - d:len(out) - d + n]
                else:
                    for _ in range(n):
                        out.append(out[-d])
    return bytes(out)


def huffman_depth(freqs):
    """Depth of the deepest leaf of the Huffman tree over the non-zero frequencies, with no length limit:
    the two lightest nodes merge, the shallower one first among equal weights (the order that keeps the tree
    as shallow as any Huffman tree of these weights can be).  One symbol: 1; none: 0."""
    h = [(f, 0, i) for i, f in enumerate(freqs) if f]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    k = len(freqs)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1, k))
        k += 1
    return h[0][1]


def huffman_lengths(freqs):
    """Leaf depths of that same unlimited tree, per symbol (0 for an unused one)."""
    h = [(f, 0, i, (i,)) for i, f in enumerate(freqs) if f]
    lens = [0] * len(freqs)
    if len(h) == 1:
        lens[h[0][2]] = 1
        return lens
    heapq.heapify(h)
    k = len(freqs)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for i in a[3] + b[3]:
            lens[i] += 1
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1, k, a[3] + b[3]))
        k += 1
    return lens


def _first_list_diff(x, y):
    for i in range(min(len(x), len(y))):
        if x[i] != y[i]:
            return i
    return min(len(x), len(y)) if len(x) != len(y) else None


def first_difference(a, b):
    """Where two raw deflate streams first differ, as text: block number and field (block type, a header count,
    a code length, a header op, a symbol), or None when they are equal.  A stream that is no valid deflate is
    compared as far as it reads."""
    if a == b:
        return None
    at = _first_list_diff(a, b)
    where = "first differing byte %d (lengths %d / %d)" % (at, len(a), len(b))
    pa, pb = parse(a, strict=False), parse(b, strict=False)
    for k, (x, y) in enumerate(zip(pa, pb)):
        pre = "block %d (bit %d): " % (k, x.start)
        if x.start != y.start:
            return "block %d starts at bit %d / %d; %s" % (k, x.start, y.start, where)
        if (x.type, x.final) != (y.type, y.final):
            return pre + "block type / final %d/%d against %d/%d" % (x.type, x.final, y.type, y.final)
        for f in ("hlit", "hdist", "hclen"):
            if getattr(x, f) != getattr(y, f):
                return pre + "%s %s against %s" % (f, getattr(x, f), getattr(y, f))
        for f, name in (("bl_lens", "bit-length code length"), ("lit_lens", "literal/length code length"),
                        ("dist_lens", "distance code length")):
            u, v = getattr(x, f), getattr(y, f)
            if u != v:
                u, v = u or [], v or []
                i = _first_list_diff(u, v)
                return pre + "%s of symbol %d: %s against %s" % (
                    name, i, u[i] if i < len(u) else None, v[i] if i < len(v) else None)
        if x.ops != y.ops:
            i = _first_list_diff(x.ops, y.ops)
            return pre + "header op %d: %s against %s" % (i, x.ops[i:i + 1], y.ops[i:i + 1])
        if x.stored != y.stored:
            return pre + "stored bytes differ (%d / %d)" % (len(x.stored or b""), len(y.stored or b""))
        if x.symbols != y.symbols:
            i = _first_list_diff(x.symbols, y.symbols)
            return pre + "symbol %d: %s against %s" % (i, x.symbols[i:i + 1], y.symbols[i:i + 1])
        if x.error != y.error:
            return pre + "error %s against %s" % (x.error, y.error)
        if x.end != y.end:
            return pre + "ends at bit %s / %s" % (x.end, y.end)
    if len(pa) != len(pb):
        return "%d blocks against %d" % (len(pa), len(pb))
    return "equal blocks; " + where
