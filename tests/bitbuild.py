"""Hand-built deflate / deflate64 streams (fixed-Huffman blocks, RFC 1951
3.2.6, and dynamic ones, 3.2.7) for edge cases no encoder here produces: deflate64 length code 285
with its 16 extra bits (inflate/constants.ts:12,28: base 3, up to 65,538
bytes) and the 32,769 / 49,153 distance codes 30/31 (constants.ts:34).

A symbol list is [("lit", byte) | ("copy", length, distance) | ...]; expand()
is the plain LZ77 meaning of the list (the expected output), build() the bits.
blocks() strings stored blocks (RFC 1951 3.2.4), fixed and dynamic ones into one
member; dynamic_block() writes a dynamic header as given -- code lengths,
run-length ops, counts -- valid or not, for headers zlib's send_tree never writes."""


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):  # k bits of v, LSB first (RFC 1951 3.1.1)
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, k):  # a Huffman code: most significant bit first
        self.put(int(format(c, "0%db" % k)[::-1], 2), k)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def _fixed_lit(b, sym):
    if sym < 144:
        b.code(0x30 + sym, 8)
    elif sym < 256:
        b.code(0x190 + sym - 144, 9)
    elif sym < 280:
        b.code(sym - 256, 7)
    else:
        b.code(0xc0 + sym - 280, 8)


# (base, extra bits) per length code 257.. and distance code 0..; deflate64
# differs in length code 285 (3 + 16 extra bits) and adds distance codes 30/31
_LEN = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1),
        (19, 2), (23, 2), (27, 2), (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4),
        (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0)]
_DIST = [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (7, 1), (9, 2), (13, 2), (17, 3), (25, 3), (33, 4), (49, 4),
         (65, 5), (97, 5), (129, 6), (193, 6), (257, 7), (385, 7), (513, 8), (769, 8), (1025, 9), (1537, 9),
         (2049, 10), (3073, 10), (4097, 11), (6145, 11), (8193, 12), (12289, 12), (16385, 13), (24577, 13),
         (32769, 14), (49153, 14)]


def _len_code(n, d64):
    if d64 and n > 257:  # only code 285 reaches past 257 in deflate64
        return 28, n - 3, 16
    if not d64 and n == 258:
        return 28, 0, 0
    for i in range(27, -1, -1):
        base, x = _LEN[i]
        if base <= n < base + (1 << x):
            return i, n - base, x
    raise ValueError(n)


def _dist_code(d):
    for i in range(len(_DIST) - 1, -1, -1):
        base, x = _DIST[i]
        if base <= d < base + (1 << x):
            return i, d - base, x
    raise ValueError(d)


def _fixed_block(b, symbols, final, d64):
    b.put(1 if final else 0, 1)  # BFINAL
    b.put(1, 2)  # BTYPE = 01 (fixed)
    for s in symbols:
        if s[0] == "lit":
            _fixed_lit(b, s[1])
        elif s[0] == "sym":  # a literal/length symbol as numbered (286 / 287: in the fixed code, never valid)
            _fixed_lit(b, s[1])
        elif s[0] == "dsym":  # a length, then a distance symbol as numbered (30 / 31), no extra bits
            i, ev, ex = _len_code(s[1], d64)
            _fixed_lit(b, 257 + i)
            b.put(ev, ex)
            b.code(s[2], 5)
        else:
            _, n, d = s
            i, ev, ex = _len_code(n, d64)
            _fixed_lit(b, 257 + i)
            b.put(ev, ex)
            j, dv, dx = _dist_code(d)
            b.code(j, 5)
            b.put(dv, dx)
    _fixed_lit(b, 256)


_BL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical(lens):
    """{symbol: (code, length)}: the canonical Huffman code of the lengths (RFC 1951 3.2.2)."""
    count = [0] * 17
    for x in lens:
        count[x] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for k in range(1, 17):
        code = (code + count[k - 1]) << 1
        nxt[k] = code
    out = {}
    for sym, x in enumerate(lens):
        if x:
            out[sym] = (nxt[x], x)
            nxt[x] += 1
    return out


def flat_lengths(used, size):
    """Lengths of a complete code over the symbols `used` (of an alphabet of `size`), as even as can be: 2^k - n of
    the n symbols take k - 1 bits, the rest k; one symbol alone takes 1 bit (incomplete: the distance code's
    allowed case)."""
    used = sorted(used)
    lens, n = [0] * size, len(used)
    if n == 1:
        lens[used[0]] = 1
        return lens
    k = (n - 1).bit_length()
    for i, sym in enumerate(used):
        lens[sym] = k - 1 if i < (1 << k) - n else k
    return lens


def path_lengths(used, size, depth=15):
    """Lengths of a complete code `depth` deep over the symbols `used` (more than depth of them): the first ones a
    path 1, 2, .. depth - 1 bits or shorter as the count allows, the rest filling the deepest levels -- the last two
    symbols of `used` get `depth` bits."""
    used = list(used)
    lens = [0] * size
    # a path of depth - 1 single leaves and two at the bottom is complete with depth + 1 symbols; each further
    # symbol splits the shallowest leaf that is not on the path's end into two one level down
    ls = list(range(1, depth)) + [depth, depth]
    while len(ls) < len(used):
        x = min(ls)
        ls.remove(x)
        ls += [x + 1, x + 1]
    assert len(ls) == len(used) and max(ls) == depth
    for sym, x in zip(used, sorted(ls)):
        lens[sym] = x
    return lens


def plain_ops(lens):
    """The simple default of dynamic_block: every length as its own symbol, no repeat codes."""
    return [(x, 1) for x in lens]


def dynamic_block(lit_lens, dist_lens, symbols, ops=None, final=True, bl_lens=None, hclen=None, hlit=None,
                  hdist=None, eob=True, bits=None):
    """One dynamic-Huffman block (RFC 1951 3.2.7), written as told.

    lit_lens / dist_lens: the code lengths of the two alphabets (HLIT = len(lit_lens), HDIST = len(dist_lens)
    unless hlit / hdist say otherwise -- counts as coded, 257.. / 1..).  ops: the run-length coding of the two
    arrays as one sequence, [(symbol, count)]: (0..15, 1) a length, (16, 3..6) repeat the previous one, (17, 3..10)
    and (18, 11..138) zeros; None: plain_ops.  The ops are written as given, whether or not they spell the arrays.
    bl_lens: the 19 bit-length code lengths (None: flat_lengths over the ops' symbols); hclen: how many of them the
    header carries (None: up to the last non-zero one in the header's order, 4 at least).
    symbols: ("lit", byte) | ("copy", length, distance) | ("sym", n) a literal/length symbol as numbered, no extra
    bits; eob False leaves the end-of-block code out.  bits: the _Bits to append to (None: a new stream).
    Returns (bytes so far, expansion of the lit / copy symbols)."""
    b = bits if bits is not None else _Bits()
    if ops is None:
        ops = plain_ops(list(lit_lens) + list(dist_lens))
    if bl_lens is None:
        used = {o[0] for o in ops}
        if len(used) == 1:
            used.add(0 if 0 not in used else 1)  # (a bit-length code must be complete)
        bl_lens = flat_lengths(used, 19)
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if bl_lens[_BL_ORDER[i]]])
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put((len(lit_lens) if hlit is None else hlit) - 257, 5)
    b.put((len(dist_lens) if hdist is None else hdist) - 1, 5)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(bl_lens[_BL_ORDER[i]], 3)
    bc = canonical(bl_lens)
    for sym, count in ops:
        b.code(*bc[sym])
        if sym == 16:
            b.put(count - 3, 2)
        elif sym == 17:
            b.put(count - 3, 3)
        elif sym == 18:
            b.put(count - 11, 7)
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for s in symbols:
        if s[0] == "lit" or s[0] == "sym":
            b.code(*lc[s[1]])
        else:
            _, n, d = s
            i, ev, ex = _len_code(n, False)
            b.code(*lc[257 + i])
            b.put(ev, ex)
            j, dv, dx = _dist_code(d)
            b.code(*dc[j])
            b.put(dv, dx)
    if eob:
        b.code(*lc[256])
    return b.bytes(), expand([s for s in symbols if s[0] != "sym"])


def build(symbols, d64=True):
    """One final fixed-Huffman block holding the symbols."""
    b = _Bits()
    _fixed_block(b, symbols, True, d64)
    return b.bytes()


def blocks(parts, d64=False):
    """A member of blocks in order, the last one final: ("stored", bytes) -- BTYPE 00, the bits to the byte
    boundary, LEN, NLEN, the bytes (at most 65,535) -- ("fixed", symbols), ("dynamic", keyword arguments of
    dynamic_block: its copies stay within the block), or ("bits", block, nbits, expansion): one block taken
    verbatim from an encoder's member (its first nbits, BFINAL rewritten).  Returns (member, expansion)."""
    b, out = _Bits(), bytearray()
    for k, part in enumerate(parts):
        final = k + 1 == len(parts)
        if part[0] == "bits":
            _, data, nbits, exp = part
            b.put(1 if final else 0, 1)
            for i in range(1, nbits):
                b.put((data[i >> 3] >> (i & 7)) & 1, 1)
            out += exp
        elif part[0] == "dynamic":
            out += dynamic_block(final=final, bits=b, **part[1])[1]
        elif part[0] == "stored":
            data = part[1]
            assert len(data) <= 65535
            b.put(1 if final else 0, 1)
            b.put(0, 2)
            b.put(0, (8 - b.n) & 7)
            b.put(len(data), 16)
            b.put(len(data) ^ 0xFFFF, 16)
            for x in data:
                b.put(x, 8)
            out += data
        else:
            _fixed_block(b, part[1], final, d64)
            for s in part[1]:
                if s[0] == "lit":
                    out.append(s[1])
                elif s[0] == "copy":
                    for _ in range(s[1]):
                        out.append(out[-s[2]])
    return b.bytes(), bytes(out)


def expand(symbols):
    out = bytearray()
    for s in symbols:
        if s[0] == "lit":
            out.append(s[1])
        else:
            _, n, d = s
            for _ in range(n):
                out.append(out[-d])
    return bytes(out)


def long_copies():
    """deflate64 members with copies longer than the 64 KiB window: lengths
    65,537 / 65,538 at distances that do not divide 65,536, and a 49,153+
    distance behind them."""
    cases = []
    lits = [("lit", c) for c in b"abc"]
    cases.append(lits + [("copy", 65538, 3)])
    seed = [("lit", (i * 37 + 11) & 0xff) for i in range(300)]
    cases.append(seed + [("copy", 65537, 299), ("copy", 1000, 50000)])
    cases.append([("lit", c) for c in b"xy"] + [("copy", 65538, 2), ("copy", 65538, 65536), ("copy", 300, 7)])
    return [(build(s, True), expand(s)) for s in cases]


def stored_mix(rng, n, src, level0=False):
    """A member of about n output bytes: stored blocks (0 .. 65,535 bytes of src, sizes not multiples of 4) and,
    unless level0, fixed blocks between them whose copies reach back up to 32 KiB -- into the stored bytes too.
    Returns (member, expansion)."""
    parts, made, at = [], 0, 0
    while made < n:
        if level0 or rng.random() < 0.5:
            k = min(rng.choice([0, 1, 7, 999, 5003, 20001, 65535]), n - made + 1)
            parts.append(("stored", src[at % len(src):at % len(src) + k]))
            at += k
            made += len(parts[-1][1])
        else:
            syms = []
            for _ in range(rng.choice([10, 300, 4000])):
                if made < 1 or rng.random() < 0.6:
                    syms.append(("lit", src[at % len(src)]))
                    at += 1
                    made += 1
                else:  # (short copies: under 8 output bytes per input byte, as the segmented decode takes)
                    ln = rng.choice([3, 4, 9, 17, 40])
                    syms.append(("copy", ln, rng.randint(1, min(made, 32768))))
                    made += ln
            parts.append(("fixed", syms))
    return blocks(parts)


def greedy_ops(lens):
    """Run-length ops over the two length arrays taken as one sequence, every run coded as long as it goes -- so a
    run that spans the end of the literal/length array becomes one repeat across the boundary (zlib's send_tree
    codes the two arrays apart and never writes that; inflate.ts:760-810 reads it)."""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        n = j - i
        if v:
            ops.append((v, 1))
            n -= 1
        while n >= 3:
            k = min(n, 138 if not v else 6)
            ops.append((16, k) if v else ((17, k) if k <= 10 else (18, k)))
            n -= k
        ops += [(v, 1)] * n
        i = j
    return ops


def _lens(size, pairs):
    out = [0] * size
    for syms, x in pairs:
        for sym in syms:
            out[sym] = x
    return out


def header_cases():
    """Dynamic headers zlib's send_tree never writes, [(name, parts)] with parts for blocks(): valid ones (by RFC
    1951; the oracle judges) and invalid ones, which the reference reports as data errors by message
    (inflate.ts:713-900).  Every case is one small block."""
    text = [("lit", c) for c in b"ABCDEF" * 3] + [("copy", 3, 6), ("lit", 70), ("copy", 3, 1)]
    abc = list(range(65, 71))
    lit8 = _lens(258, [(abc + [256, 257], 3)])  # eight 3-bit codes
    cases = []

    def dyn(name, **kw):
        cases.append((name, [("dynamic", kw)]))

    # ---- valid by the RFC
    dyn("repeat16_across", lit_lens=lit8, dist_lens=[3] * 8, symbols=text, ops=greedy_ops(lit8 + [3] * 8))
    l17 = lit8 + [0, 0]
    dyn("repeat17_across", lit_lens=l17, dist_lens=[0, 0, 1], symbols=text[:18] + [("copy", 3, 3)],
        ops=greedy_ops(l17 + [0, 0, 1]))
    l18 = lit8 + [0] * 12
    dyn("repeat18_across", lit_lens=l18, dist_lens=[0] * 5 + [1], symbols=text[:18] + [("copy", 3, 7)],
        ops=greedy_ops(l18 + [0] * 5 + [1]))
    dyn("one_distance_code_used", lit_lens=lit8, dist_lens=[1], symbols=text[:18] + [("copy", 3, 1)])
    dyn("one_distance_code_unused", lit_lens=lit8, dist_lens=[1], symbols=text[:18])
    dyn("hdist1_length0", lit_lens=lit8, dist_lens=[0], symbols=text[:18])
    dyn("hclen19", lit_lens=lit8, dist_lens=[3] * 8, symbols=text, ops=greedy_ops(lit8 + [3] * 8), hclen=19)
    dyn("hclen4_no_codes", lit_lens=[0] * 257, dist_lens=[0], symbols=[], eob=False, ops=[(18, 138), (18, 120)],
        bl_lens=_lens(19, [([0, 18], 1)]), hclen=4)
    # both trees 15 deep and complete, the 15-bit codes used: literal 'Z' and length code 285 (258 bytes),
    # distance codes 1 and 0 (distances 2 and 1)
    used = [256] + list(range(65, 82)) + [257, 258, 90, 285]
    deep_l = path_lengths(used, 286)
    deep_d = path_lengths(list(range(29, -1, -1)), 30)
    deep = ([("lit", c) for c in b"ABCDEFGHIJKLMNOPQZ"] + [("copy", 258, 1), ("lit", 90), ("copy", 258, 2),
                                                            ("copy", 3, 1), ("copy", 4, 18), ("copy", 258, 24)])
    dyn("both_trees_15_deep", lit_lens=deep_l, dist_lens=deep_d, symbols=deep)
    dyn("both_trees_15_deep_rle", lit_lens=deep_l, dist_lens=deep_d, symbols=deep, ops=greedy_ops(deep_l + deep_d))
    all_l, all_d = flat_lengths(range(286), 286), flat_lengths(range(30), 30)
    every = ([("lit", c) for c in range(0, 256, 5)] + [("copy", n, d) for n, d in
                                                        ((3, 1), (10, 4), (11, 5), (18, 7), (35, 9), (67, 17),
                                                         (130, 33), (131, 49), (257, 50), (258, 52))])
    dyn("all_316_codes", lit_lens=all_l, dist_lens=all_d, symbols=every, ops=greedy_ops(all_l + all_d))
    # a bit-length code 7 deep, the 7-bit codes (of lengths 8 and 9) the ones most used
    dyn("bit_length_codes_of_7_bits", lit_lens=all_l, dist_lens=all_d, symbols=every,
        bl_lens=path_lengths([0, 1, 2, 3, 6, 7, 10, 11, 4, 5, 8, 9], 19, depth=7))
    # ---- invalid: data errors by message
    none = dict(symbols=[], eob=False)
    dyn("lit_oversubscribed", lit_lens=_lens(257, [([65, 66, 256], 1)]), dist_lens=[1], **none)
    dyn("lit_incomplete", lit_lens=_lens(257, [([65, 256], 2)]), dist_lens=[1], **none)
    dyn("dist_oversubscribed", lit_lens=lit8, dist_lens=[1, 1, 1], **none)
    dyn("dist_incomplete", lit_lens=lit8, dist_lens=[2, 2], **none)
    dyn("dist_incomplete_used", lit_lens=lit8, dist_lens=[0, 2], symbols=text[:6] + [("copy", 3, 2)])
    dyn("repeat16_first", lit_lens=lit8, dist_lens=[1], ops=[(16, 3)] + greedy_ops(lit8 + [1])[1:], **none)
    dyn("repeat_past_the_end", lit_lens=lit8, dist_lens=[1], ops=greedy_ops(lit8 + [1])[:-1] + [(18, 138)], **none)
    dyn("repeat16_past_the_end", lit_lens=lit8, dist_lens=[3], ops=greedy_ops(lit8)[:-1] + [(16, 6)], **none)
    dyn("no_end_of_block", lit_lens=_lens(258, [(abc + [255, 257], 3)]), dist_lens=[1], **none)
    dyn("hlit_287", lit_lens=_lens(287, [(abc + [256, 257], 3)]), dist_lens=[1], **none)
    dyn("hlit_288", lit_lens=_lens(288, [(abc + [256, 257], 3)]), dist_lens=[1], **none)
    dyn("hdist_31", lit_lens=lit8, dist_lens=[5] * 31, **none)
    dyn("hdist_32", lit_lens=lit8, dist_lens=[5] * 32, **none)
    for name, syms in (("symbol_286", [("lit", 65), ("sym", 286)]), ("symbol_287", [("lit", 65), ("sym", 287)]),
                       ("distance_symbol_30", [("lit", 65), ("lit", 66), ("lit", 67), ("dsym", 3, 30)]),
                       ("distance_symbol_31", [("lit", 65), ("lit", 66), ("lit", 67), ("dsym", 3, 31)])):
        cases.append((name, [("fixed", syms)]))
    return cases
