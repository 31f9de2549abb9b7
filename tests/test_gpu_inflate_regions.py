"""zs_inflate_batch_device_ex on every decode route, through the harness of regioncases.py: output regions
at every 4-byte residue of 16 with capacities of exactly the output rounded up to 4 (and 64 more), one
dword of canary between them at the narrowest; inputs at odd offsets between zeros, 0xff and random bytes.

Every run must leave the canaries and the input as they were, give the same rows whatever the filler, and
equal the oracle (oracle.decompress with the reference's window-wrap copy, or without it under
inflate_ref_wrap = 0) in status, phase, message, bytes and consumed, and the trailer's check value for the
wrapped formats.  The route each test means to run is forced with options and asserted by the lane and
segmented counts (zs_last_inflate_lane_count counts the members ANY fast decoder finished, the segmented
count those inflate_seg.hip finished) and, where the counts cannot tell two decoders apart, by the phase
the timing marks name.  tests/test_plan_model.py holds the same route claims without a GPU.

Each route also gets damaged members -- a flipped bit, truncations to 2/3, 1/3 and one byte, capacities 4
bytes and a half too small -- which leave the fast decoders part-way and are decoded again by the fallback
wave kernel or the exact kernel into the same region."""
import functools
import os

import pytest

import corpus
import oracle
import regioncases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = (-5, 0, "output capacity exceeded")  # test_gpu_inflate.py::test_capacity_too_small
FORMATS = ["deflate-raw", "deflate", "gzip", "deflate64-raw"]
KAT_285 = bytes.fromhex("4b1cfdff07a3e5030000")  # deflate64 length code 285: 66,539 x "a"


@functools.lru_cache(maxsize=None)
def source(kind, n, seed):
    if kind == "runs":
        return rc.runs(seed, n)
    return corpus.make({"kind": kind, "n": n, "seed": corpus.stream_seed(seed)})


@functools.lru_cache(maxsize=None)
def member(kind, n, seed, level, fmt):
    """(compressed, output length) of a corpus member; a deflate64-raw one is the deflate-raw stream (the
    oracle decides what it decodes to as deflate64)"""
    return oracle.compress(source(kind, n, seed), level, "deflate-raw" if fmt == "deflate64-raw" else fmt)[1], n


@functools.lru_cache(maxsize=None)
def fixture(name):
    """a deflate64 fixture of tests/golden/d64 and its output length (by the oracle)"""
    c = open(os.path.join(ROOT, "tests", "golden", "d64", name + ".deflate64"), "rb").read()
    st, out, *_ = oracle.decompress(c, "deflate64-raw", cap=3 << 20)
    assert st == 1
    return c, len(out)


@functools.lru_cache(maxsize=None)
def want(comp, fmt, cap, bugs):
    return oracle.decompress(comp, fmt, cap=cap, reference_bugs=bugs)


# ---- members: source lengths with len % 4 = 0, 1, 2, 3, below and above 16 and 64 bytes (the unit tail, the ring
# flush), above 32,768 and 65,536 (the resolve's rings wrap; the reference's output buffers change)
SMALL = [("text", 0, 1, 6), ("text", 1, 2, 6), ("text", 5, 3, 1), ("text", 15, 4, 9), ("text", 63, 5, 6),
         ("mixed", 66, 6, 1), ("text", 259, 7, 9), ("text", 6001, 8, 6), ("mixed", 6002, 9, 1), ("rand", 3003, 10, 6),
         ("runs", 5000, 11, 9)]
LARGE = [("text", 33002, 21, 6), ("mixed", 70003, 22, 1), ("text", 150001, 23, 9), ("mixed", 200002, 24, 6),
         ("text", 262144, 25, 1), ("runs", 157919, 26, 6), ("rand", 70000, 27, 6)]


def small(fmt):
    """(as deflate64 the runs member's length-258 copies mean longer ones: a text member in its place)"""
    last = ("text", 4099, 12, 9) if fmt == "deflate64-raw" else SMALL[-1]
    ms = [member(k, n, seed, lv, fmt) for k, n, seed, lv in SMALL[:-1] + [last]]
    assert all(len(c) <= 4096 for c, _ in ms)
    return ms


def large(fmt):
    return [member(k, n, seed, lv, fmt) for k, n, seed, lv in LARGE]


def both_caps(ms):
    """each member with a capacity of exactly its output rounded up to 4, and with 64 more"""
    return [(c, rc.cap4(n) + extra) for c, n in ms for extra in (0, 64)]


def damaged(bases):
    """The damaged set of `bases` [(member, output length)], 8 per base and one more: the truncated members stand
    where filler follows them (regioncases.follows_filler), the last one in front of the tail."""
    items, cut = [], []
    for c, n in bases:
        assert n >= 8 and len(c) >= 12
        flip, late = bytearray(c), bytearray(c)
        flip[len(c) // 2] ^= 0x10
        late[len(c) - 6] ^= 0x01
        at = len(items)
        items += [(c, rc.cap4(n)), (c[:2 * len(c) // 3], rc.cap4(n)), (c[:1], rc.cap4(n)), (bytes(flip), rc.cap4(n) + 64),
                  (c, rc.cap4(n) - 4), (c[:len(c) // 3], rc.cap4(n) + 64), (c, rc.cap4(n // 2)), (bytes(late), rc.cap4(n))]
        cut += [at + 1, at + 2, at + 5]
    items.append((bases[0][0][:2 * len(bases[0][0]) // 3], rc.cap4(bases[0][1]) + 64))
    cut.append(len(items) - 1)
    assert all(rc.follows_filler(i, len(items)) for i in cut)
    return items


def expected(comp, fmt, cap, bugs):
    """(status, phase, message, bytes, consumed) by the oracle, or None where the output passes `cap` (the
    oracle's ZO_MEM_ERROR without a phase): the engine's capacity outcome"""
    st, out, cons, ph, msg = want(comp, fmt, cap, bugs)
    if st == oracle.Z_MEM_ERROR and ph == oracle.PHASE_NONE:
        return None
    return st, ph, msg, out, cons


def check_rows(run, fmt, items, bugs, exact=None):
    """Every row against the oracle; a member whose output passes its capacity gives CAPACITY, and its other
    fields equal `exact`, the rows of the same batch with inflate_fast = 0."""
    short = 0
    for i, ((c, cap), row) in enumerate(zip(items, run.rows)):
        e = expected(c, fmt, cap, bugs)
        where = (fmt, i, len(c), cap, row[:3], len(row[3]), row[4])
        if e is None:
            short += 1
            assert row[:3] == CAPACITY, where
            assert exact is not None and row[3:] == exact[i][3:], where
            continue
        assert row[:5] == e, where + (e[:3], len(e[3]), e[4])
        chk = 0
        if e[0] == 1 and fmt in ("deflate", "gzip"):
            chk = oracle.crc32(e[3]) if fmt == "gzip" else oracle.adler32(e[3])
        assert row[5] == chk, where
    return short


def route(engine, fmt, items, opts, bugs=True, lanes=None, segs=None, phase=None, exact=None):
    """`items` [(member, capacity)] through the device entry under `opts`, once per filler.  lanes: the lane
    count expected ("ok": the members the oracle decodes, all finished by a fast decoder); segs: the segmented
    count; phase: a timing mark that must have been set.  Returns the last run."""
    comps, caps = [c for c, _ in items], [cap for _, cap in items]
    first = None
    for kind in rc.FILLERS:
        with rc.options(engine, **opts):
            engine.set_timing(phase is not None)
            try:
                if phase:
                    engine.last_ms()  # (earlier marks)
                run = rc.inflate_run(engine, fmt, comps, caps, kind)
                ran = phase is None or engine.last_ms(phase) >= 0
            finally:
                engine.set_timing(False)
        assert not run.dirty, "%s / %s: bytes outside every region changed at %r" % (fmt, kind, run.dirty)
        assert run.input_kept, (fmt, kind)
        check_rows(run, fmt, items, bugs, exact)
        if lanes is not None:
            assert run.lanes == (sum(1 for r in run.rows if r[0] == 1) if lanes == "ok" else lanes), (fmt, kind)
        if segs is not None:
            assert run.segs == segs, (fmt, kind, run.segs)
        assert ran, (fmt, kind, phase)
        first = first or run.rows
        assert run.rows == first, (fmt, kind)  # the bytes around a member do not matter
    return run


def route_damaged(engine, fmt, bases, opts, bugs=True, beside=(), **kw):
    """The damaged set of `bases` (in front of the members `beside`): the capacity members' remaining fields
    come from the exact kernel's run of the same batch."""
    items = damaged(bases) + list(beside)
    with rc.options(engine, **dict(opts, inflate_fast=0)):
        exact = rc.inflate_run(engine, fmt, [c for c, _ in items], [cap for _, cap in items])
    assert exact.ok() and exact.lanes == 0
    run = route(engine, fmt, items, opts, bugs, exact=exact.rows, **kw)
    # both short capacities of every base, the truncations and the flipped bit in the middle among the failures
    assert sum(1 for r in run.rows if r[:3] == CAPACITY) >= 2 * len(bases)
    assert sum(1 for r in run.rows if r[0] != 1) >= 5 * len(bases) + 1
    return run


def residues(run):
    return {o % 16 for o in run.offs}


# ---- the harness itself
def test_the_clean_check_reports_a_region_declared_short(engine):
    """The negative control: a member whose output fills its capacity, decoded; with its region declared 4
    bytes shorter than it is, the clean check reports exactly those 4 offsets (and nothing as it is)."""
    ms = [member("text", 63, 5, 6, "deflate-raw"), member("text", 6000, 31, 6, "deflate-raw"),
          member("text", 259, 7, 9, "deflate-raw")]
    items = [(c, rc.cap4(n)) for c, n in ms]
    run = rc.inflate_run(engine, "deflate-raw", [c for c, _ in items], [cap for _, cap in items])
    assert run.ok() and [r[0] for r in run.rows] == [1, 1, 1]
    assert run.out_len[1] == run.caps[1] == 6000
    caps = list(run.caps)
    caps[1] -= 4
    end = run.offs[1] + 6000
    assert rc.dirty(run.out, run.offs, caps) == [end - 4, end - 3, end - 2, end - 1]
    assert rc.dirty(run.out, run.offs, run.caps) == []


# ---- the lane kernel
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("lane_block", [1, 64])
def test_lane_kernel(engine, fmt, lane_block):
    """zs_k_inflate_lane<1, false> (lane_block 1: per-lane root tables) and <0, false> (64 members per
    workgroup, two workgroups): members of at most 4 KB of input, four times over so that every member
    meets several input gaps and output residues."""
    items = both_caps(small(fmt)) * 4
    opts = {"lane_block": lane_block}
    run = route(engine, fmt, items, opts, lanes="ok", segs=0)
    assert len(items) > 64 and residues(run) == {0, 4, 8, 12}
    route_damaged(engine, fmt, [small(fmt)[7], small(fmt)[9], small(fmt)[10]], opts, segs=0)


@pytest.mark.parametrize("fmt", FORMATS)
def test_lane_kernel_beside_a_large_member(engine, fmt):
    """zs_k_inflate_lane<2, false>: thin workgroups with a large member beside them (the segmented decode takes
    it).  The deflate64 batch ends in payload_63k, whose last code is a 1-bit end of block in front of the tail."""
    big = fixture("payload_63k") if fmt == "deflate64-raw" else member("text", 70003, 41, 6, fmt)
    items = both_caps(small(fmt)) + [(big[0], rc.cap4(big[1]))]
    run = route(engine, fmt, items, {}, lanes="ok", segs=1)
    assert run.rows[-1][0] == 1 and run.out_len[-1] == big[1]


# ---- the segmented decode
@pytest.mark.parametrize("fmt", ["deflate-raw", "deflate", "gzip"])
def test_segmented_decode_few_members(engine, fmt):
    """zs_k_seg_resolve<512, 65536> (at most two members per compute unit): 14 members of 33,002 .. 262,144
    bytes, every one finished by the segmented decode."""
    items = both_caps(large(fmt))
    run = route(engine, fmt, items, {}, segs=len(items))
    assert residues(run) == {0, 4, 8, 12}
    route_damaged(engine, fmt, [large(fmt)[1], large(fmt)[3], large(fmt)[5]], {})


@pytest.mark.parametrize("fmt", ["deflate-raw", "deflate"])
def test_segmented_decode_wide_window(engine, fmt):
    """zs_k_seg_walk<false, 2048, true>, 4,096-bit lanes and pieces cut in two: what a batch of few members of
    64 KiB of input and more on average gets at the defaults"""
    ms = [large(fmt)[3], large(fmt)[4]]
    assert sum(len(c) for c, _ in ms) >= 2 * 65536
    route(engine, fmt, both_caps(ms), {}, segs=4)


@pytest.mark.parametrize("opt", [("seg_split", 0), ("seg_split", 1), ("seg_bits", 1024)])
def test_segmented_decode_piece_options(engine, opt):
    """pieces whole or cut in two at the walk's mid points, and the narrowest lanes (seg_bits 1024 keeps the
    walk's 1,024-bit window): the same 14 members"""
    fmt, opts = "deflate-raw", {opt[0]: opt[1]}
    items = both_caps(large(fmt))
    route(engine, fmt, items, opts, segs=len(items))
    route_damaged(engine, fmt, [large(fmt)[0], large(fmt)[2]], opts)


@functools.lru_cache(maxsize=None)
def distinct(fmt):
    """40 members of 6,001 / 33,002 / 70,003 bytes, text and mixed at levels 1 / 6 / 9"""
    return tuple(member(("text", "mixed")[k % 2], (6001, 33002, 70003)[k % 3], 100 + k, (1, 6, 9)[(k // 6) % 3], fmt)
                 for k in range(40))


def many(fmt, n):
    """n members cycling the 40 distinct ones, the capacities exact and 64 more in turn"""
    d = distinct(fmt)
    return [(d[k % 40][0], rc.cap4(d[k % 40][1]) + 64 * ((k // 40) % 2)) for k in range(n)]


@pytest.mark.parametrize("fmt", ["deflate-raw", "gzip"])
def test_segmented_decode_many_members(engine, fmt):
    """zs_k_seg_resolve<256, 32768>: more than two segmented members per compute unit (seg_small_min 256 sends
    the 6,001-byte members there too); its 32 KiB ring wraps in the 33,002- and 70,003-byte members."""
    import torch

    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 8
    opts = {"seg_small_min": 256}
    items = many(fmt, n)
    assert all(len(c) > 256 for c, _ in items)
    run = route(engine, fmt, items, opts, segs=n)
    assert residues(run) == {0, 4, 8, 12}
    # the damaged set in front of the same members: still more than two per compute unit
    route_damaged(engine, fmt, [distinct(fmt)[1], distinct(fmt)[2]], opts, beside=items)


# ---- the split decode
def test_split_decode_deflate64(engine):
    """inflate_split.hip on deflate64: the fixtures whose capacity shows their expansion (and the length-285
    test vector), inflate_seg off; the batch ends in repeat_63k (a 1-bit end of block in front of the tail).
    100k_lines (2.19 MB from 149,744 bytes, the one fixture over inflate_wave_min) runs in a batch of its own:
    its pieces' scratch bounds the members beside it."""
    fmt, opts = "deflate64-raw", {"inflate_seg": 0}
    fx = [fixture(f) for f in ("zeros_100k", "10k_lines", "payload_65k", "repeat_65k", "payload_64k")]
    items = both_caps(fx + [(KAT_285, 66539)])
    items = [it for it in items if it[1] > 65536] + [(fixture("repeat_63k")[0], rc.cap4(fixture("repeat_63k")[1]))]
    run = route(engine, fmt, items, opts, lanes=len(items), segs=0, phase="split_decode")
    assert residues(run) == {0, 4, 8, 12}
    big = fixture("100k_lines")
    route(engine, fmt, [(big[0], rc.cap4(big[1])), (fx[0][0], rc.cap4(fx[0][1]))], opts, lanes=2, segs=0,
          phase="split_decode")
    route_damaged(engine, fmt, [fx[1], fx[2]], opts, segs=0)


def test_split_decode_raw_without_the_window_wrap_copy(engine):
    """... and on raw deflate with zlib semantics (inflate_ref_wrap 0): every member over one input byte
    (inflate_wave_min 1) splits at its block boundaries"""
    fmt, opts = "deflate-raw", {"inflate_seg": 0, "inflate_ref_wrap": 0, "inflate_wave_min": 1}
    items = both_caps(large(fmt) + small(fmt)[4:])
    route(engine, fmt, items, opts, bugs=False, lanes=len(items), segs=0, phase="split_decode")
    route_damaged(engine, fmt, [large(fmt)[1], large(fmt)[6]], opts, bugs=False, segs=0)


@pytest.mark.parametrize("fmt", ["deflate64-raw", "deflate-raw"])
def test_expanding_members_at_the_defaults(engine, fmt):
    """Members with a capacity past 64 KiB and 8 output bytes or more per input byte (zeros; the deflate64
    fixtures and the length-285 vector) leave the segmented decode at the defaults: deflate64 for the split
    decode, raw deflate -- with the window-wrap copy to reproduce -- for the wave kernel; the text member
    beside them is segmented."""
    if fmt == "deflate64-raw":
        wide = [fixture("zeros_100k"), fixture("10k_lines"), (KAT_285, 66539)]
    else:
        wide = [member("zeros", n, 0, lv, fmt) for n, lv in ((70001, 6), (100002, 1), (262147, 9))]
    assert all(rc.cap4(n) > 65536 and rc.cap4(n) // 8 >= len(c) for c, n in wide)
    items = both_caps(wide + [member("text", 33002, 21, 6, fmt)])
    phase = "split_decode" if fmt == "deflate64-raw" else "inflate_wave"
    route(engine, fmt, items, {}, lanes=len(items), segs=2, phase=phase)
    route_damaged(engine, fmt, [wide[0], wide[1]], {})


# ---- the wave kernel and the lanes for large members
@pytest.mark.parametrize("fmt", ["deflate", "gzip"])
@pytest.mark.parametrize("ref_wrap", [1, 0])
def test_wave_kernel(engine, fmt, ref_wrap):
    """zs_k_inflate_wave<true> / <false>: inflate_seg off and every member over one input byte large; zlib and
    gzip never split.  256 bytes leave its ring per step, whole words at the end."""
    opts = {"inflate_seg": 0, "inflate_wave_min": 1, "inflate_ref_wrap": ref_wrap}
    items = both_caps(large(fmt) + small(fmt)[1:])
    run = route(engine, fmt, items, opts, bugs=bool(ref_wrap), lanes="ok", segs=0, phase="inflate_wave")
    assert residues(run) == {0, 4, 8, 12}
    route_damaged(engine, fmt, [large(fmt)[0], large(fmt)[3]], opts, bugs=bool(ref_wrap), segs=0)


def test_one_lane_per_large_member(engine):
    """zs_k_inflate_lane<2, true>, the instance that tracks the reference's calls: inflate_seg off, and one
    large member is enough for the lanes (lane_large_min 1)"""
    fmt, opts = "deflate-raw", {"inflate_seg": 0, "lane_large_min": 1, "inflate_wave_min": 1024}
    items = both_caps(large(fmt) + small(fmt)[6:])
    assert sum(1 for c, _ in items if len(c) > 1024) >= 2 * len(LARGE) + 6
    route(engine, fmt, items, opts, lanes="ok", segs=0, phase="inflate_large")
    route_damaged(engine, fmt, [large(fmt)[2], large(fmt)[4]], opts, segs=0)


# ---- the exact kernel
@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_kernel(engine, fmt):
    """zs_k_inflate alone (inflate_fast 0), the state machine every other route falls back to"""
    opts = {"inflate_fast": 0}
    if fmt == "deflate64-raw":
        bigs = [fixture("payload_64k"), fixture("10k_lines"), fixture("zeros_100k")]
    else:
        bigs = [large(fmt)[0], large(fmt)[1], large(fmt)[5]]
    items = both_caps(small(fmt) + bigs)
    run = route(engine, fmt, items, opts, lanes=0, segs=0)
    assert residues(run) == {0, 4, 8, 12}
    route_damaged(engine, fmt, [small(fmt)[7], bigs[0]], opts, lanes=0, segs=0)
