"""GPU parity on the Huffman edge cases: the tree kernels (deflate_emit.hip
zs_k_trees / zs_k_layout / zs_k_emit: gen_bitlen's clamp and overflow repair in
all three trees, trees of one or two codes, the run-length header at its chunk
limits, 15-bit codes and the 48-bit symbol) against the oracle byte for byte on
the inputs of tests/huffcases.py -- tests/test_huffman_cases.py pins, on the CPU,
what each of them reaches --, and every decoder (lanes, wave, segmented, split,
exact) on the oracle's members of the same inputs and on the hand-built dynamic
headers of tests/bitbuild.py header_cases(), valid and invalid, that zlib's
send_tree never writes."""
import functools

import pytest

import bitbuild
import corpus
import deflate_header as dh
import oracle
import test_huffman_cases as hc

pytestmark = pytest.mark.gpu

WRAP = {"deflate-raw": (0, None), "deflate": (2, -4), "gzip": (10, -8)}  # header and trailer bytes around the blocks


def _check_compressed(engine, level, fmt, what=""):
    ins = hc.inputs()
    res = engine.compress_batch_raw([d for _, d in ins], fmt, level)
    lo, hi = WRAP[fmt]
    for (name, d), (st, out), ref in zip(ins, res, hc.compressed(level, fmt)):
        assert st == 1, (name, level, fmt, what, st)
        assert out == ref, "%s L%d %s %s: %s" % (name, level, fmt, what, dh.first_difference(ref[lo:hi], out[lo:hi]))


@pytest.mark.parametrize("level", hc.LEVELS)
def test_compress_equals_the_oracle(engine, level):
    _check_compressed(engine, level, "deflate-raw")


@pytest.mark.parametrize("fmt", ["deflate", "gzip"])
@pytest.mark.parametrize("level", [1, 6])
def test_compress_equals_the_oracle_in_the_wrapped_formats(engine, level, fmt):
    _check_compressed(engine, level, fmt)


@pytest.mark.parametrize("opt", [("lane_order", 0, 1), ("parse_waves", 1, 0), ("parse_waves", 4, 0)])
def test_compress_with_the_other_symbol_producers(engine, opt):
    """The tree kernel is shared, the symbol buffers feeding it are not: the ballot-ranked chain builders
    (lane_order = 0) and the one- and four-wave parsers at level 6."""
    name, value, default = opt
    try:
        engine.set_option(name, value)
        _check_compressed(engine, 6, "deflate-raw", "%s=%d" % (name, value))
    finally:
        engine.set_option(name, default)


# ---- decode side

DEFAULTS = {"inflate_seg": 1, "inflate_split": 1, "inflate_wave_min": 32768, "inflate_ref_wrap": 1, "inflate_fast": 1}
# path -> (options, reference_bugs of the matching oracle decode)
PATHS = {
    "default": ({}, True),  # the segmented decode for members over 4,096 input bytes, the lanes below
    "noseg": ({"inflate_seg": 0}, True),  # the wave kernel over 32,768 input bytes, the lanes below
    "wave": ({"inflate_seg": 0, "inflate_wave_min": 1, "inflate_split": 0, "inflate_ref_wrap": 0}, False),
    "split": ({"inflate_seg": 0, "inflate_wave_min": 1, "inflate_split": 1, "inflate_ref_wrap": 0}, False),
    "exact": ({"inflate_fast": 0}, True),
}


def _decode(engine, path, members, fmt, caps):
    """(results, lane count, segmented count) of one batch on a path; the options restored."""
    kw = PATHS[path][0]
    try:
        for k, v in kw.items():
            engine.set_option(k, v)
        res = engine.decompress_batch_raw(members, fmt, out_caps=caps)
        return res, engine.last_lane_count(), engine.last_seg_count()
    finally:
        for k in kw:
            engine.set_option(k, DEFAULTS[k])


@functools.lru_cache(maxsize=None)
def _oracle_decodes(members, fmt, caps, bugs):
    return tuple(oracle.decompress(m, fmt, cap=cap, reference_bugs=bugs) for m, cap in zip(members, caps))


def _check_decoded(engine, path, names, members, fmt, caps):
    res, lanes, segs = _decode(engine, path, list(members), fmt, list(caps))
    want = _oracle_decodes(tuple(members), fmt, tuple(caps), PATHS[path][1])
    for name, g, (st, out, cons, ph, msg) in zip(names, res, want):
        assert (g[0], g[1], g[2], g[4]) == (st, ph, msg, cons), (path, fmt, name, g[:3], g[4], st, ph, msg, cons)
        assert g[3] == out, (path, fmt, name, len(g[3]), len(out))
    return lanes, segs, want


def _check_paths(engine, path, names, members, fmt, caps, want, counts, leaves_fast=(), leaves_seg=()):
    """Every clean member stays on the path it is sent to, but for the named ones: each member decoded once more
    as a batch of its own tells whether a fast kernel (lanes, wave, segmented, split: last_lane_count) and whether
    the segmented decode (last_seg_count) finished it; the whole batch's counts must be the sums."""
    if path == "exact":
        assert counts == (0, 0)
        return
    left_fast, left_seg = [], []
    for name, m, cap, w in zip(names, members, caps, want):
        if w[0] != 1:
            continue
        _, fast, seg = _decode(engine, path, [m], fmt, [cap])
        if not fast:
            left_fast.append(name)
        if path == "default" and len(m) > 4096 and not seg:  # (seg_small_min: the segmented decode's members)
            left_seg.append(name)
    print("left", path, fmt, left_fast, left_seg)
    assert (left_fast, left_seg) == (list(leaves_fast), list(leaves_seg)), path
    clean = [m for m, w in zip(members, want) if w[0] == 1]
    seg = sum(1 for m in clean if len(m) > 4096) - len(left_seg) if path == "default" else 0
    assert counts == (len(clean) - len(left_fast), seg), path


# debruijn31 does not finish in the segmented decode at any level or format: the sequence's long stretches of
# the form a a x, a a y, ... are near-periodic in bits, and the chains of lanes started off a symbol boundary do
# not meet the true one inside the sync window (zs_seg.h ZS_SEG_W), as with the R-corpus stretches of
# tests/test_gpu_seg.py _runs_member; the wave kernel finishes the member with the same bytes
LEAVES_SEG = ("debruijn31",)


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_decode_of_the_oracles_members(engine, path, level):
    """The oracle's outputs of the cases: 15-bit codes in both trees, 7-bit bit-length codes, match-free blocks
    with two dummy distance codes, HLIT 286 / HDIST 30 -- status, phase, message, bytes and consumed of every
    member equal the oracle's decode, and the members stay on the path they were sent to."""
    names = [n for n, _ in hc.inputs()]
    members = hc.compressed(level)
    caps = tuple(len(d) + 16 for _, d in hc.inputs())
    lanes, segs, want = _check_decoded(engine, path, names, members, "deflate-raw", caps)
    assert all(w[0] == 1 for w in want)
    _check_paths(engine, path, names, members, "deflate-raw", caps, want, (lanes, segs),
                 leaves_seg=LEAVES_SEG if path == "default" else ())


@pytest.mark.parametrize("path", sorted(PATHS))
def test_decode_of_the_oracles_gzip_members(engine, path):
    names = [n for n, _ in hc.inputs()]
    members = hc.compressed(6, "gzip")
    caps = tuple(len(d) + 16 for _, d in hc.inputs())
    lanes, segs, want = _check_decoded(engine, path, names, members, "gzip", caps)
    _check_paths(engine, path, names, members, "gzip", caps, want, (lanes, segs),
                 leaves_seg=LEAVES_SEG if path == "default" else ())


INCOMPLETE_DISTANCE_CODE = ["repeat17_across", "repeat18_across", "one_distance_code_used",
                            "one_distance_code_unused", "hdist1_length0"]


@functools.lru_cache(maxsize=None)
def _headers():
    """(names, members, caps): every hand-built header as a tiny member and behind a 40,000-byte stored block,
    which takes the same header to the segmented, wave and split decoders."""
    pad = corpus.rand(corpus.stream_seed(40), 40000)
    names, members, caps = [], [], []
    for name, parts in bitbuild.header_cases():
        for tag, pre in (("", []), ("+stored", [("stored", pad)])):
            m, e = bitbuild.blocks(pre + parts)
            names.append(name + tag)
            members.append(m)
            caps.append(len(e) + 1024)
    return tuple(names), tuple(members), tuple(caps)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_hand_built_headers(engine, path):
    """Headers other encoders write and the reference accepts (repeat codes across the literal/distance boundary,
    one distance code, HCLEN 19, both trees complete and 15 deep, all 316 codes, 7-bit bit-length codes) and
    the reference's data errors (over-subscribed and incomplete sets, a repeat with no length before it or past
    HLIT + HDIST, no end-of-block code, HLIT 287 / 288, HDIST 31 / 32, symbols 286 / 287 and distance symbols 30 /
    31): the oracle's status, phase, message, bytes and consumed on every path; the clean members stay on it."""
    names, members, caps = _headers()
    lanes, segs, want = _check_decoded(engine, path, names, members, "deflate-raw", caps)
    assert [n for n, w in zip(names, want) if w[0] == 1] == [n + t for n in hc.HEADERS_ACCEPTED for t in ("", "+stored")]
    # the lanes and the segmented decode take complete codes only and leave a distance code that is incomplete
    # (inftrees.ts:128-139 allows a lone 1-bit code, and none at all) to the exact kernel; the wave and split
    # decoders build it themselves
    tiny = [n for n in INCOMPLETE_DISTANCE_CODE]
    padded = [n + "+stored" for n in INCOMPLETE_DISTANCE_CODE]
    leaves_fast = {"default": tiny, "noseg": tiny}.get(path, [])
    _check_paths(engine, path, names, members, "deflate-raw", caps, want, (lanes, segs),
                 leaves_fast=sorted(leaves_fast, key=names.index), leaves_seg=padded if path == "default" else ())
