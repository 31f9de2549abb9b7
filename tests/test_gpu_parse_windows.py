"""GPU: pass A of the lazy parse stages its match-table windows cooperatively (deflate_parse.hip):
the lanes of a wave load each other's windows, a piece each, and the input byte of every entry
rides in the staged entry.  The outputs are compared byte for byte with the C oracle
(tests/oracle.py); the `_dict`, `_filt` and `_par` instances, which the oracle does not compress
for, with the committed goldens of their case helpers.

The shapes are the smallest at which the staging can go wrong: lengths around the window, the
segment and the table-row edges, one stream with a second round of 64 segments; content that
keeps the lanes of a wave at different places (258-byte jumps, every entry visited, text, all of
them in one stream); streams at every byte offset mod 4 of the packed input."""
import functools

import pytest

import corpus
import deflate_header
import oracle

LENS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 1024 + 258, 2047, 2048, 2049, 65535, 65536]
LENS += list(range(4092, 4100))  # every n mod 8: the table's rows are rounded to 8 entries
LENS += [70000]  # 69 segments of 1,024 positions: a second round in the one-wave instance
KINDS = ["zeros", "runs", "rand", "text", "patchwork"]
LEVELS = [4, 6, 9]
WAVES = [1, 2, 4]
FMT = "deflate-raw"


def runs(seed, n):
    """runs of 1 .. 700 equal bytes, bytes >= 0x80 among them: matches of 258 and short tails"""
    r = corpus._xs(seed)
    out = bytearray()
    while len(out) < n:
        a = next(r)
        out += bytes([a & 0xFF]) * (1 + (a >> 8) % 700)
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def content(kind, n):
    seed = corpus.stream_seed(7000 + n)
    if kind == "zeros":
        return bytes(n)
    if kind == "runs":
        return runs(seed, n)
    if kind == "rand":
        return corpus.rand(seed, n)
    if kind == "text":
        return corpus.text(seed, n)
    return corpus.patchwork(n, n)


@functools.lru_cache(maxsize=None)
def batch(kind):
    return tuple(content(kind, n) for n in LENS)


@functools.lru_cache(maxsize=None)
def want(kind, level):
    """the oracle's bytes for batch(kind): computed once, shared by the instances"""
    return tuple(reference(x, level) for x in batch(kind))


def reference(x, level):
    st, out, _ = oracle.compress(x, level, FMT)
    assert st == oracle.Z_STREAM_END
    return out


def copies(out):
    return [s for b in deflate_header.parse(out) for s in b.symbols if s[0] == "copy"]


def test_the_inputs_reach_the_paths_they_are_meant_for():
    """CPU: zeros and runs parse into matches of 258 (lanes that leave a window after one entry),
    random bytes into no match at all (every entry of every window is visited)"""
    for n in (1024 + 258, 4096, 65536):
        z = copies(reference(content("zeros", n), 6))
        assert z and all(s[2] == 1 for s in z) and sum(s[1] == 258 for s in z) == (n - 1) // 258
    r = copies(reference(content("runs", 65536), 6))
    assert sum(s[1] == 258 for s in r) > 50 and sum(s[1] < 258 for s in r) > 50
    for n in (33, 1025, 4097, 65536):
        x = content("rand", n)
        assert copies(reference(x, 6)) == []
    # bytes >= 0x80 (bit 7 is packed apart) before a window's first entry and at its last slot
    assert any(x[i] >= 0x80 for i in range(3, len(x), 4)) and any(x[i] >= 0x80 for i in range(31, len(x), 32))
    assert copies(reference(content("text", 4096), 6))


def compress(engine, xs, level, waves, **kw):
    try:
        engine.set_option("parse_waves", waves)
        return engine.compress_batch(list(xs), FMT, level, **kw)
    finally:
        engine.set_option("parse_waves", 0)


def first_mismatch(got, ref, xs):
    for i, (g, w) in enumerate(zip(got, ref)):
        if g != w:
            return "stream %d (%d bytes): %d bytes out, the oracle %d" % (i, len(xs[i]), len(g), len(w))
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_length_equals_the_oracle(engine, kind, waves, level):
    xs = batch(kind)
    assert first_mismatch(compress(engine, xs, level, waves), want(kind, level), xs) is None


PLACED_LENS = [1, 2, 3, 4, 5, 31, 33, 64, 1023, 1025, 2049, 4093, 4098]


@functools.lru_cache(maxsize=None)
def placed(k):
    """streams of rand, text and runs, each at a byte offset = k (mod 4) of the packed input (the
    engine packs a batch's inputs back to back): a filler of 1 .. 4 bytes in front of each"""
    xs, at, off = [], [], 0
    for kind in ("rand", "text", "runs"):
        for n in PLACED_LENS:
            pad = (k - off) % 4 or 4
            xs.append(content("rand", 8)[:pad])
            off += pad
            assert off % 4 == k
            at.append(len(xs))
            xs.append(content(kind, n))
            off += n
    return tuple(xs), tuple(at)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_streams_at_every_offset_mod_4(engine, k, waves):
    xs, at = placed(k)
    assert len(at) == 3 * len(PLACED_LENS)
    ref = [reference(x, 6) for x in xs]
    assert first_mismatch(compress(engine, xs, 6, waves), ref, xs) is None


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_preset_dictionary_instances(engine, waves):
    """the `_dict` instances: the window, slide and block corners behind dictionaries of 32,768, 32,767 and 257 bytes"""
    import deflatedictcases as cases
    import zsamd

    b = cases.set2(6)
    try:
        engine.set_option("parse_waves", waves)
        res = engine.compress_batch_detailed([c[1] for c in b], FMT, 6, zdict=[c[2] for c in b])
    finally:
        engine.set_option("parse_waves", 0)
    g = cases.golden()
    for (name, x, d, level, fmt), (st, out, chk) in zip(b, res):
        assert st == zsamd.Z_STREAM_END, (name, st)
        assert cases.digest(out) == g[name], (name, len(out), g[name])


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_filtered_instances(engine, waves):
    """the `_filt` instances: Z_FILTERED at level 6"""
    import strategycases as cases
    import zsamd

    b = cases.filtered_cases(6)
    try:
        engine.set_option("parse_waves", waves)
        res = engine.compress_batch_detailed([c[1] for c in b], FMT, 6, strategy=cases.Z_FILTERED)
    finally:
        engine.set_option("parse_waves", 0)
    g = cases.golden()
    for c, (st, out, chk) in zip(b, res):
        assert st == zsamd.Z_STREAM_END, (c[0], st)
        assert cases.digest(out) == g[c[0]], (c[0], len(out), g[c[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("waves", WAVES)
def test_window_bits_instances(engine, waves):
    """the `_par` build: a 4 KiB window at memLevel 4 (slides, the NIL corner, 200,000 bytes of text)"""
    import paramcases as cases
    import zsamd

    b = [c for name in ("slide", "dist", "long") for c in cases.group(name) if c[2:5] == (6, FMT, 12)]
    assert {c[0].split("/")[0] for c in b} == {"slide", "dist", "long"}
    g = cases.golden()
    for call in cases.by_call(b):
        _, _, level, fmt, wb, ml = call[0]
        try:
            engine.set_option("parse_waves", waves)
            res = engine.compress_batch_detailed([c[1] for c in call], fmt, level, window_bits=wb, mem_level=ml)
        finally:
            engine.set_option("parse_waves", 0)
        assert len(call) >= 1
        for c, (st, out, chk) in zip(call, res):
            assert st == zsamd.Z_STREAM_END, (c[0], st)
            assert cases.digest(out) == g[c[0]], (c[0], len(out), g[c[0]])
