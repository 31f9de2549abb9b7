"""GPU: decoding members compressed with a preset dictionary (zs_inflate_batch_dict*,
raw deflate and zlib).  Inputs come from the system zlib (dictcases); every member
but the large one is single-call, so the expected bytes are the plaintext and the
dictionary lane instances must decode them (zs_last_inflate_lane_count)."""
import ctypes
import zlib

import pytest

import corpus
import dictcases

pytestmark = pytest.mark.gpu

FMTS = ["deflate-raw", "deflate"]
TOO_FAR = "invalid distance too far back"


def want_check(fmt, s):
    return zlib.adler32(s) if fmt == "deflate" else 0


def device_run(engine, fmt, comps, caps, dblob, doffs, dlens, lead=3):
    """zs_inflate_batch_dict_device over torch buffers: the dictionary bytes `lead`
    bytes into their buffer (an odd offset), every output region between canaries.
    Returns ([(status, phase, msg, bytes, consumed, check)], lane count, bytes outside the regions unchanged)."""
    import torch
    import zsamd

    n = len(comps)
    offs, o = [], 0
    for c in comps:
        offs.append(o)
        o += len(c)
    ooffs, oo = [], 16
    for c in caps:
        ooffs.append(oo)
        oo += c + 16  # 16 canary bytes between the regions (offsets stay multiples of 4)
    d_in = torch.frombuffer(bytearray(b"".join(comps) + b"\0" * 16), dtype=torch.uint8).cuda()
    d_dict = torch.frombuffer(bytearray(b"\xee" * lead + dblob + b"\xee" * 16), dtype=torch.uint8).cuda()
    d_out = torch.full((oo,), 0xa5, dtype=torch.uint8, device="cuda")
    res = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(6)]
    engine.decompress_device(fmt, n, d_in.data_ptr(), (ctypes.c_uint64 * n)(*offs),
                             (ctypes.c_uint32 * n)(*[len(c) for c in comps]), d_out.data_ptr(),
                             (ctypes.c_uint64 * n)(*ooffs), (ctypes.c_uint32 * n)(*caps),
                             *[r.data_ptr() for r in res[:5]], 0, d_dict.data_ptr(),
                             (ctypes.c_uint64 * n)(*[x + lead for x in doffs]), (ctypes.c_uint32 * n)(*dlens),
                             res[5].data_ptr())
    torch.cuda.synchronize()
    lanes = engine.last_lane_count()
    st, ph, ms, ol, co, ck = [r.tolist() for r in res]
    raw = bytes(d_out.cpu().numpy())
    inside = bytearray(len(raw))
    for a, c in zip(ooffs, caps):
        inside[a:a + c] = b"\1" * c
    clean = all(b == 0xa5 for b, i in zip(raw, inside) if not i)
    L = zsamd.lib()
    out = [(st[i], ph[i], L.zs_inflate_message(ms[i]).decode(), raw[ooffs[i]:ooffs[i] + ol[i]], co[i],
            ck[i] & 0xffffffff) for i in range(n)]
    return out, lanes, clean


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("L", dictcases.DICT_LENS)
def test_shared_dictionary(engine, L, fmt):
    d = dictcases.dictionary(L)
    ms = dictcases.members(L, fmt)
    comps = [c for c, _ in ms]
    caps = [dictcases.cap4(len(s)) for _, s in ms]
    n = len(ms)
    # the host entry
    res = engine.decompress_batch_detailed(comps, fmt, caps, zdict=d)
    lanes = engine.last_lane_count()
    for i, ((c, s), (st, ph, msg, out, cons, chk)) in enumerate(zip(ms, res)):
        assert (st, ph, msg) == (1, 0, ""), (i, st, ph, msg)
        assert out == s and cons == len(c) and chk == want_check(fmt, s), i
    assert lanes == n  # the fast path decoded them: a fallback to the exact kernel fails here
    # the device entry: the dictionary at an odd byte offset, canaries around every region
    res, lanes, clean = device_run(engine, fmt, comps, caps, d, [0] * n, [L] * n)
    for i, ((c, s), (st, ph, msg, out, cons, chk)) in enumerate(zip(ms, res)):
        assert (st, ph, msg, out, cons, chk) == (1, 0, "", s, len(c), want_check(fmt, s)), i
    assert lanes == n
    assert clean, "a byte outside [out_off, out_off + out_cap) changed"


@pytest.mark.parametrize("fmt", FMTS)
def test_per_member_dictionaries(engine, fmt):
    """three dictionaries, aliased among the members; members without one (dict_len 0)"""
    ds = [dictcases.dictionary(257, 900), dictcases.dictionary(3001, 901), dictcases.dictionary(32768, 902), None]
    zd, comps, srcs = [], [], []
    for i in range(96):
        d = ds[(i * 7 + i // 5) % 4]
        s = dictcases.record(i % 64)
        zd.append(d)
        srcs.append(s)
        comps.append(dictcases.compress(s, dictcases.LEVELS[i % 3], fmt, d))
    caps = [dictcases.cap4(len(s)) for s in srcs]
    res = engine.decompress_batch_detailed(comps, fmt, caps, zdict=zd)
    assert engine.last_lane_count() == len(comps)
    for i, (s, c, r) in enumerate(zip(srcs, comps, res)):
        assert r == (1, 0, "", s, len(c), want_check(fmt, s)), i
    # the device entry with explicit offsets: dictionaries back to back, none = (0, 0)
    pos, blob = {}, b""
    for d in ds[:3]:
        pos[d] = len(blob)
        blob += d
    res, lanes, clean = device_run(engine, fmt, comps, caps, blob, [pos[d] if d else 0 for d in zd],
                                   [len(d) if d else 0 for d in zd], lead=1)
    assert lanes == len(comps) and clean
    for i, (s, c, r) in enumerate(zip(srcs, comps, res)):
        assert r == (1, 0, "", s, len(c), want_check(fmt, s)), i


@pytest.mark.parametrize("L", dictcases.DICT_LENS)
def test_hand_built_copies_on_the_boundary(engine, L):
    d = dictcases.dictionary(L)
    cases = dictcases.hand_built(L)
    names = sorted(cases) * 16  # (a batch of at least 48 members)
    comps = [cases[k][0] for k in names]
    caps = [dictcases.cap4(len(cases[k][1] or b"") + 8) for k in names]
    res = engine.decompress_batch_detailed(comps, "deflate-raw", caps, zdict=d)
    lanes = engine.last_lane_count()
    for k, m, (st, ph, msg, out, cons, chk) in zip(names, comps, res):
        exp = cases[k][1]
        if exp is None:
            assert (st, msg, out) == (-3, TOO_FAR, b""), (L, k, st, msg)
        else:
            assert (st, ph, msg, out, cons, chk) == (1, 0, "", exp, len(m), 0), (L, k, st, msg)
    assert lanes == sum(1 for k in names if cases[k][1] is not None)


def test_statuses(engine):
    import zsamd

    d, other = dictcases.dictionary(257), dictcases.dictionary(257, seed=901)
    srcs = [dictcases.record(i) for i in range(64)]
    caps = [dictcases.cap4(len(s)) for s in srcs]
    withd = [dictcases.compress(s, 6, "deflate", d) for s in srcs]
    plain = [dictcases.compress(s, 6, "deflate") for s in srcs]
    # the wrong dictionary: inflateSetDictionary returns Z_DATA_ERROR, no message, nothing produced
    res = engine.decompress_batch_detailed(withd, "deflate", caps, zdict=other)
    assert all(r[:4] == (-3, zsamd.PHASE_PROCESS, "", b"") for r in res), res[0]
    assert all(r[5] == 0 for r in res)
    # FDICT without a dictionary: exactly zs_inflate_batch's answer (Z_NEED_DICT)
    base = engine.decompress_batch_detailed(withd, "deflate", caps)
    assert all(r[0] == 2 for r in base)
    assert engine.decompress_batch_detailed(withd, "deflate", caps, zdict=[None] * 64) == base
    assert engine.decompress_batch_detailed(withd, "deflate", caps, zdict=[d if i % 2 else None for i in range(64)]) \
        == [(1, 0, "", srcs[i], len(withd[i]), zlib.adler32(srcs[i])) if i % 2 else base[i] for i in range(64)]
    # FDICT clear, a dictionary given: ignored, every result array as zs_inflate_batch's
    base = engine.decompress_batch_detailed(plain, "deflate", caps)
    assert [r[0] for r in base] == [1] * 64
    assert engine.decompress_batch_detailed(plain, "deflate", caps, zdict=d) == base
    # gzip and deflate64-raw with a dictionary: the call fails
    for fmt in ("gzip", "deflate64-raw"):
        with pytest.raises(zsamd.ZsError) as e:
            engine.decompress_batch_detailed(plain, fmt, caps, zdict=d)
        assert e.value.status == zsamd.Z_STREAM_ERROR
        # ... but not when no member has one
        engine.decompress_batch_detailed(plain[:2], fmt, caps[:2], zdict=[None, b""])
    # capacity 4 bytes short: what zs_inflate_batch gives a member without a dictionary
    short = [c - 4 for c in caps]
    for fmt, a, b in (("deflate", withd, plain),
                      ("deflate-raw", [dictcases.compress(s, 6, "deflate-raw", d) for s in srcs],
                       [dictcases.compress(s, 6, "deflate-raw") for s in srcs])):
        got = engine.decompress_batch_detailed(a, fmt, short, zdict=d)
        ref = engine.decompress_batch_detailed(b, fmt, short)
        assert [r[:4] for r in got] == [r[:4] for r in ref]
        assert all(r[0] != 1 for r in got)


def test_options_leave_bytes_unchanged(engine):
    d = dictcases.dictionary(32767)
    for fmt in FMTS:
        ms = dictcases.members(32767, fmt, n=128)
        comps = [c for c, _ in ms] + [dictcases.hand_built(32767)["too_far"][0]] * (fmt == "deflate-raw")
        caps = [dictcases.cap4(len(s)) for _, s in ms] + [16] * (fmt == "deflate-raw")
        base = engine.decompress_batch_detailed(comps, fmt, caps, zdict=d)
        assert [r[3] for r in base[:128]] == [s for _, s in ms]
        for name, value, default, lanes in (("inflate_fast", 0, 1, 0), ("lane_block", 1, 0, 128),
                                            ("lane_block", 64, 0, 128), ("inflate_wave_min", 0, 32768, 128)):
            engine.set_option(name, value)
            try:
                got = engine.decompress_batch_detailed(comps, fmt, caps, zdict=d)
                assert engine.last_lane_count() == lanes, (name, value)
            finally:
                engine.set_option(name, default)
            assert got == base, (fmt, name, value)


def test_large_member_takes_the_exact_kernel(engine):
    d = dictcases.dictionary(40000)
    big = corpus.mixed(corpus.stream_seed(77), 200003)
    for fmt in FMTS:
        ms = dictcases.members(40000, fmt, n=63)
        comps = [c for c, _ in ms] + [dictcases.compress(big, 6, fmt, d)]
        caps = [dictcases.cap4(len(s)) for _, s in ms] + [200004]
        assert len(comps[-1]) > 32768  # more than one input sub-chunk
        engine.set_option("inflate_ref_wrap", 0)
        try:
            res = engine.decompress_batch_detailed(comps, fmt, caps, zdict=d)
            lanes = engine.last_lane_count()
        finally:
            engine.set_option("inflate_ref_wrap", 1)
        assert res[-1] == (1, 0, "", big, len(comps[-1]), want_check(fmt, big))
        assert [r[3] for r in res[:-1]] == [s for _, s in ms]
        assert lanes == 63  # the large member is not the lane kernel's
        # the reference's calls emulated (window-wrap copy included): status and lengths only
        res = engine.decompress_batch_detailed(comps, fmt, caps, zdict=d)
        assert engine.last_lane_count() == 63
        st, ph, msg, out, cons, chk = res[-1]
        assert (st, len(out), cons) == (1, len(big), len(comps[-1])), (fmt, st, ph, msg)
        assert [r[3] for r in res[:-1]] == [s for _, s in ms]


def test_auto_and_pool_match_the_bounded_call(engine):
    import zsamd

    d = dictcases.dictionary(3001, 901)
    for fmt in FMTS:
        ms = dictcases.members(3001, fmt, n=96, seed=901)
        comps = [c for c, _ in ms]
        zd = [d if i % 5 else None for i in range(96)]  # (every fifth: FDICT without one / distance too far back)
        caps = [dictcases.cap4(len(s)) for _, s in ms]
        base = engine.decompress_batch_detailed(comps, fmt, caps, zdict=zd)
        assert [r[3] for i, r in enumerate(base) if i % 5] == [s for i, (_, s) in enumerate(ms) if i % 5]
        assert engine.decompress_batch_detailed(comps, fmt, None, zdict=zd) == base
        pool = zsamd.Pool([0, 0], repeat=True)
        try:
            assert pool.decompress_batch_detailed(comps, fmt, caps, zdict=zd) == base
            assert pool.decompress_batch_detailed(comps, fmt, None, zdict=zd) == base
        finally:
            pool.close()
