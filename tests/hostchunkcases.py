"""The harness of the host entries' chunk tests (test_gpu_host_chunks.py): batches whose seams between
the four chunks of capi.cpp's host_batch_run carry the edge members, host calls on caller-owned
memory with a canary pattern between the output regions, the oracle's bytes per distinct (content,
parameters), and the comparison of a chunked call with the same call unchunked and with its four
ranges issued as four calls.

A host batch of at least 64 streams and "host_chunk_min" input bytes runs as four chunks of streams,
[bnd[k], bnd[k + 1]) with bnd = bounds(n); chunked(engine) lowers the option to 1 byte."""
import contextlib
import ctypes
import functools
import zlib

import corpus
import dictcases
import flushcases
import oracle
import paramcases
import strategycases

DEFAULTS = {"host_chunk_min": 33554432, "host_pack_min": 67108864, "checksum_split": 1 << 18,
            "checksum_part": 65536, "rle_ref": 1, "inflate_ref_wrap": 1}
SIZES = (64, 67, 71)  # the stream counts of the route matrix; 520 once per direction
Z_FULL_FLUSH = 3


def bounds(n):
    return [0, n // 8, n // 2, 7 * n // 8, n]


def chunk_of(n, i):
    b = bounds(n)
    return max(k for k in range(4) if b[k] <= i)


def seams(n):
    """the last member of a chunk and the first of the next, for the three cuts"""
    b = bounds(n)
    return [b[k] - 1 + j for k in (1, 2, 3) for j in (0, 1)]


@contextlib.contextmanager
def options(engine, **kw):
    """the engine with these options; their defaults again afterwards"""
    try:
        for k, v in kw.items():
            engine.set_option(k, v)
        yield engine
    finally:
        for k in kw:
            engine.set_option(k, DEFAULTS[k])


def chunked(engine, min_bytes=1):
    """the engine with host_chunk_min = min_bytes (0: never); the default again afterwards"""
    return options(engine, host_chunk_min=min_bytes)


# ------------------------------------------------------------------ the members
def _text(i, n):
    return corpus.text(corpus.stream_seed(7000 + i), n)


@functools.lru_cache(maxsize=None)
def edges():
    """the seam slots' members: empty, one byte, a word short of 4 KiB, the sweep's one-window limit and a byte
    more, a stored block, a long run"""
    return (b"", b"Z", _text(1, 4095), _text(2, 65536), _text(3, 65537), corpus.rand(77, 300), bytes(40000))


@functools.lru_cache(maxsize=None)
def fillers():
    """16 distinct contents, lengths pairwise different, about 1 .. 9 KiB, none a multiple of 4: packed one
    behind the other they start at every byte residue"""
    out = []
    for k in range(16):
        n = 1021 + 531 * k
        n += n % 4 == 0
        seed = corpus.stream_seed(7100 + k)
        if k >= 14:
            out.append(corpus.mixed(seed, n))  # (past 8,192 bytes: a stretch of random bytes inside)
        elif k % 3 == 0:
            out.append(corpus.text(seed, n))
        elif k % 3 == 1:
            out.append(corpus.rand(seed, n))
        else:
            out.append(corpus.patchwork(7100 + k, n))
    lens = [len(b) for b in out]
    assert len(set(lens)) == 16 and all(n % 4 for n in lens) and {n % 4 for n in lens} == {1, 2, 3}
    assert len(set(out)) == 16 and min(lens) == 1021 and max(lens) < 9216
    return tuple(out)


def filler_at(i, shift=0):
    """slot i's filler: neighbours differ, and so do slots 8, n / 8, n / 2 - n / 8 ... apart (a view that is
    off by one stream or one chunk reads another content)"""
    return fillers()[(3 * i + i // 16 + shift) % 16]


def batch(n, shift=0):
    """n members: the edge members on the seam slots (cycled, from `shift` on), fillers elsewhere"""
    s, e = seams(n), edges()
    return [e[(s.index(i) + shift) % len(e)] if i in s else filler_at(i, shift) for i in range(n)]


# ------------------------------------------------------------------ expected values, once per distinct input
@functools.lru_cache(maxsize=None)
def deflated(data, fmt, level, zdict=None, strategy=0, params=None, flush=None):
    """the oracle's bytes.  params: (window_bits, mem_level); flush: the positions (a tuple).  Level 0: the C
    oracle does not restate deflate_stored; zlib fed in the stream layer's 32 KiB calls (paramcases.compress)
    writes the reference's level-0 bytes (it reproduces every case of tests/golden/deflate_level0.json)"""
    if level == 0 and not (flush or params or strategy or zdict):
        params = (15, 8)
    if flush:
        return flushcases.compress(data, level, fmt, flush)
    if params is not None:
        return paramcases.compress(data, level, fmt, *params)
    if strategy:
        return strategycases.compress(data, level, fmt, strategy)
    if zdict:
        return dictcases.compress(data, level, fmt, zdict)
    st, out, _ = oracle.compress(data, level, fmt)
    assert st == 1
    return out


@functools.lru_cache(maxsize=None)
def deflate_check(data, fmt):
    """strm.adler behind the stream"""
    return zlib.adler32(data) if fmt == "deflate" else zlib.crc32(data) if fmt == "gzip" else 1


@functools.lru_cache(maxsize=None)
def flush_parts(data, fmt, level, flush):
    return tuple(len(p) for p in flushcases.parts(data, level, fmt, flush))


def flush_index(data, fmt, level, flush):
    """the offsets behind the markers: running sums of flushcases.parts, the header in the first"""
    out, at = [], 0
    for ln in flush_parts(data, fmt, level, tuple(flush))[:-1]:
        at += ln
        out.append(at)
    return out


@functools.lru_cache(maxsize=None)
def inflated(member, fmt, cap, ref_wrap=True):
    """(status, phase, message, bytes, consumed) by the oracle"""
    st, out, cons, ph, msg = oracle.decompress(member, fmt, cap=max(cap, 1), reference_bugs=ref_wrap)
    if cap == 0 and out:
        raise AssertionError("capacity 0 is not modelled")
    return st, ph, msg, out, cons


def inflate_check(data, fmt):
    return zlib.adler32(data) if fmt == "deflate" else zlib.crc32(data) if fmt == "gzip" else 0


# ------------------------------------------------------------------ host calls on caller-owned memory
_PERIOD = bytes((37 * p + 11) & 0xFF for p in range(256))


def canary(n):
    return (_PERIOD * (n // 256 + 1))[:n]


def regions(caps):
    """output offsets with odd gaps: region i starts 1, 3, 5 or 7 bytes behind region i - 1's end"""
    offs, at = [], 0
    for i, c in enumerate(caps):
        at += 1 + 2 * (i % 4)
        offs.append(at)
        at += c
    return offs, at + 9


def _u32(v):
    return (ctypes.c_uint32 * max(1, len(v)))(*v)


def _u64(v):
    return (ctypes.c_uint64 * max(1, len(v)))(*v)


def _inputs(items):
    """the inputs one behind the other, behind a prefix of one byte"""
    offs, at = [], 1
    for b in items:
        offs.append(at)
        at += len(b)
    return b"\xa5" + b"".join(items), offs


def _dicts(zdict):
    """(blob, offsets, lengths): equal dictionaries stored once, behind a prefix of three bytes"""
    parts, at, offs, lens, o = [b"\x00\x01\x02"], {}, [], [], 3
    for d in zdict:
        d = d or b""
        if d and d not in at:
            at[d] = o
            parts.append(d)
            o += len(d)
        offs.append(at[d] if d else 0)
        lens.append(len(d))
    return b"".join(parts), _u64(offs), _u32(lens)


def _pairs(per):
    first, flat = [0], []
    for ps in per:
        flat.extend(ps or [])
        first.append(len(flat))
    return first, flat


def _collect(engine, rc, what, out, total, offs, lens):
    """the call's return code, then the output buffer: the streams' bytes, and nothing else changed"""
    if rc != 0:
        raise AssertionError("%s returned %d: %s" % (what, rc, engine._L.zs_last_error().decode()))
    raw = out.raw
    want = bytearray(canary(total))
    data = []
    for o, ln in zip(offs, lens):
        data.append(raw[o:o + ln])
        want[o:o + ln] = raw[o:o + ln]
    if raw != bytes(want):
        bad = next(p for p in range(total) if raw[p] != want[p])
        i = max((k for k in range(len(offs)) if offs[k] <= bad), default=-1)
        raise AssertionError("%s: byte %d changed outside the produced bytes (stream %d: offset %d, %d bytes)"
                             % (what, bad, i, offs[i] if i >= 0 else 0, lens[i] if i >= 0 else 0))
    return data


def deflate(engine, items, fmt, level, caps=None, zdict=None, strategy=None, params=None, flush=None):
    """One host compress call, outputs to regions with odd gaps and a canary between them.
    caps: the capacities (default: the entry's bound, exactly); zdict: one dictionary or None per stream
    (the _dict entry); strategy: the _strategy entry; params: (window_bits, mem_level), the _params entry;
    flush: one position list per stream (the _flush entry).  Returns the result arrays and the bytes."""
    L, n = engine._L, len(items)
    wb = engine_wbits(fmt) if params is None else paramcases.wbits_code(fmt, params[0])
    if caps is None:
        if flush is not None:
            caps = [int(L.zs_deflate_bound_flush(len(b), wb, len(flush[i] or []))) for i, b in enumerate(items)]
        elif params is not None:
            caps = [int(L.zs_deflate_bound_params(len(b), wb, params[1], level)) for b in items]
        elif zdict is not None:
            caps = [int(L.zs_deflate_bound_dict(len(b), wb, len(zdict[i] or b""))) for i, b in enumerate(items)]
        else:
            caps = [int(L.zs_deflate_bound(len(b), wb)) for b in items]
    blob, ioffs = _inputs(items)
    offs, total = regions(caps)
    out = ctypes.create_string_buffer(canary(total), total)
    status, olen, chk = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    for a in (status, olen, chk):
        ctypes.memset(a, 0x5A, 4 * n)
    tail = (blob, _u64(ioffs), _u32([len(b) for b in items]), out, _u64(offs), _u32(caps), status, olen, chk)
    h = engine.handle
    if flush is not None:
        first, pos = _pairs(flush)
        rc, what = L.zs_deflate_batch_flush(h, level, wb, n, *tail, Z_FULL_FLUSH, _u64(first), _u32(pos)), "flush"
    elif params is not None:
        rc, what = L.zs_deflate_batch_params(h, level, wb, params[1], n, *tail), "params"
    elif strategy is not None:
        rc, what = L.zs_deflate_batch_strategy(h, level, strategy, wb, n, *tail), "strategy"
    elif zdict is not None:
        rc, what = L.zs_deflate_batch_dict(h, level, wb, n, *tail, *_dicts(zdict)), "dict"
    else:
        rc, what = L.zs_deflate_batch_ex(h, level, wb, n, *tail), "deflate"
    data = _collect(engine, rc, "zs_deflate_batch_" + what, out, total, offs, list(olen))
    return {"status": list(status), "len": list(olen), "check": list(chk), "data": data}


def engine_wbits(fmt):
    return {"deflate-raw": -15, "deflate": 15, "gzip": 31, "deflate64-raw": -16}[fmt]


def inflate(engine, items, fmt, caps, zdict=None, restart=None):
    """One host decode call (zs_inflate_batch_ex, _dict or _restart), outputs as deflate()'s.  restart: one list
    of (in_pos, out_pos) per stream WITH its start.  Returns the result arrays and the bytes."""
    L, n = engine._L, len(items)
    blob, ioffs = _inputs(items)
    offs, total = regions(caps)
    out = ctypes.create_string_buffer(canary(total), total)
    res = [(ctypes.c_int32 * n)() for _ in range(3)] + [(ctypes.c_uint32 * n)() for _ in range(3)]
    for a in res:
        ctypes.memset(a, 0x5A, 4 * n)
    args = (engine.handle, engine_wbits(fmt), n, blob, _u64(ioffs), _u32([len(b) for b in items]), out, _u64(offs),
            _u32(caps), *res)
    if restart is not None:
        first, flat = _pairs(restart)
        rc, what = L.zs_inflate_batch_restart(*args, _u64(first), _u32([a for a, _ in flat]),
                                              _u32([b for _, b in flat])), "restart"
    elif zdict is not None:
        rc, what = L.zs_inflate_batch_dict(*args, *_dicts(zdict)), "dict"
    else:
        rc, what = L.zs_inflate_batch_ex(*args), "ex"
    status, phase, msg, olen, cons, chk = res
    data = _collect(engine, rc, "zs_inflate_batch_" + what, out, total, offs, list(olen))
    return {"status": list(status), "phase": list(phase), "msg": [L.zs_inflate_message(m).decode() for m in msg],
            "len": list(olen), "consumed": list(cons), "check": list(chk), "data": data}


def inflate_auto(engine, items, fmt, zdict=None):
    """zs_inflate_batch_auto / _dict_auto: the entry's own buffer and offsets"""
    L, n = engine._L, len(items)
    blob, ioffs = _inputs(items)
    res = [(ctypes.c_int32 * n)() for _ in range(3)] + [(ctypes.c_uint32 * n)() for _ in range(3)]
    ooffs, outp = (ctypes.c_uint64 * n)(), ctypes.c_void_p()
    args = (engine.handle, engine_wbits(fmt), n, blob, _u64(ioffs), _u32([len(b) for b in items]), ctypes.byref(outp),
            ooffs, *res)
    rc = L.zs_inflate_batch_auto(*args) if zdict is None else L.zs_inflate_batch_dict_auto(*args, *_dicts(zdict))
    if rc != 0:
        raise AssertionError("zs_inflate_batch_auto returned %d: %s" % (rc, L.zs_last_error().decode()))
    status, phase, msg, olen, cons, chk = res
    try:
        data = [ctypes.string_at(outp.value + ooffs[i], olen[i]) if olen[i] else b"" for i in range(n)]
    finally:
        L.zs_free(outp)
    return {"status": list(status), "phase": list(phase), "msg": [L.zs_inflate_message(m).decode() for m in msg],
            "len": list(olen), "consumed": list(cons), "check": list(chk), "data": data}


# ------------------------------------------------------------------ the comparison of the three ways
def first_difference(a, b):
    for key in a:
        if a[key] != b[key]:
            i = next((i for i, (x, y) in enumerate(zip(a[key], b[key])) if x != y), min(len(a[key]), len(b[key])))
            x, y = a[key][i], b[key][i]
            if key == "data":
                x, y = (len(x), x[:16].hex()), (len(y), y[:16].hex())
            return "%s[%d]: %r != %r" % (key, i, x, y)
    return None


def three_ways(engine, n, run, counters=None):
    """run(a, b): streams [a, b) as one host call, its result.  The call chunked (four chunks, asserted), the
    same call with host_chunk_min = 0 (one chunk) and the four ranges as four calls: the bytes and the result
    arrays must be identical, and counters() -- figures that go on over a call's chunks -- must be, after
    the chunked call, the sum over the four calls.  Returns the chunked call's result and counters."""
    bnd = bounds(n)
    with chunked(engine, 1):
        whole = run(0, n)
        assert engine.last_host_chunks() == 4, "the call did not run as four chunks"
        cw = counters() if counters else ()
    with chunked(engine, 0):
        one = run(0, n)
        assert engine.last_host_chunks() == 1
        parts, cs = [], []
        for k in range(4):
            parts.append(run(bnd[k], bnd[k + 1]))
            assert engine.last_host_chunks() == 1
            cs.append(counters() if counters else ())
    d = first_difference(whole, one)
    assert d is None, "chunked call != unchunked call: " + d
    joined = {key: [x for p in parts for x in p[key]] for key in whole}
    d = first_difference(whole, joined)
    assert d is None, "chunked call != four calls: " + d
    if counters:
        assert tuple(cw) == tuple(sum(c[j] for c in cs) for j in range(len(cw))), (cw, cs)
    return whole, cw


def check_deflate(res, items, fmt, want, ok=None):
    """every stream against the oracle: status, length, check value, bytes.  want[i]: the expected bytes;
    ok[i] False: a stream whose capacity is short (Z_BUF_ERROR: status -5, length 0, no bytes)"""
    for i, (d, w) in enumerate(zip(items, want)):
        got = (res["status"][i], res["len"][i], res["data"][i])
        if ok is not None and not ok[i]:
            assert got == (-5, 0, b""), (i, got[:2])
            continue
        assert got[:2] == (1, len(w)), (i, len(d), got[:2], len(w))
        assert got[2] == w, (i, len(d), "bytes differ at %d" % next(k for k in range(len(w)) if w[k] != got[2][k]))
        assert res["check"][i] == deflate_check(d, fmt), (i, len(d))


def check_inflate(res, want, fmt):
    """every stream against want[i] = (status, phase, message, bytes, consumed; consumed None: any): all result
    arrays; the check value of a stream that ended is the checksum of its bytes"""
    for i, w in enumerate(want):
        got = (res["status"][i], res["phase"][i], res["msg"][i], res["data"][i], res["consumed"][i])
        if w[4] is None:  # (a consumed count that nothing specifies)
            w = w[:4] + (got[4],)
        assert got[:3] + got[4:] == w[:3] + w[4:], (i, got[:3], got[4], w[:3], w[4])
        assert res["len"][i] == len(w[3]) and got[3] == w[3], (i, res["len"][i], len(w[3]))
        if w[0] == 1:
            assert res["check"][i] == inflate_check(w[3], fmt), i
