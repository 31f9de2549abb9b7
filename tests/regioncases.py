"""The harness of the region tests (test_gpu_inflate_regions.py, test_gpu_deflate_regions.py): a batch
through a device entry over torch buffers laid out so that the three promises of include/zs_gpu.h can
be seen to hold --

* "no store leaves [out_off[i], out_off[i] + out_cap[i])": the output buffer is 0xa5 everywhere, the
  first region starts at offset 4, the gaps between regions cycle through 4, 8, 12 and 20 bytes (so
  out_off mod 16 takes every residue and the narrowest canary is one dword) and 64 bytes follow the
  last region; `dirty` lists the bytes outside the regions that changed;
* "inputs may be packed at any byte offset": one byte of filler leads the input buffer (odd offsets),
  0, 1, 3 or 7 bytes of it stand between the members and 64 behind the last one -- zeros, 0xff or
  seeded random bytes, which no member's outcome may depend on; the buffer is compared after the call;
* a deflate stream that does not fit touches nothing: `region(i)` is the whole region of stream i.

A member that failed may leave anything between its out_len and its region's end; outside the region
nothing may change."""
import ctypes
import random

import numpy as np

IN_LEAD = 1
IN_GAPS = (0, 1, 3, 7)  # the filler between member i and member i + 1: IN_GAPS[i % 4] bytes
OUT_FIRST = 4
OUT_GAPS = (4, 8, 12, 20)  # the canary between region i and region i + 1: OUT_GAPS[i % 4] bytes
TAIL = 64
CANARY = 0xa5
FILLERS = ("zeros", "ones", "random")

# every option the region tests set, with its default (zs_gpu.h)
DEFAULTS = {"inflate_fast": 1, "inflate_ref_wrap": 1, "inflate_split": 1, "inflate_seg": 1, "inflate_wave_min": 32768,
            "lane_large_min": 2304, "lane_block": 0, "seg_bits": 0, "seg_small_min": 4096, "seg_split": 2,
            "parse_waves": 0}


class options:
    """engine options for the length of a `with` block, the defaults (zs_gpu.h) after it"""

    def __init__(self, engine, **kw):
        self.e, self.kw = engine, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.e.set_option(k, v)

    def __exit__(self, *a):
        for k in self.kw:
            self.e.set_option(k, DEFAULTS[k])


def cap4(n):
    """n rounded up to the device entries' 4-byte granularity (0 stays 0)"""
    return (n + 3) & ~3


def filler(kind, n, seed=0x51ed):
    if kind == "zeros":
        return bytes(n)
    if kind == "ones":
        return b"\xff" * n
    assert kind == "random"
    return random.Random(seed).getrandbits(8 * n).to_bytes(n, "little") if n else b""


def follows_filler(i, n):
    """member i of n stands directly in front of filler bytes (not of the next member)"""
    return i == n - 1 or IN_GAPS[i % 4] > 0


def pack_inputs(members, kind):
    """(buffer, offsets): the members behind IN_LEAD bytes of filler, IN_GAPS between them, TAIL behind"""
    fill = filler(kind, IN_LEAD + 8 * len(members) + TAIL)
    blob, offs, at = bytearray(fill[:IN_LEAD]), [], IN_LEAD
    for i, m in enumerate(members):
        offs.append(len(blob))
        blob += m
        g = TAIL if i == len(members) - 1 else IN_GAPS[i % 4]
        blob += fill[at:at + g]
        at += g
    return bytes(blob), offs


def out_layout(caps):
    """(offsets, buffer size): the first region at OUT_FIRST, OUT_GAPS between the regions, TAIL behind"""
    offs, at = [], OUT_FIRST
    for i, c in enumerate(caps):
        assert c % 4 == 0
        offs.append(at)
        at += c + (TAIL if i == len(caps) - 1 else OUT_GAPS[i % 4])
    return offs, at


def dirty(out, offs, caps, limit=8):
    """The clean check: the offsets of the first `limit` bytes of `out` (a numpy u8 array) outside the
    regions [offs[i], offs[i] + caps[i]) that are not CANARY -- [] when no store left a region."""
    inside = np.zeros(out.shape[0], dtype=bool)
    for a, c in zip(offs, caps):
        inside[a:a + c] = True
    return np.flatnonzero((out != CANARY) & ~inside)[:limit].tolist()


class Run:
    """One call's outcome: rows (a tuple per member), the output buffer (numpy u8) and its layout, the
    bytes outside the regions that changed (`dirty`, [] expected), whether the input buffer is still
    what it was (`input_kept`), and for inflate the lane and segmented counts."""

    def region(self, i):
        return self.out[self.offs[i]:self.offs[i] + self.caps[i]].tobytes()

    def ok(self):
        return not self.dirty and self.input_kept


def _buffers(members, caps, kind):
    import torch

    blob, in_off = pack_inputs(members, kind)
    out_off, total = out_layout(caps)
    n = len(members)
    d_in = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_out = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    arrays = ((ctypes.c_uint64 * n)(*in_off), (ctypes.c_uint32 * n)(*[len(m) for m in members]),
              (ctypes.c_uint64 * n)(*out_off), (ctypes.c_uint32 * n)(*caps))
    return blob, d_in, d_out, out_off, arrays


def _finish(run, blob, d_in, d_out, out_off, caps):
    run.out = d_out.cpu().numpy()
    run.offs, run.caps = out_off, list(caps)
    run.dirty = dirty(run.out, out_off, caps)
    run.input_kept = d_in.cpu().numpy().tobytes() == blob
    return run


def inflate_run(engine, fmt, comps, caps, kind="zeros"):
    """zs_inflate_batch_device_ex: rows (status, phase, message, bytes, consumed, check)"""
    import torch
    import zsamd

    L = zsamd.lib()
    P, U64P, U32P = ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    L.zs_inflate_batch_device_ex.argtypes = [P, ctypes.c_int, ctypes.c_uint32, P, U64P, U32P, P, U64P, U32P] + [P] * 7
    n = len(comps)
    blob, d_in, d_out, out_off, (a_ioff, a_ilen, a_ooff, a_ocap) = _buffers(comps, caps, kind)
    res = [torch.full((n,), -77, dtype=torch.int32, device="cuda") for _ in range(6)]
    r = L.zs_inflate_batch_device_ex(engine.handle, zsamd.decompress_wbits(fmt), n, d_in.data_ptr(), a_ioff, a_ilen,
                                     d_out.data_ptr(), a_ooff, a_ocap, *[x.data_ptr() for x in res], None)
    assert r == 0, L.zs_last_error()
    torch.cuda.synchronize()
    run = Run()
    run.lanes, run.segs = engine.last_lane_count(), engine.last_seg_count()
    st, ph, ms, ol, co, ck = [x.tolist() for x in res]
    _finish(run, blob, d_in, d_out, out_off, caps)
    run.rows = [(st[i], ph[i], L.zs_inflate_message(ms[i]).decode(),
                 run.out[out_off[i]:out_off[i] + (ol[i] & 0xffffffff)].tobytes(), co[i] & 0xffffffff,
                 ck[i] & 0xffffffff) for i in range(n)]
    run.out_len = [x & 0xffffffff for x in ol]
    return run


def deflate_run(engine, level, fmt, datas, caps, kind="zeros"):
    """zs_deflate_batch_device_ex: rows (status, bytes, check)"""
    import torch

    n = len(datas)
    blob, d_in, d_out, out_off, (a_ioff, a_ilen, a_ooff, a_ocap) = _buffers(datas, caps, kind)
    res = [torch.full((n,), -77, dtype=torch.int32, device="cuda") for _ in range(3)]
    engine.compress_device(level, fmt, n, d_in.data_ptr(), a_ioff, a_ilen, d_out.data_ptr(), a_ooff, a_ocap,
                           res[0].data_ptr(), res[1].data_ptr(), d_check=res[2].data_ptr())
    torch.cuda.synchronize()
    run = Run()
    st, ol, ck = [x.tolist() for x in res]
    _finish(run, blob, d_in, d_out, out_off, caps)
    run.out_len = [x & 0xffffffff for x in ol]
    run.rows = [(st[i], run.out[out_off[i]:out_off[i] + run.out_len[i]].tobytes(), ck[i] & 0xffffffff)
                for i in range(n)]
    return run


def runs(seed, n):
    """Text stretches between runs of period 1 .. 7 (1 .. 3,000 bytes) and far repeats of 64 .. 258
    bytes: long copies at distance 1 .. 7 at every alignment to the decoders' 16- and 64-byte units."""
    import corpus

    rng = random.Random(seed)
    text = corpus.text(corpus.stream_seed(seed), 1 << 16)
    out = bytearray()
    while len(out) < n:
        at = rng.randrange(0, len(text) - 1200)
        out += text[at:at + rng.randrange(200, 1200)]
        p = rng.randrange(1, 8)
        pat = bytes(rng.randrange(256) for _ in range(p))
        k = rng.choice([rng.randrange(1, 64), rng.randrange(64, 400), rng.randrange(400, 3000)])
        out += (pat * (k // p + 1))[:k]
        if len(out) > 31000 and rng.random() < 0.5:
            at = len(out) - rng.randrange(300, 30000)
            out += out[at:at + rng.randrange(64, 259)]
    return bytes(out[:n])
