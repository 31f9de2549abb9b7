#!/usr/bin/env python3
"""Primed-pieces workload: the headline's T-corpus bytes (4,096 x 64 KiB = 256 MiB) as
ONE stream, compressed on the device with a point every --every bytes in two ways --
  flushed  Z_FULL_FLUSH at every point (zs_deflate_batch_flush_device): the yardstick
  primed   primed pieces between the points (zs_deflate_batch_primed_device)
-- for deflate-raw and for gzip (where the stream's one crc32 is over all the bytes), at every --levels
level.  Prints one JSON line: per configuration the median, minimum and maximum device time
(zs_last_batch_ms over --steps timed batches, taken in --rounds rounds that alternate primed and
flushed, after --warmup untimed batches of each), the phase medians and the compressed size.

Outside the timed region every primed output is compared with what C zlib builds for the same
construction (a raw stream per piece, zdict = the 32 KiB in front of it, Z_SYNC_FLUSH / Z_FINISH; the
wrapper around all of them): "verified" is true when the bytes are equal, and null when the zlib that
is running is not 1.2.11 or --no-verify is given.

    python tools/bench_primed.py [--streams 4096] [--stream-bytes 65536] [--levels 1 6 9] [--every 65536 131072]

With ZS_LIB naming a library built before the primed entries, `flushed` alone runs (the comparison
against an earlier build)."""
import argparse
import concurrent.futures
import ctypes
import hashlib
import json
import os
import statistics
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("checksum", "bucket", "sweep", "prev", "match", "fast", "parse", "trees", "layout", "emit", "finish")
W = 32768


def zlib_primed_body(data, level, every, threads=16):
    """the pieces' bytes as zlib writes them, each compressed on its own (zlib releases the GIL)"""
    edges = list(range(0, len(data), every)) + [len(data)]
    view = memoryview(data)

    def piece(j):
        a, b = edges[j], edges[j + 1]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0, bytes(view[max(0, a - W):a])) if a else \
            zlib.compressobj(level, zlib.DEFLATED, -15, 8, 0)
        out = [c.compress(view[i:min(i + W, b)]) for i in range(a, b, W)]
        out.append(c.flush() if j + 2 == len(edges) else c.flush(zlib.Z_SYNC_FLUSH))
        return b"".join(out)

    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        return b"".join(ex.map(piece, range(len(edges) - 1)))


def wrapped(body, data, level, fmt):
    if fmt == "deflate-raw":
        return body
    wb = 15 if fmt == "deflate" else 31
    c = zlib.compressobj(level, zlib.DEFLATED, wb, 8, 0)
    head = (c.compress(b"") + c.flush())[:2 if fmt == "deflate" else 10]
    if fmt == "deflate":
        return head + body + struct.pack(">I", zlib.adler32(data))
    return head[:9] + b"\xff" + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-bytes", type=int, default=65536)
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 6, 9])
    ap.add_argument("--every", type=int, nargs="+", default=[65536, 131072])
    ap.add_argument("--formats", nargs="+", default=["deflate-raw", "gzip"])
    ap.add_argument("--steps", type=int, default=5, help="timed batches per configuration and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-verify", action="store_true")
    a = ap.parse_args()

    import torch
    import zsamd

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    total = a.streams * a.stream_bytes
    assert total < 1 << 32, "one stream's length is a u32"
    host = zsamd.corpus("text", 0, a.streams, a.stream_bytes, threads=8)
    eng = zsamd.Engine(0)
    have = hasattr(zsamd.lib(), "zs_deflate_batch_primed_device")
    verify = have and not a.no_verify and zlib.ZLIB_RUNTIME_VERSION == "1.2.11"

    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    points = max(total // e for e in a.every)
    cap = max((zsamd.deflate_bound(total, f) + 12 * points + 3) & ~3 for f in a.formats)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = lambda ctype, v: (ctype * 1)(v)

    def run(kind, fmt, level, every):
        kw = {"primed": True} if kind == "primed" else {}
        eng.compress_device(level, fmt, 1, d_in.data_ptr(), one(ctypes.c_uint64, 0), one(ctypes.c_uint32, total),
                            d_out.data_ptr(), one(ctypes.c_uint64, 0), one(ctypes.c_uint32, cap), d_status.data_ptr(),
                            d_len.data_ptr(), flush_every=every, **kw)

    kinds = (["primed"] if have else []) + ["flushed"]
    configs = [(k, f, lv, e) for lv in a.levels for e in a.every for f in a.formats for k in kinds]
    name = lambda c: "%s/%s/l%d/every%d" % c
    times = {name(c): [] for c in configs}
    phases = {name(c): {} for c in configs}
    sizes, verified, bodies = {}, {}, {}
    for c in configs:
        for _ in range(a.warmup):
            run(*c)
        torch.cuda.synchronize()
        assert int(d_status[0]) == 1, "the stream failed (%s)" % name(c)
        sizes[name(c)] = int(d_len[0]) & 0xffffffff
        if c[0] == "primed":  # outside the timed region: the bytes are zlib's for the same construction
            verified[name(c)] = None
            if verify:
                key = (c[2], c[3])
                if key not in bodies:
                    bodies = {key: zlib_primed_body(host, c[2], c[3])}  # (one at a time: 100 MB each)
                want = wrapped(bodies[key], host, c[2], c[1])
                got = bytes(d_out[:sizes[name(c)]].cpu().numpy())
                verified[name(c)] = hashlib.sha256(got).digest() == hashlib.sha256(want).digest()
                assert verified[name(c)], "the primed output differs from zlib's (%s)" % name(c)
    bodies = {}
    for _ in range(a.rounds):
        for c in configs:
            for _ in range(a.steps):
                eng.set_timing(True)
                run(*c)
                torch.cuda.synchronize()
                times[name(c)].append(eng.last_ms())
                for ph in PHASES:
                    v = eng.last_ms(ph)
                    if v >= 0:
                        phases[name(c)].setdefault(ph, []).append(v)
                eng.set_timing(False)
    res = {"in_bytes": total, "levels": a.levels, "every": a.every, "build_id": zsamd.build_id(),
           "lib": os.path.basename(os.path.dirname(zsamd.LIB_PATH)), "rounds": a.rounds, "steps": a.steps,
           "zlib": zlib.ZLIB_RUNTIME_VERSION, "configs": {}}
    for c in configs:
        t = times[name(c)]
        med = statistics.median(t)
        res["configs"][name(c)] = {"batches": len(t), "ms_median": round(med, 4), "ms_min": round(min(t), 4),
                                   "ms_max": round(max(t), 4), "gbps": round(total / med / 1e6, 2),
                                   "out_bytes": sizes[name(c)],
                                   "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[name(c)].items()}}
        if c[0] == "primed":
            res["configs"][name(c)]["verified"] = verified[name(c)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
