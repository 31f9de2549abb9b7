#!/usr/bin/env python3
"""Z_FULL_FLUSH workload: the headline's N T-corpus streams of R bytes (4,096 x
64 KiB), compressed on the device at one level in three ways --
  batch    the N streams as a plain batch (zs_deflate_batch_device_ex: bench.py's headline config)
  one      the same N R bytes as ONE stream without flush points: what a user with one long file
           had before flush points existed
  flushed  that one stream with flush_every = R (zs_deflate_batch_flush_device): N segments
-- for deflate-raw and for gzip (where the stream's one crc32 is over all N R bytes).  Prints one
JSON line: per configuration the median, minimum and maximum device time (zs_last_batch_ms over
--steps timed batches, taken in --rounds rounds that alternate the configurations, after --warmup
untimed batches of each; `one` is timed --one-steps times per round), the phase medians and the
compressed size.

    python tools/bench_flush.py [--streams 4096] [--stream-bytes 65536] [--level 6]

With ZS_LIB naming a library built before the flush entries, `batch` and `one` alone run (the
comparison against an earlier build)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("checksum", "bucket", "sweep", "prev", "match", "fast", "parse", "trees", "layout", "emit", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-bytes", type=int, default=65536)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--formats", nargs="+", default=["deflate-raw", "gzip"])
    ap.add_argument("--steps", type=int, default=5, help="timed batches per configuration and round")
    ap.add_argument("--one-steps", type=int, default=1, help="... of the one unflushed stream (one workgroup parses it)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-one", action="store_true")
    a = ap.parse_args()

    import torch
    import zsamd

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    n, rb = a.streams, a.stream_bytes
    total = n * rb
    assert total < 1 << 32, "one stream's length is a u32"
    host = zsamd.corpus("text", 0, n, rb, threads=8)
    eng = zsamd.Engine(0)
    have = hasattr(zsamd.lib(), "zs_deflate_batch_flush_device")

    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    cap_b = max(zsamd.deflate_capacity(rb, f) for f in a.formats)
    cap_1 = max((zsamd.deflate_bound(total, f) + 12 * n + 3) & ~3 for f in a.formats)
    d_out = torch.zeros(max(n * cap_b, cap_1), dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    b_in_off = (ctypes.c_uint64 * n)(*range(0, total, rb))
    b_in_len = (ctypes.c_uint32 * n)(*[rb] * n)
    b_out_off = (ctypes.c_uint64 * n)(*range(0, n * cap_b, cap_b))
    b_cap = (ctypes.c_uint32 * n)(*[cap_b] * n)
    one = lambda ctype, v: (ctype * 1)(v)

    def run(kind, fmt):
        if kind == "batch":
            eng.compress_device(a.level, fmt, n, d_in.data_ptr(), b_in_off, b_in_len, d_out.data_ptr(), b_out_off, b_cap,
                                d_status.data_ptr(), d_len.data_ptr())
            return n
        kw = {"flush_every": rb} if kind == "flushed" else {}
        eng.compress_device(a.level, fmt, 1, d_in.data_ptr(), one(ctypes.c_uint64, 0), one(ctypes.c_uint32, total),
                            d_out.data_ptr(), one(ctypes.c_uint64, 0), one(ctypes.c_uint32, cap_1), d_status.data_ptr(),
                            d_len.data_ptr(), **kw)
        return 1

    kinds = ["batch"] + ([] if a.skip_one else ["one"]) + (["flushed"] if have else [])
    configs = [(k, f) for f in a.formats for k in kinds]
    name = lambda c: "%s/%s" % c
    times = {name(c): [] for c in configs}
    phases = {name(c): {} for c in configs}
    sizes = {}
    for c in configs:
        for _ in range(1 if c[0] == "one" else a.warmup):
            m = run(*c)
        torch.cuda.synchronize()
        assert int((d_status[:m] != 1).sum()) == 0, "some streams failed (%s)" % name(c)
        sizes[name(c)] = int(d_len[:m].to(torch.int64).sum())
    for _ in range(a.rounds):
        for c in configs:
            for _ in range(a.one_steps if c[0] == "one" else a.steps):
                eng.set_timing(True)
                run(*c)
                torch.cuda.synchronize()
                times[name(c)].append(eng.last_ms())
                for ph in PHASES:
                    v = eng.last_ms(ph)
                    if v >= 0:
                        phases[name(c)].setdefault(ph, []).append(v)
                eng.set_timing(False)
    res = {"streams": n, "stream_bytes": rb, "level": a.level, "in_bytes": total, "build_id": zsamd.build_id(),
           "lib": os.path.basename(os.path.dirname(zsamd.LIB_PATH)), "rounds": a.rounds, "steps": a.steps,
           "one_steps": a.one_steps, "configs": {}}
    for c in configs:
        t = times[name(c)]
        med = statistics.median(t)
        res["configs"][name(c)] = {"batches": len(t), "ms_median": round(med, 4), "ms_min": round(min(t), 4),
                                   "ms_max": round(max(t), 4), "gbps": round(total / med / 1e6, 2),
                                   "out_bytes": sizes[name(c)],
                                   "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[name(c)].items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
