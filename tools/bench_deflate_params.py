#!/usr/bin/env python3
"""windowBits / memLevel workload: N T-corpus streams of R bytes compressed on
the device, raw deflate, once per configuration -- levels 1 and 6 through the plain entry
(zs_deflate_batch_device_ex: window 15, memLevel 8, the sweep at level 6), then both levels
at (window_bits, mem_level) = (9, 8), (12, 8), (15, 1) and (15, 9) through
zs_deflate_batch_params_device (the chain-walk kernels at level 6; at level 1 the
group-speculative kernel, and the step-by-step one with head[] in global memory at (15, 9)).
Prints one JSON line: per configuration the median, minimum and maximum device time
(zs_last_batch_ms over --steps timed batches, taken in --rounds rounds that alternate the
configurations, after --warmup untimed batches of each), the phase medians and the
compressed size.

    python tools/bench_deflate_params.py [--streams 4096] [--stream-bytes 65536] [--levels 1 6]

With ZS_LIB naming a library built before the params entries, only the plain
configurations run (the comparison against an earlier build)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("checksum", "bucket", "sweep", "prev", "match", "fast", "parse", "trees", "layout", "emit", "finish")
PARAMS = ((9, 8), (12, 8), (15, 1), (15, 9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-bytes", type=int, default=65536)
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 6])
    ap.add_argument("--format", default="deflate-raw")
    ap.add_argument("--steps", type=int, default=5, help="timed batches per configuration and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import torch
    import zsamd

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    n, rb = a.streams, a.stream_bytes
    host = zsamd.corpus("text", 0, n, rb, threads=8)
    eng = zsamd.Engine(0)
    L = zsamd.lib()
    have = hasattr(L, "zs_deflate_batch_params_device")

    # name -> (level, window_bits, mem_level, capacity)
    configs = {}
    for level in a.levels:
        configs["l%d" % level] = (level, None, 8, zsamd.deflate_capacity(rb, a.format))
        for wb, ml in PARAMS if have else ():
            bound = int(L.zs_deflate_bound_params(rb, zsamd.compress_params(a.format, wb, ml), ml, level))
            configs["l%d/w%d/m%d" % (level, wb, ml)] = (level, wb, ml, (bound + 3) & ~3)
    cap = max(c[3] for c in configs.values())
    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    d_out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    in_off = (ctypes.c_uint64 * n)(*range(0, n * rb, rb))
    in_len = (ctypes.c_uint32 * n)(*[rb] * n)
    out_off = (ctypes.c_uint64 * n)(*range(0, n * cap, cap))

    def run(cfg):
        level, wb, ml, c = cfg
        kw = {"window_bits": wb, "mem_level": ml} if have else {}
        eng.compress_device(level, a.format, n, d_in.data_ptr(), in_off, in_len, d_out.data_ptr(), out_off,
                            (ctypes.c_uint32 * n)(*[c] * n), d_status.data_ptr(), d_len.data_ptr(), **kw)

    times = {k: [] for k in configs}
    phases = {k: {} for k in configs}
    sizes = {}
    for name, cfg in configs.items():
        for _ in range(a.warmup):
            run(cfg)
        torch.cuda.synchronize()
        assert int((d_status != 1).sum()) == 0, "some streams failed (%s)" % name
        sizes[name] = int(d_len.sum())
    for _ in range(a.rounds):
        for name, cfg in configs.items():
            for _ in range(a.steps):
                eng.set_timing(True)
                run(cfg)
                torch.cuda.synchronize()
                times[name].append(eng.last_ms())
                for ph in PHASES:
                    v = eng.last_ms(ph)
                    if v >= 0:
                        phases[name].setdefault(ph, []).append(v)
                eng.set_timing(False)
    res = {"streams": n, "stream_bytes": rb, "format": a.format, "in_bytes": n * rb, "build_id": zsamd.build_id(),
           "lib": os.path.basename(os.path.dirname(zsamd.LIB_PATH)), "batches_per_config": a.rounds * a.steps, "configs": {}}
    for name in configs:
        t = times[name]
        med = statistics.median(t)
        res["configs"][name] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                                "gbps": round(n * rb / med / 1e6, 2), "out_bytes": sizes[name],
                                "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[name].items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
