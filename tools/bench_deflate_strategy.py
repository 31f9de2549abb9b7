#!/usr/bin/env python3
"""Compression-strategy workload: N T-corpus streams of R bytes
compressed on the device, raw deflate, once per configuration -- level 1 and level 6
through the plain entry (zs_deflate_batch_device_ex), then level 6 with Z_FILTERED,
Z_HUFFMAN_ONLY, Z_RLE (rle_ref 1 and 0) and Z_FIXED through
zs_deflate_batch_strategy_device.  Prints one JSON line: per configuration the median,
minimum and maximum device time (zs_last_batch_ms over --steps timed batches, taken in
--rounds rounds that alternate the configurations, after --warmup untimed batches of
each), the phase medians and the compressed size.

    python tools/bench_deflate_strategy.py [--streams 4096] [--stream-bytes 65536] [--level 6]

With ZS_LIB naming a library built before the strategy entries, only the two plain
configurations run (the comparison against an earlier build: Z_HUFFMAN_ONLY and Z_RLE
search no matches and are to be compared with its level 1, Z_FILTERED and Z_FIXED with
its level 6)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("checksum", "bucket", "sweep", "fast", "parse", "huff_tally", "rle_tally", "trees", "layout", "emit", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--stream-bytes", type=int, default=65536)
    ap.add_argument("--level", type=int, default=6)
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
    have = hasattr(zsamd.lib(), "zs_deflate_batch_strategy_device")
    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    cap = zsamd.deflate_capacity(rb, a.format)
    d_out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    in_off = (ctypes.c_uint64 * n)(*range(0, n * rb, rb))
    in_len = (ctypes.c_uint32 * n)(*[rb] * n)
    out_off = (ctypes.c_uint64 * n)(*range(0, n * cap, cap))
    out_cap = (ctypes.c_uint32 * n)(*[cap] * n)

    # name -> (level, strategy, rle_ref)
    configs = {"l1": (1, 0, 1), "l%d" % a.level: (a.level, 0, 1)}
    if have:
        configs.update({"filtered": (a.level, 1, 1), "huffman_only": (a.level, 2, 1), "rle_ref1": (a.level, 3, 1),
                        "rle_ref0": (a.level, 3, 0), "fixed": (a.level, 4, 1)})

    def run(cfg):
        level, strategy, rle_ref = cfg
        kw = {}
        if have:
            eng.set_option("rle_ref", rle_ref)
            kw["strategy"] = strategy
        eng.compress_device(level, a.format, n, d_in.data_ptr(), in_off, in_len, d_out.data_ptr(), out_off, out_cap,
                            d_status.data_ptr(), d_len.data_ptr(), **kw)

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
    res = {"streams": n, "stream_bytes": rb, "level": a.level, "format": a.format, "in_bytes": n * rb,
           "build_id": zsamd.build_id(), "lib": os.path.basename(os.path.dirname(zsamd.LIB_PATH)),
           "batches_per_config": a.rounds * a.steps, "configs": {}}
    for name in configs:
        t = times[name]
        res["configs"][name] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
                                "ms_max": round(max(t), 4), "out_bytes": sizes[name],
                                "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[name].items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
