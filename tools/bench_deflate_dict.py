#!/usr/bin/env python3
"""Dictionary-compression workload: N T-corpus records of R bytes
compressed on the device, level 6 by default, raw deflate -- each against one shared
32 KiB T-corpus dictionary (zs_deflate_batch_dict_device), and the same records
without one (zs_deflate_batch_device_ex).  Prints one JSON line: the median device
time of each (zs_last_batch_ms over --steps timed batches, phases included), the
compressed sizes, and the share of the sweep's 64-member chunks whose members are
all dictionary positions (look-back only: built, hashed and sorted, never swept),
counted on the host over --sample streams with the sweep's order (hash, then
position).

    python tools/bench_deflate_dict.py [--records 65536] [--record-bytes 4096] [--level 6]

With ZS_LIB naming a library built before the dictionary entries, only the
no-dictionary half runs (the comparison against an earlier build)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("dict_join", "checksum", "bucket", "sweep", "fast", "parse", "trees", "layout", "emit", "finish")


def lookback_share(dictionary, records, rec_bytes, sample):
    """share of the 64-member chunks of a stream's window without an own position"""
    import numpy as np

    lp = len(dictionary)
    d = np.frombuffer(dictionary, dtype=np.uint8)
    chunks = lookback = 0
    for i in range(sample):
        j = np.concatenate([d, np.frombuffer(records, dtype=np.uint8, count=rec_bytes, offset=i * rec_bytes)]).astype(np.uint32)
        m = len(j) - 2  # inserted positions (p <= nv - 3)
        h = ((j[:m] << 10) ^ (j[1:m + 1] << 5) ^ j[2:m + 2]) & 0x7fff
        order = np.argsort(h, kind="stable")  # the sweep's members: by hash, stable in position
        pad = (-m) % 64
        own = np.concatenate([order >= lp, np.zeros(pad, dtype=bool)]).reshape(-1, 64)
        chunks += own.shape[0]
        lookback += int((~own.any(axis=1)).sum())
    return lookback / chunks, chunks // sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--record-bytes", type=int, default=4096)
    ap.add_argument("--dict-bytes", type=int, default=32768)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--format", default="deflate-raw")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=16, help="streams of the host-side chunk count")
    a = ap.parse_args()

    import torch
    import zsamd

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    n, rb = a.records, a.record_bytes
    host = zsamd.corpus("text", 0, n, rb, threads=8)
    dictionary = bytes(zsamd.corpus("text", 1 << 20, 1, a.dict_bytes, threads=1))  # (a stream index outside the records')
    eng = zsamd.Engine(0)
    have_dict = hasattr(zsamd.lib(), "zs_deflate_batch_dict_device")
    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    d_dict = torch.frombuffer(bytearray(dictionary), dtype=torch.uint8).cuda()
    cap = zsamd.deflate_capacity(rb, a.format, a.dict_bytes) if have_dict else zsamd.deflate_capacity(rb, a.format)
    d_out = torch.zeros(n * cap, dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    in_off = (ctypes.c_uint64 * n)(*range(0, n * rb, rb))
    in_len = (ctypes.c_uint32 * n)(*[rb] * n)
    out_off = (ctypes.c_uint64 * n)(*range(0, n * cap, cap))
    out_cap = (ctypes.c_uint32 * n)(*[cap] * n)
    dict_off = (ctypes.c_uint64 * n)()
    dict_len = (ctypes.c_uint32 * n)(*[a.dict_bytes] * n)

    def run(with_dict):
        kw = dict(d_dict=d_dict.data_ptr(), dict_off=dict_off, dict_len=dict_len) if with_dict else {}
        eng.compress_device(a.level, a.format, n, d_in.data_ptr(), in_off, in_len, d_out.data_ptr(), out_off, out_cap,
                            d_status.data_ptr(), d_len.data_ptr(), **kw)

    def measure(with_dict):
        for _ in range(a.warmup):
            run(with_dict)
        torch.cuda.synchronize()
        times, phases = [], {}
        for _ in range(a.steps):
            eng.set_timing(True)
            run(with_dict)
            torch.cuda.synchronize()
            times.append(eng.last_ms())
            for ph in PHASES:
                v = eng.last_ms(ph)
                if v >= 0:
                    phases.setdefault(ph, []).append(v)
            eng.set_timing(False)
        assert int((d_status != 1).sum()) == 0, "some streams failed"
        return {"ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4),
                "ms_max": round(max(times), 4), "out_bytes": int(d_len.sum()),
                "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases.items()}}

    res = {"records": n, "record_bytes": rb, "dict_bytes": a.dict_bytes, "level": a.level, "format": a.format,
           "in_bytes": n * rb, "build_id": zsamd.build_id(), "lib": os.path.basename(os.path.dirname(zsamd.LIB_PATH)),
           "no_dict": measure(False)}
    if have_dict:
        res["dict"] = measure(True)
        share, chunks = lookback_share(dictionary, host, rb, min(a.sample, n))
        res["lookback_only_chunk_share"] = round(share, 4)
        res["chunks_per_stream"] = chunks
    print(json.dumps(res))


if __name__ == "__main__":
    main()
