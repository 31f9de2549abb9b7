#!/usr/bin/env python3
"""Restart points without an index: N R bytes of the T corpus (1,024 x 64 KiB) as ONE
gzip stream flushed every R bytes (the engine's own zs_deflate_batch_flush_device), decoded on the
device in three ways --
  plain    the plain entry with inflate_ref_wrap = 0 (one stream, one decoder)
  restart  the restart entry with the given points (zs_last_flush_index)
  sync     the entry that finds the points itself (zs_inflate_batch_sync_device)
-- and, for `sync` and `plain`, a batch of B unflushed members of R bytes (4,096 x 64 KiB), which gains
nothing from the search.  Prints one JSON line: per configuration the median, minimum and maximum of
the call's device time (zs_last_batch_ms: first to last mark on the stream, so the sync entry's host
planning in the middle counts) and of its wall time (the call and the wait for the stream) over
--steps timed calls, taken in --rounds rounds that alternate the configurations, after --warmup untimed
calls of each; the phases' medians, minima and maxima ("sync_scan", "sync_size" and the restart phases).

    python tools/bench_sync.py [--segments 1024] [--members 4096] [--stream-bytes 65536]

With ZS_LIB naming a library built before the sync entries, `plain` and `restart` alone run (the
comparison against an earlier build)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("sync_scan", "sync_size", "restart_gather", "inflate", "restart_place", "restart_stitch", "finish")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=1024)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--stream-bytes", type=int, default=65536)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5, help="timed calls per configuration and round")
    ap.add_argument("--plain-steps", type=int, default=1, help="... of the one stream's plain decode (one decoder)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import torch
    import zsamd

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    fmt, rb = "gzip", a.stream_bytes
    n_seg, n_mem = a.segments, a.members
    total1, totalb = n_seg * rb, n_mem * rb
    assert max(total1, totalb) < 1 << 32, "one stream's length is a u32"
    host = zsamd.corpus("text", 0, max(n_seg, n_mem), rb, threads=8)
    eng = zsamd.Engine(0)
    have = hasattr(zsamd.lib(), "zs_inflate_batch_sync_device")
    arr = lambda ctype, v: (ctype * len(v))(*v)

    d_src = torch.frombuffer(host, dtype=torch.uint8).cuda()
    # the inputs: the one flushed stream and its index; the batch of members
    cap_1 = (zsamd.deflate_bound(total1, fmt) + 12 * n_seg + 3) & ~3
    cap_b = zsamd.deflate_capacity(rb, fmt)
    d_comp1 = torch.zeros(cap_1, dtype=torch.uint8, device="cuda")
    d_compb = torch.zeros(n_mem * cap_b, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(max(n_mem, 1), dtype=torch.int32, device="cuda")
    d_len = torch.zeros(max(n_mem, 1), dtype=torch.int32, device="cuda")
    eng.compress_device(a.level, fmt, 1, d_src.data_ptr(), arr(ctypes.c_uint64, [0]), arr(ctypes.c_uint32, [total1]),
                        d_comp1.data_ptr(), arr(ctypes.c_uint64, [0]), arr(ctypes.c_uint32, [cap_1]), d_st.data_ptr(),
                        d_len.data_ptr(), flush_every=rb)
    torch.cuda.synchronize()
    assert int(d_st[0]) == 1
    len1 = int(d_len[0])
    index = eng.last_flush_index()[0]
    points = [list(zip(index, range(rb, total1 + 1, rb)))]
    header = bytes(d_comp1[:64].cpu().numpy())
    eng.compress_device(a.level, fmt, n_mem, d_src.data_ptr(), arr(ctypes.c_uint64, list(range(0, totalb, rb))),
                        arr(ctypes.c_uint32, [rb] * n_mem), d_compb.data_ptr(),
                        arr(ctypes.c_uint64, list(range(0, n_mem * cap_b, cap_b))), arr(ctypes.c_uint32, [cap_b] * n_mem),
                        d_st.data_ptr(), d_len.data_ptr())
    torch.cuda.synchronize()
    assert int((d_st[:n_mem] != 1).sum()) == 0
    lenb = [int(x) for x in d_len[:n_mem].tolist()]

    d_out = torch.zeros(max(total1, totalb), dtype=torch.uint8, device="cuda")
    res = [torch.zeros(max(n_mem, 1), dtype=torch.int32, device="cuda") for _ in range(5)]
    ptrs = [t.data_ptr() for t in res]
    one = (1, d_comp1.data_ptr(), arr(ctypes.c_uint64, [0]), arr(ctypes.c_uint32, [len1]), d_out.data_ptr(),
           arr(ctypes.c_uint64, [0]), arr(ctypes.c_uint32, [total1]))
    batch = (n_mem, d_compb.data_ptr(), arr(ctypes.c_uint64, list(range(0, n_mem * cap_b, cap_b))), arr(ctypes.c_uint32, lenb),
             d_out.data_ptr(), arr(ctypes.c_uint64, list(range(0, totalb, rb))), arr(ctypes.c_uint32, [rb] * n_mem))

    def run(kind, what):
        args = one if what == "one" else batch
        kw = {"restart": "scan"} if kind == "sync" else {"restart": points, "headers": [header]} if kind == "restart" else {}
        eng.set_option("inflate_ref_wrap", 0)
        try:
            eng.decompress_device(fmt, *args, *ptrs, **kw)
        finally:
            eng.set_option("inflate_ref_wrap", 1)
        return args[0]

    configs = [("plain", "one"), ("restart", "one")] + ([("sync", "one"), ("sync", "batch")] if have else []) + [("plain", "batch")]
    name = lambda c: "%s/%s" % c
    steps = lambda c: a.plain_steps if c == ("plain", "one") else a.steps
    dev = {name(c): [] for c in configs}
    wall = {name(c): [] for c in configs}
    phases = {name(c): {} for c in configs}
    want = bytes(host[:4096]), bytes(host[total1 - 4096:total1])
    for c in configs:
        for _ in range(1 if c == ("plain", "one") else a.warmup):
            m = run(*c)
        torch.cuda.synchronize()
        assert int((res[0][:m] != 1).sum()) == 0, "some streams failed (%s)" % name(c)
        if c[1] == "one":
            assert int(res[3][0]) == total1 and bytes(d_out[:4096].cpu().numpy()) == want[0]
            assert bytes(d_out[total1 - 4096:total1].cpu().numpy()) == want[1]
    for _ in range(a.rounds):
        for c in configs:
            for _ in range(steps(c)):
                eng.set_timing(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(*c)
                torch.cuda.synchronize()
                wall[name(c)].append((time.perf_counter() - t0) * 1e3)
                dev[name(c)].append(eng.last_ms())
                for ph in PHASES:
                    v = eng.last_ms(ph)
                    if v >= 0:
                        phases[name(c)].setdefault(ph, []).append(v)
                eng.set_timing(False)
    out = {"segments": n_seg, "members": n_mem, "stream_bytes": rb, "level": a.level, "format": fmt, "one_bytes": len1,
           "batch_bytes": sum(lenb), "build_id": zsamd.build_id(), "lib": os.path.basename(os.path.dirname(zsamd.LIB_PATH)),
           "rounds": a.rounds, "steps": a.steps, "plain_steps": a.plain_steps, "configs": {}}
    if have:
        eng.decompress_device(fmt, *one, *ptrs, restart="scan")
        torch.cuda.synchronize()
        out["points_found_equal_the_index"] = eng.last_restart_points() == points
    q = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for c in configs:
        out["configs"][name(c)] = {"calls": len(dev[name(c)]), "device_ms": q(dev[name(c)]), "wall_ms": q(wall[name(c)]),
                                   "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[name(c)].items()},
                                   "phase_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)]
                                                        for k, v in phases[name(c)].items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
