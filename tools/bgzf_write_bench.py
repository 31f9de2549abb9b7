#!/usr/bin/env python3
"""BGZF write workload: 64 MiB of the T corpus, compressed on the device at one level in
three ways --
  floor    the ceil(64 MiB / 65,280) = 1,029 pieces as a plain gzip batch (zs_deflate_batch_device_ex):
           the work of the blocks without the BGZF layout, which a build before the writer can also run
  flushed  the 64 MiB as ONE gzip stream with flush_every = 65,280 (zs_deflate_batch_flush_device): the
           nearest path before the writer, one member that bgzip readers cannot seek in
  bgzf     the 64 MiB as ONE stream with bgzf=True (zs_deflate_batch_bgzf_device)
Times are HIP-event times (zs_last_batch_ms) over --steps timed calls per configuration and round, taken in
--rounds rounds that alternate the configurations, after --warmup untimed calls of each: median, minimum and
maximum, the phases' medians, and the two ratios over the floor.  The BGZF output is then fed to the reader
(members="bgzf") and must give the input back.  Writes one JSON document to --out
(profiles/bgzf_write/bgzf_write_bench.json) and prints it.

    python tools/bgzf_write_bench.py [--mib 64] [--level 6]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("checksum", "bucket", "sweep", "prev", "match", "fast", "parse", "trees", "layout", "emit", "bgzf_frame",
          "stored", "finish")
B = 65280


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5, help="timed calls per configuration and round")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_write", "bgzf_write_bench.json"))
    a = ap.parse_args()

    import torch
    import zsamd

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    total = a.mib << 20
    host = zsamd.corpus("text", 0, total >> 16, 65536, threads=8)
    eng = zsamd.Engine(0)
    n = (total + B - 1) // B
    lens = [min(B, total - i * B) for i in range(n)]

    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    cap_b = zsamd.deflate_capacity(B, "gzip")
    cap_1 = (max(zsamd.deflate_bound(total, "gzip", bgzf=True), zsamd.deflate_bound(total, "gzip", n_flush=n)) + 3) & ~3
    d_out = torch.zeros(max(n * cap_b, cap_1), dtype=torch.uint8, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    b_in_off = (ctypes.c_uint64 * n)(*range(0, total, B))
    b_in_len = (ctypes.c_uint32 * n)(*lens)
    b_out_off = (ctypes.c_uint64 * n)(*range(0, n * cap_b, cap_b))
    b_cap = (ctypes.c_uint32 * n)(*[cap_b] * n)
    one = lambda ctype, v: (ctype * 1)(v)

    def run(kind):
        if kind == "floor":
            eng.compress_device(a.level, "gzip", n, d_in.data_ptr(), b_in_off, b_in_len, d_out.data_ptr(), b_out_off,
                                b_cap, d_status.data_ptr(), d_len.data_ptr())
            return n
        kw = {"flush_every": B} if kind == "flushed" else {"bgzf": True}
        eng.compress_device(a.level, "gzip", 1, d_in.data_ptr(), one(ctypes.c_uint64, 0), one(ctypes.c_uint32, total),
                            d_out.data_ptr(), one(ctypes.c_uint64, 0), one(ctypes.c_uint32, cap_1), d_status.data_ptr(),
                            d_len.data_ptr(), **kw)
        return 1

    configs = ["floor", "flushed", "bgzf"]
    times = {c: [] for c in configs}
    phases = {c: {} for c in configs}
    sizes = {}
    for c in configs:
        for _ in range(a.warmup):
            m = run(c)
        torch.cuda.synchronize()
        assert int((d_status[:m] != 1).sum()) == 0, "some streams failed (%s)" % c
        sizes[c] = int(d_len[:m].to(torch.int64).sum())
    for _ in range(a.rounds):
        for c in configs:
            for _ in range(a.steps):
                eng.set_timing(True)
                run(c)
                torch.cuda.synchronize()
                times[c].append(eng.last_ms())
                for ph in PHASES:
                    v = eng.last_ms(ph)
                    if v >= 0:
                        phases[c].setdefault(ph, []).append(v)
                eng.set_timing(False)
    res = {"in_bytes": total, "block_bytes": B, "blocks": n, "level": a.level, "build_id": zsamd.build_id(),
           "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "configs": {}}
    for c in configs:
        t = times[c]
        med = statistics.median(t)
        res["configs"][c] = {"calls": len(t), "ms_median": round(med, 4), "ms_min": round(min(t), 4),
                             "ms_max": round(max(t), 4), "gbps": round(total / med / 1e6, 2), "out_bytes": sizes[c],
                             "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[c].items()}}
    floor = res["configs"]["floor"]
    res["floor_spread_ms"] = round(floor["ms_max"] - floor["ms_min"], 4)
    for c in ("flushed", "bgzf"):
        res[c + "_over_floor"] = round(res["configs"][c]["ms_median"] / floor["ms_median"], 4)
    res["bgzf_over_flushed"] = round(res["configs"]["bgzf"]["ms_median"] / res["configs"]["flushed"]["ms_median"], 4)

    # the file, through the reader: the blocks' index against the headers, then the decode back to the input
    run("bgzf")
    torch.cuda.synchronize()
    blocks = eng.last_bgzf_blocks()[0]
    out_len = int(d_len[0])
    bgzf = bytes(d_out[:out_len].cpu().numpy())
    assert len(blocks) == n + 1 and blocks[-1] == (total, out_len - 28)
    assert zsamd.bgzf_out_len(bgzf) == total
    eng.set_timing(True)
    back = eng.decompress_batch([bgzf], "gzip", members="bgzf")
    dec_ms = eng.last_ms()
    eng.set_timing(False)
    assert back[0] == bytes(host), "the reader does not give the input back"
    res["reader"] = {"file_bytes": out_len, "blocks_trusted": eng.last_bgzf_trusted(), "round_trip": True,
                     "host_call_kernels_ms": round(dec_ms, 4)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
