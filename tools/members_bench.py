#!/usr/bin/env python3
"""Multi-member gzip files: 64 MiB of the T corpus as ONE gzip file of 65,280-byte members
at level 6 plus the BGZF end-of-file block, made by zlib on the host, decoded on the device --
  plain/members    (a) the plain gzip batch over the same members with their boundaries given: the decode
                   alone, the floor
  restart/flushed  the restart entry with the given points over the same bytes as one stream flushed
                   every 65,280 bytes: the sibling's floor
  sync/flushed     (b) restart="scan" over that stream: the sibling
  members/one      (c) the members call over the one file
  members/eight    ... and over the same members as 8 files of 8 MiB
Prints one JSON line: per configuration the median, minimum and maximum of the call's device time
(zs_last_batch_ms: first to last mark on the stream, so the host planning in the middle counts) and of its
wall time over --steps timed calls, taken in --rounds rounds that alternate the configurations, after
--warmup untimed calls of each; the phases' medians; the ratios c/a, c/b and b to its own floor.

    python tools/members_bench.py [--mib 64] [--member-bytes 65280] [--steps 7] [--rounds 3]"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("members_scan", "members_size", "members_stitch", "sync_scan", "sync_size", "restart_gather", "inflate_lane",
          "inflate", "inflate_check", "restart_place", "restart_stitch", "finish")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--member-bytes", type=int, default=65280)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--steps", type=int, default=7, help="timed calls per configuration and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch
    import zsamd

    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.init()
    fmt, mb = "gzip", a.member_bytes
    total = a.mib << 20
    host = bytes(zsamd.corpus("text", 0, total // 65536, 65536, threads=8))
    assert len(host) == total
    cuts = list(range(0, total, mb)) + [total]
    M = len(cuts) - 1

    def gz(k):
        co = zlib.compressobj(a.level, zlib.DEFLATED, 31)
        return co.compress(host[cuts[k]:cuts[k + 1]]) + co.flush()

    with ThreadPoolExecutor(8) as ex:
        mem = list(ex.map(gz, range(M)))
    one_file = b"".join(mem) + BGZF_EOF
    starts, at = [], 0
    for m in mem:
        starts.append(at)
        at += len(m)
    # the same bytes as one stream flushed at every member boundary, and its index
    co = zlib.compressobj(a.level, zlib.DEFLATED, 31)
    flushed, points = b"", []
    for k in range(M):
        flushed += co.compress(host[cuts[k]:cuts[k + 1]]) + (co.flush(zlib.Z_FULL_FLUSH) if k + 1 < M else co.flush())
        if k + 1 < M:
            points.append((len(flushed), cuts[k + 1]))
    # ... and as 8 files
    per = (M + 7) // 8
    groups = [list(range(g, min(g + per, M))) for g in range(0, M, per)]
    files = [b"".join(mem[k] for k in g) + BGZF_EOF for g in groups]

    eng = zsamd.Engine(0)
    arr = lambda ctype, v: (ctype * len(v))(*v)
    up = lambda b: torch.frombuffer(bytearray(b + b"\0" * 16), dtype=torch.uint8).cuda()
    d_one, d_flushed, d_files = up(one_file), up(flushed), up(b"".join(files))
    cap = (total + 3) & ~3
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    res = [torch.zeros(max(M, 8), dtype=torch.int32, device="cuda") for _ in range(5)]
    d_chk = torch.zeros(max(M, 8), dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in res]
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    f_in, f_out, o = [], [], 0
    for f in files:
        f_in.append(o)
        o += len(f)
    f_lens = [cuts[g[-1] + 1] - cuts[g[0]] for g in groups]
    f_out = [cuts[g[0]] for g in groups]
    assert mb % 4 == 0 and all(x % 4 == 0 for x in f_out)
    f_caps = [(x + 3) & ~3 for x in f_lens]
    configs = {
        "plain/members": (dict(), (M, d_one.data_ptr(), arr(u64, starts), arr(u32, [len(m) for m in mem]), d_out.data_ptr(),
                                   arr(u64, cuts[:-1]), arr(u32, [(cuts[k + 1] - cuts[k] + 3) & ~3 for k in range(M)]))),
        "restart/flushed": (dict(restart=[points], headers=[flushed[:64]]),
                            (1, d_flushed.data_ptr(), arr(u64, [0]), arr(u32, [len(flushed)]), d_out.data_ptr(), arr(u64, [0]),
                             arr(u32, [cap]))),
        "sync/flushed": (dict(restart="scan"), (1, d_flushed.data_ptr(), arr(u64, [0]), arr(u32, [len(flushed)]),
                                                d_out.data_ptr(), arr(u64, [0]), arr(u32, [cap]))),
        "members/one": (dict(members=True), (1, d_one.data_ptr(), arr(u64, [0]), arr(u32, [len(one_file)]), d_out.data_ptr(),
                                             arr(u64, [0]), arr(u32, [cap]))),
        "members/eight": (dict(members=True), (len(files), d_files.data_ptr(), arr(u64, f_in), arr(u32, [len(f) for f in files]),
                                               d_out.data_ptr(), arr(u64, f_out), arr(u32, f_caps))),
    }

    def run(name):
        kw, args = configs[name]
        eng.set_option("inflate_ref_wrap", 0)
        try:
            eng.decompress_device(fmt, *args, *ptrs, d_check=d_chk.data_ptr(), **kw)
        finally:
            eng.set_option("inflate_ref_wrap", 1)
        return args[0]

    want = zlib.crc32(host)
    for name in configs:
        d_out.zero_()
        for _ in range(a.warmup):
            n = run(name)
        torch.cuda.synchronize()
        assert int((res[0][:n] != 1).sum()) == 0, "some streams failed (%s)" % name
        assert zlib.crc32(bytes(d_out[:total].cpu().numpy())) == want, "wrong output (%s)" % name
        if n == 1:
            assert int(res[3][0]) & 0xffffffff == total and int(d_chk[0]) & 0xffffffff == want, name
    dev = {c: [] for c in configs}
    wall = {c: [] for c in configs}
    phases = {c: {} for c in configs}
    for _ in range(a.rounds):
        for c in configs:
            for _ in range(a.steps):
                eng.set_timing(True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(c)
                torch.cuda.synchronize()
                wall[c].append((time.perf_counter() - t0) * 1e3)
                dev[c].append(eng.last_ms())
                for ph in PHASES:
                    v = eng.last_ms(ph)
                    if v >= 0:
                        phases[c].setdefault(ph, []).append(v)
                eng.set_timing(False)
    run("members/one")
    torch.cuda.synchronize()
    idx = eng.last_members()[0]
    q = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    med = lambda c: statistics.median(dev[c])
    out = {"mib": a.mib, "member_bytes": mb, "members": M, "level": a.level, "file_bytes": len(one_file), "flushed_bytes": len(flushed),
           "build_id": zsamd.build_id(), "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup,
           "index_equals_the_boundaries": idx == list(zip(starts, cuts[:-1])) + [(len(one_file) - 28, total)],
           "c_over_a": round(med("members/one") / med("plain/members"), 3),
           "c_over_b": round(med("members/one") / med("sync/flushed"), 3),
           "b_over_its_floor": round(med("sync/flushed") / med("restart/flushed"), 3), "configs": {}}
    for c in configs:
        out["configs"][c] = {"calls": len(dev[c]), "device_ms": q(dev[c]), "wall_ms": q(wall[c]),
                             "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[c].items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
