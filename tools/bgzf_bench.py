#!/usr/bin/env python3
"""BGZF files: tools/members_bench.py's file -- 64 MiB of the T corpus as ONE file of 65,280-byte
members at level 6 plus the BGZF end-of-file block -- written as bgzip writes it, every member with the BC subfield
and its BSIZE, made by zlib on the host, decoded on the device in one process and in alternating rounds --
  plain/members    the plain gzip batch over the same members with their boundaries given: the decode alone, the floor
  members/one      the members call over the one file (the _members code, which sizes every member by decoding it)
  bgzf/one         the _bgzf call over the one file (every member sized from its header)
Prints one JSON line: per configuration the median, minimum and maximum of the call's device time (zs_last_batch_ms:
first to last mark on the stream, so the host planning in the middle counts) and of its wall time over --steps timed
calls, taken in --rounds rounds that alternate the configurations, after --warmup untimed calls of each; the phases'
medians; bgzf/one over its floor and over members/one; its "bgzf_size" phase next to its "members_scan" phase.

    python tools/bgzf_bench.py [--mib 64] [--member-bytes 65280] [--steps 7] [--rounds 3]"""
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

PHASES = ("members_scan", "members_size", "bgzf_size", "members_stitch", "inflate_lane", "inflate", "inflate_check",
          "restart_place", "finish")
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

    def block(k):
        d = host[cuts[k]:cuts[k + 1]]
        co = zlib.compressobj(a.level, zlib.DEFLATED, -15)
        raw = co.compress(d) + co.flush()
        size = 18 + len(raw) + 8
        assert size <= 65536
        return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + raw
                + struct.pack("<II", zlib.crc32(d), len(d)))

    with ThreadPoolExecutor(8) as ex:
        mem = list(ex.map(block, range(M)))
    one_file = b"".join(mem) + BGZF_EOF
    assert zsamd.bgzf_out_len(one_file) == total
    starts, at = [], 0
    for m in mem:
        starts.append(at)
        at += len(m)

    eng = zsamd.Engine(0)
    arr = lambda ctype, v: (ctype * len(v))(*v)
    d_one = torch.frombuffer(bytearray(one_file + b"\0" * 16), dtype=torch.uint8).cuda()
    cap = (total + 3) & ~3
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    res = [torch.zeros(max(M, 8), dtype=torch.int32, device="cuda") for _ in range(5)]
    d_chk = torch.zeros(max(M, 8), dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in res]
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    assert mb % 4 == 0
    one = (1, d_one.data_ptr(), arr(u64, [0]), arr(u32, [len(one_file)]), d_out.data_ptr(), arr(u64, [0]), arr(u32, [cap]))
    configs = {
        "plain/members": (dict(), (M, d_one.data_ptr(), arr(u64, starts), arr(u32, [len(m) for m in mem]), d_out.data_ptr(),
                                   arr(u64, cuts[:-1]), arr(u32, [(cuts[k + 1] - cuts[k] + 3) & ~3 for k in range(M)]))),
        "members/one": (dict(members=True), one),
        "bgzf/one": (dict(members="bgzf"), one),
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
    index = list(zip(starts, cuts[:-1])) + [(len(one_file) - 28, total)]
    checks = {}
    for name in configs:
        d_out.zero_()
        for _ in range(a.warmup):
            n = run(name)
        torch.cuda.synchronize()
        assert int((res[0][:n] != 1).sum()) == 0, "some streams failed (%s)" % name
        assert zlib.crc32(bytes(d_out[:total].cpu().numpy())) == want, "wrong output (%s)" % name
        if n == 1:
            assert int(res[3][0]) & 0xffffffff == total and int(d_chk[0]) & 0xffffffff == want, name
            checks[name] = {"index_equals_the_boundaries": eng.last_members()[0] == index, "trusted": eng.last_bgzf_trusted()}
    assert checks["bgzf/one"]["trusted"] == M + 1 and checks["members/one"]["trusted"] == 0
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
    q = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    med = lambda c: statistics.median(dev[c])
    pm = lambda c, ph: round(statistics.median(phases[c][ph]), 4)
    out = {"mib": a.mib, "member_bytes": mb, "members": M, "level": a.level, "file_bytes": len(one_file),
           "build_id": zsamd.build_id(), "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "checks": checks,
           "bgzf_device_ms": round(med("bgzf/one"), 4),
           "bgzf_over_floor": round(med("bgzf/one") / med("plain/members"), 3),
           "bgzf_over_members": round(med("bgzf/one") / med("members/one"), 3),
           "members_over_floor": round(med("members/one") / med("plain/members"), 3),
           "bgzf_size_ms": pm("bgzf/one", "bgzf_size"), "members_scan_ms": pm("bgzf/one", "members_scan"), "configs": {}}
    for c in configs:
        out["configs"][c] = {"calls": len(dev[c]), "device_ms": q(dev[c]), "wall_ms": q(wall[c]),
                             "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[c].items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
