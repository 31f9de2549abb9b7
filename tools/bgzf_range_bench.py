#!/usr/bin/env python3
"""BGZF ranges by virtual offset: tools/bgzf_bench.py's file -- 64 MiB of the T corpus as ONE BGZF
file of 65,280-byte blocks at level 6 plus the end-of-file block, made by zlib on the host -- read on the device in
one process and in alternating rounds --
  bgzf/one         the _bgzf call over the one file
  range/whole      the _bgzf_range call with the range (0, file_bytes << 16) over it: the same blocks, every one through
                   staging and the place kernel -- the difference is the staging and the "bgzf_range_place" phase
  plain/touched    the plain gzip batch over exactly the blocks the 4,096 ranges below touch, a block once per range
                   that touches it, with their boundaries given: the decode alone, the floor of range/4096
  range/4096       4,096 ranges of one to three blocks at random virtual offsets, all naming the one file, in one call
  range/one        one range of two blocks alone: the call's latency
Prints one JSON line (and writes it to --out): per configuration the median, minimum and maximum of the call's device
time (zs_last_batch_ms: first to last mark on the stream, so the host planning in the middle counts) and of its wall
time over --steps timed calls, taken in --rounds rounds that alternate the configurations, after --warmup untimed
calls of each; the phases' medians; range/whole over bgzf/one and range/4096 over its floor.

    python tools/bgzf_range_bench.py [--mib 64] [--ranges 4096] [--steps 7] [--rounds 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zlib-streams-ts_amd"))

PHASES = ("bgzf_range_end", "bgzf_range_wait", "members_scan", "bgzf_size", "members_stitch", "bgzf_range_place",
          "checksum", "inflate_lane", "inflate", "inflate_check", "restart_place", "finish")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--member-bytes", type=int, default=65280)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=7, help="timed calls per configuration and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
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
    F = len(one_file)
    starts, at = [], 0
    for m in mem:
        starts.append(at)
        at += len(m)
    isize = [cuts[k + 1] - cuts[k] for k in range(M)]
    assert zsamd.bgzf_range_out_len(one_file, 0, F << 16) == total

    # the ranges: a first block, one to three blocks, a position in the first and in the last
    r = random.Random(17)
    ranges, spans, touched = [], [], []
    for _ in range(a.ranges):
        k0 = r.randrange(M)
        k1 = min(M - 1, k0 + r.randrange(3))
        ub = r.randrange(isize[k0])
        ue = r.randrange(ub + 1 if k1 == k0 else 1, isize[k1] + 1)
        ranges.append(((starts[k0] << 16) | ub, (starts[k1] << 16) | ue))
        spans.append((cuts[k0] + ub, cuts[k1] + ue))
        touched += list(range(k0, k1 + 1))
    R, Tn = len(ranges), len(touched)
    caps = [(e - b + 3) & ~3 for b, e in spans]
    two = ((starts[M // 2] << 16) | 1000, (starts[M // 2 + 1] << 16) | 2000)
    two_span = (cuts[M // 2] + 1000, cuts[M // 2 + 1] + 2000)

    eng = zsamd.Engine(0)
    arr = lambda ctype, v: (ctype * len(v))(*v)
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    d_one = torch.frombuffer(bytearray(one_file + b"\0" * 16), dtype=torch.uint8).cuda()
    cap = (total + 3) & ~3
    t_off, o = [], 0
    for k in touched:
        t_off.append(o)
        o += (isize[k] + 3) & ~3
    r_off, q = [], 0
    for c in caps:
        r_off.append(q)
        q += c
    d_out = torch.zeros(max(cap, o, q) + 64, dtype=torch.uint8, device="cuda")
    nres = max(M, R, Tn, 8)
    res = [torch.zeros(nres, dtype=torch.int32, device="cuda") for _ in range(5)]
    d_chk = torch.zeros(nres, dtype=torch.int32, device="cuda")
    ptrs = [t.data_ptr() for t in res]
    one = (1, d_one.data_ptr(), arr(u64, [0]), arr(u32, [F]), d_out.data_ptr(), arr(u64, [0]), arr(u32, [cap]))
    configs = {
        "bgzf/one": (dict(members="bgzf"), one),
        "range/whole": (dict(members="bgzf", ranges=[(0, F << 16)]), one),
        "plain/touched": (dict(), (Tn, d_one.data_ptr(), arr(u64, [starts[k] for k in touched]),
                                   arr(u32, [len(mem[k]) for k in touched]), d_out.data_ptr(), arr(u64, t_off),
                                   arr(u32, [(isize[k] + 3) & ~3 for k in touched]))),
        "range/4096": (dict(members="bgzf", ranges=ranges),
                       (R, d_one.data_ptr(), arr(u64, [0] * R), arr(u32, [F] * R), d_out.data_ptr(), arr(u64, r_off),
                        arr(u32, caps))),
        "range/one": (dict(members="bgzf", ranges=[two]),
                      (1, d_one.data_ptr(), arr(u64, [0]), arr(u32, [F]), d_out.data_ptr(), arr(u64, [0]),
                       arr(u32, [(two_span[1] - two_span[0] + 3) & ~3]))),
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
    checks = {}
    for name in configs:
        d_out.zero_()
        for _ in range(a.warmup):
            n = run(name)
        torch.cuda.synchronize()
        assert int((res[0][:n] != 1).sum()) == 0, "some streams failed (%s)" % name
        chk = [x & 0xffffffff for x in d_chk[:n].tolist()]
        lens = [x & 0xffffffff for x in res[3][:n].tolist()]
        if name in ("bgzf/one", "range/whole"):
            assert zlib.crc32(bytes(d_out[:total].cpu().numpy())) == want, "wrong output (%s)" % name
            assert lens == [total] and chk == [want], name
            checks[name] = {"trusted": eng.last_bgzf_trusted()}
        elif name == "range/4096":
            assert lens == [e - b for b, e in spans], name
            assert chk == [zlib.crc32(host[b:e]) for b, e in spans], "wrong output (%s)" % name
            out = bytes(d_out[:q].cpu().numpy())
            assert all(out[r_off[i]:r_off[i] + lens[i]] == host[spans[i][0]:spans[i][1]] for i in range(0, R, 97)), name
            checks[name] = {"trusted": eng.last_bgzf_trusted(), "blocks_touched": Tn}
            assert checks[name]["trusted"] == Tn
        elif name == "range/one":
            assert lens == [two_span[1] - two_span[0]] and chk == [zlib.crc32(host[two_span[0]:two_span[1]])], name
        else:
            assert lens == [isize[k] for k in touched], name
    assert checks["bgzf/one"]["trusted"] == M + 1 and checks["range/whole"]["trusted"] == M + 1
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
    qq = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    med = lambda c: statistics.median(dev[c])
    pm = lambda c, ph: round(statistics.median(phases[c][ph]), 4) if ph in phases[c] else None
    out = {"mib": a.mib, "member_bytes": mb, "members": M, "level": a.level, "file_bytes": F, "ranges": R,
           "blocks_touched": Tn, "range_bytes": sum(e - b for b, e in spans), "build_id": zsamd.build_id(),
           "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "checks": checks,
           "whole_minus_bgzf_ms": round(med("range/whole") - med("bgzf/one"), 4),
           "whole_place_ms": pm("range/whole", "bgzf_range_place"),
           "whole_over_bgzf": round(med("range/whole") / med("bgzf/one"), 3),
           "ranges_over_floor": round(med("range/4096") / med("plain/touched"), 3),
           "one_range_device_ms": round(med("range/one"), 4),
           "one_range_wall_ms": round(statistics.median(wall["range/one"]), 4), "configs": {}}
    for c in configs:
        out["configs"][c] = {"calls": len(dev[c]), "device_ms": qq(dev[c]), "wall_ms": qq(wall[c]),
                             "phase_ms": {k: round(statistics.median(v), 4) for k, v in phases[c].items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
