"""Counters of zs_k_sweep per 64-member chunk on the C2 batch (a counter build:
tools/build_variant.sh swprof deflate_sweep.hip -DZS_SW_PROF=1, then
ZS_LIB=variants/swprof/libzsgpu.so python3 tools/dbg/sweep_stats.py)."""
import ctypes, os, sys
sys.path.insert(0, "zlib-streams-ts_amd")
import torch; torch.cuda.init()
import zsamd
e = zsamd.Engine(0)
buf = bytes(zsamd.corpus("text", 0, 4096, 65536))
ins = [buf[i * 65536:(i + 1) * 65536] for i in range(4096)]
e.compress_batch_raw(ins, "deflate-raw", 6)
out = (ctypes.c_ulonglong * 8)()
print("rc", zsamd.lib().zs_sw_stats(out))
names = ["chunks", "fast groups", "ends groups", "long branches", "wave steps behind the opening group",
         "ends and opening groups reading winners' keys",
         "ends groups failing validation", "opening groups failing validation"]
for i, nm in enumerate(names):
    print(nm, out[i], "per chunk %.2f" % (out[i] / max(1, out[0])))
