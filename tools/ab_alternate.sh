#!/bin/bash
# A/B of two libzsgpu.so builds in one session, runs alternating A, B, A, B, ...
# (timing only).  Each run sits under its own timeout and the first failing run
# ends the script.  Prints per build the median / min / max of ms_per_step and
# of one phase of phase_ms (PHASE, default sweep).
# usage: [PHASE=parse] tools/ab_alternate.sh OUTDIR RUNS LIB_A LIB_B [bench args...]
set -u
cd "$(dirname "$0")/.."
OUT=$1; RUNS=$2; A=$3; B=$4; shift 4
mkdir -p "$OUT"
for i in $(seq 1 "$RUNS"); do
  for side in a b; do
    lib=$A; [ $side = b ] && lib=$B
    ZS_LIB=$lib timeout -k 10 150 python3 bench.py --no-cpu-baseline --no-shard-sweep --no-e2e --no-verify \
      --steps 20 --warmup 5 "$@" > "$OUT/${side}_$i.log" 2>&1 || { echo "$lib run $i failed"; tail -3 "$OUT/${side}_$i.log"; exit 1; }
  done
done
python3 - "$OUT" "$RUNS" "$A" "$B" "${PHASE:-sweep}" <<'EOF'
import json, statistics, sys
out, runs, libs, phase = sys.argv[1], int(sys.argv[2]), {"a": sys.argv[3], "b": sys.argv[4]}, sys.argv[5]
for side in "ab":
    rs = [json.loads(open("%s/%s_%d.log" % (out, side, i)).read().strip().splitlines()[-1]) for i in range(1, runs + 1)]
    ms = [r["ms_per_step"] for r in rs]
    sw = [r["roofline"]["phase_ms"].get(phase, 0.0) for r in rs]
    print("%s %-40s ms_per_step median %.3f min %.3f max %.3f | %s median %.3f min %.3f max %.3f | runs %s" % (
        side, libs[side], statistics.median(ms), min(ms), max(ms), phase, statistics.median(sw), min(sw), max(sw),
        " ".join("%.3f" % x for x in ms)))
EOF
