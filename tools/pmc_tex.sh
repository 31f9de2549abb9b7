#!/bin/bash
# Texture-path counter passes (TA, TCP, TCC) for the deflate kernels, one rocprofv3 --pmc pass
# per counter group, into the directory of tools/pmc_sq.sh (its summary then lists both).
# usage: tools/pmc_tex.sh OUTDIR [bench args...]
cd "$(dirname "$0")/.."
OUT=$1; shift
mkdir -p "$OUT"
i=0
# (at most two TA and four TCP or TCC counters fit one pass: a larger group is refused when the
# first kernel starts)
for group in "TCP_TOTAL_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_PENDING_STALL_CYCLES_sum TCP_TCP_TA_DATA_STALL_CYCLES_sum" \
             "TA_BUSY_avr TA_FLAT_READ_WAVEFRONTS_sum GRBM_GUI_ACTIVE" \
             "TCC_REQ_sum TCC_READ_sum TCC_HIT_sum TCC_MISS_sum" \
             "TA_ADDR_STALLED_BY_TC_CYCLES_sum TA_DATA_STALLED_BY_TC_CYCLES_sum"; do
  i=$((i+1))
  timeout -k 10 90 rocprofv3 --pmc $group --output-format csv -d "$OUT/sqtex$i" -o run -- python3 bench.py --no-cpu-baseline --no-shard-sweep --no-e2e --no-verify --steps 2 --warmup 1 "$@" > "$OUT/sqtex$i.log" 2>&1 || exit $?
done
python3 tools/sq_summary.py "$OUT" zs_k_ --json "$OUT/sq_summary.json" > "$OUT/sq_summary.txt"
echo pmc-done
