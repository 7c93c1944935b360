#!/bin/bash
# 64-wide K stages of the 256x384 GEMM (profiles/gemm384_bk64/README.md): the parent build (its own
# tree under $PARENT, built there) beside this tree, on one GPU.
#   bash scripts/gpu_gemm384_bk64.sh prof   stall counters (one --pmc pass, bench.py --mode embed) and a
#                                           kernel trace of the timed region of the default step, per arm;
#                                           then the isolated A/B at 32768 / 25000 / 8192 tokens
#   bash scripts/gpu_gemm384_bk64.sh ab     mixed step, arms alternating, 3 rounds; then --dump-outputs of
#                                           both arms compared byte for byte
# Counter runs and traces are separate runs; every GPU step has its own limit and a failure ends the script.
set -o pipefail
OUT=${OUT:-build/gemm384_bk64}
PARENT=${PARENT:-ab_old}
ROOT=$(pwd)
mkdir -p "$OUT"
export TMPDIR=/tmp
[ -f "$PARENT/bench.py" ] || { echo "no parent tree at $PARENT"; exit 2; }
tree() { [ "$1" = parent ] && echo "$ROOT/$PARENT" || echo "$ROOT"; }

prof() {
  local C="SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE"
  local arm f
  for arm in parent new; do
    (cd "$(tree $arm)" && timeout -k 10 300 rocprofv3 --pmc $C --output-format csv -d "$ROOT/$OUT/pmc_$arm" -o run -- \
      python3 bench.py --mode embed --steps 2 --warmup 1 > "$ROOT/$OUT/pmc_$arm.out" 2> "$ROOT/$OUT/pmc_$arm.err") \
      || { tail -20 "$OUT/pmc_$arm.err"; return 1; }
    f=$(find "$OUT/pmc_$arm" -name '*counter_collection.csv' | head -1)
    python3 scripts/pmc_stalls.py "$f" > "$OUT/stall_$arm.md" || return 1
    echo "== stall counters, $arm"; head -8 "$OUT/stall_$arm.md"
    gzip -f "$f"
  done
  for arm in parent new; do
    (cd "$(tree $arm)" && SPL_PROFILE_TIMED=1 timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv \
      -d "$ROOT/$OUT/tr_$arm" -o run -- python3 bench.py --gpus 1 --steps 20 --warmup 5 \
      > "$ROOT/$OUT/tr_$arm.out" 2> "$ROOT/$OUT/tr_$arm.err") || { tail -20 "$OUT/tr_$arm.err"; return 1; }
    f=$(find "$OUT/tr_$arm" -name '*kernel_trace.csv' | head -1)
    echo "== trace, $arm"
    python3 scripts/trace_window.py "$f" "$OUT/tr_$arm.err" --md "$OUT/trace_$arm.md" | head -12 || return 1
    rm -rf "$OUT/tr_$arm"
  done
  local tok shape
  for tok in 32768 25000 8192; do
    for shape in "2 6144" "3 2304"; do
      set -- $shape
      timeout -k 10 150 python3 scripts/gemm_bench.py --mode $1 --n $2 --tokens $tok --forms 384k32,384k64 --rounds 5 \
        2> "$OUT/gemm_bench.err" | tee -a "$OUT/gemm_bench.jsonl" || { tail -20 "$OUT/gemm_bench.err"; return 1; }
    done
  done
}

ab() {
  local r arm
  for r in 1 2 3; do
    for arm in parent new; do
      (cd "$(tree $arm)" && timeout -k 10 400 python3 bench.py --gpus 1 --steps 20 --warmup 5 \
        > "$ROOT/$OUT/bench_${arm}_$r.out" 2> "$ROOT/$OUT/bench_${arm}_$r.err") || { tail -20 "$OUT/bench_${arm}_$r.err"; return 1; }
      python3 -c "
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(json.dumps({'arm': sys.argv[2], 'round': int(sys.argv[3]), 'ms_per_step': d['ms_per_step'],
                  'embed_phase_ms_per_step': d['embed_phase_ms_per_step'], 'value': d['value']}))
" "$OUT/bench_${arm}_$r.out" $arm $r | tee -a "$OUT/bench_ab.jsonl" || return 1
    done
  done
  for arm in parent new; do
    (cd "$(tree $arm)" && timeout -k 10 400 python3 bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$TMPDIR/bk64_dump_$arm" \
      > "$ROOT/$OUT/dump_$arm.out" 2> "$ROOT/$OUT/dump_$arm.err") || { tail -20 "$OUT/dump_$arm.err"; return 1; }
  done
  local n=0 f
  for f in "$TMPDIR"/bk64_dump_parent/*.npy; do
    cmp "$f" "$TMPDIR/bk64_dump_new/$(basename "$f")" || return 1
    n=$((n + 1))
  done
  echo "dumps: $n arrays byte-identical" | tee "$OUT/dumps.txt"
  [ $n -ge 6 ]
}

case "$1" in
  prof) prof ;;
  ab) ab ;;
  *) echo "usage: $0 prof|ab"; exit 2 ;;
esac
