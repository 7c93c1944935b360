#!/bin/bash
# Where a batched search on the int8 candidate copy goes, beside the bf16 copy on the same vectors
# (profiles/int8_search/README.md): one rocprofv3 --kernel-trace --stats run of
# scripts/search_bench.py --copy both, then -- each its own run, counter collection serialises
# dispatches -- one --pmc pass for the MFMA busy cycles and one for the bytes the L2 fetched.
#   OUT=dir SLOTS=n PMC_SLOTS=n bash scripts/gpu_prof_search_int8.sh
set -o pipefail
OUT=${OUT:-bench_outputs/int8_prof}
SLOTS=${SLOTS:-25000000}
PMC_SLOTS=${PMC_SLOTS:-4000000}
ROOT=$(pwd)
mkdir -p "$OUT"
export TMPDIR=/tmp SPLINTER_HBM_VEC8=1
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOT/$OUT/trace" -o run -- \
  python3 scripts/search_bench.py --slots "$SLOTS" --nq 256 --iters 3 --copy both --data iid \
  > "$OUT/trace.out" 2> "$OUT/trace.err" || { tail -20 "$OUT/trace.err"; exit 1; }
pmc() {  # pmc NAME COUNTERS...
  local name=$1; shift
  timeout -k 10 400 rocprofv3 --pmc "$@" --output-format csv -d "$ROOT/$OUT/$name" -o run -- \
    python3 scripts/search_bench.py --slots "$PMC_SLOTS" --nq 256 --iters 1 --copy both --data iid \
    > "$OUT/$name.out" 2> "$OUT/$name.err" || { tail -20 "$OUT/$name.err"; return 1; }
}
pmc mfma SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE || exit 1
pmc fetch TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum GRBM_GUI_ACTIVE || exit 1
python3 - "$OUT" <<'EOF' | tee "$OUT/summary.md"
import csv, glob, sys
from collections import defaultdict
out = sys.argv[1]


def short(n):
    for k in ("k_search_side", "k_rescore", "k_search_thr", "k_search_qprep8", "k_search_qprep"):
        if k in n:  # k_search_side<OpInt8 | OpBf16, MODE>
            op = "<OpInt8" if "OpInt8" in n else "<OpBf16" if "OpBf16" in n else ""
            mode = ", 1>" if "ELi1E" in n or ", 1>" in n else ", 0>" if "ELi0E" in n or ", 0>" in n else ""
            return k + op + mode
    return None


print("| kernel | calls | avg us (kernel trace) |\n|---|---|---|")
for f in glob.glob(out + "/trace/**/*kernel_stats.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        s = short(r["Name"])
        if s:
            print(f"| {s} | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} |")
for name in ("mfma", "fetch"):
    agg = defaultdict(lambda: defaultdict(list))
    for f in glob.glob(out + f"/{name}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            s = short(r["Kernel_Name"])
            if s and "mma" in s:
                agg[s][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for s, c in sorted(agg.items()):
        m = {k: sum(v) / len(v) for k, v in c.items()}
        if name == "mfma" and m.get("GRBM_GUI_ACTIVE"):
            # busy cycles are summed over the 1024 SIMDs, GUI-active over the 8 XCDs (scripts/pmc_summary.py)
            print(f"{s}: MFMA busy {m['SQ_VALU_MFMA_BUSY_CYCLES'] / (m['GRBM_GUI_ACTIVE'] / 8 * 1024):.3f} "
                  f"({len(c['GRBM_GUI_ACTIVE'])} dispatches)")
        if name == "fetch" and "TCC_EA0_RDREQ_sum" in m:
            b = 64 * m["TCC_EA0_RDREQ_sum"] - 32 * m.get("TCC_EA0_RDREQ_32B_sum", 0.0)
            print(f"{s}: {b / 1e9:.2f} GB fetched from memory per dispatch ({m['TCC_EA0_RDREQ_sum']:.0f} read requests)")
EOF
