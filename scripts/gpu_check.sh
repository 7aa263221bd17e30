#!/bin/bash
# Runs on the GPU box via gpurun: GPU parity tests, smoke, bench, rocprof kernel trace.
# Usage: gpurun --timeout 1500 -- 'bash scripts/gpu_check.sh [quick]'
# Writes its logs and profiles to $OUT (default: out/ in the repository).
set -u
export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-.}"
OUT=$(mkdir -p "${OUT:-out}" && cd "${OUT:-out}" && pwd)
echo "== rocminfo" ; /opt/rocm/bin/rocminfo 2>/dev/null | grep -m3 -E "gfx|Marketing" 
echo "== pytest -m gpu"
timeout 900 python -m pytest tests -m gpu -x -q 2>&1 | tail -25 | tee "$OUT/pytest_gpu.log"
echo "== smoke"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5 | tee "$OUT/smoke.log"
echo "== bench"
timeout 600 python bench.py --full 2>&1 | tail -3 | tee "$OUT/bench.log"
if [ "${1:-}" != "quick" ]; then
  echo "== rocprofv3 kernel trace"
  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o reduce -- python "$OLDPWD/bench.py" --steps 50 --warmup 5 --no-cpu-baseline > "$OUT/prof_bench.log" 2>&1)
  tail -2 "$OUT/prof_bench.log"
  find "$OUT/prof" -name "*kernel_stats*" | head -3
  f=$(find "$OUT/prof" -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -8 "$f"
fi
if [ "${1:-}" != "quick" ]; then
  echo "== rocprofv3 PMC passes (separate runs, counters only)"
  for ctr in FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU SQ_BUSY_CYCLES; do
    (cd /tmp && timeout 600 rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d "$OUT/pmc_$ctr" -o reduce -- python "$OLDPWD/bench.py" --steps 3 --warmup 1 --no-cpu-baseline > "$OUT/pmc_$ctr.log" 2>&1)
    f=$(find "$OUT/pmc_$ctr" -name "*counter_collection.csv" | head -1)
    [ -n "$f" ] && python - "$f" $ctr <<'PY'
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
acc = collections.defaultdict(list)
for r in rows:
    acc[r.get("Kernel_Name", "?")[:60]].append(float(r.get("Counter_Value", 0)))
for k, v in acc.items():
    print(sys.argv[2], k, "dispatches", len(v), "mean", sum(v) / len(v))
PY
  done
fi
