#!/bin/bash
# Full GPU check: the -m gpu suite with per-test durations, smoke, the bench line as the driver runs it.
# Usage: gpurun --timeout 1700 -- 'bash scripts/gpu_full.sh'
# Writes its logs to $OUT (default: out/ in the repository).
set -u
export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-.}"
OUT=$(mkdir -p "${OUT:-out}" && cd "${OUT:-out}" && pwd)
t0=$(date +%s)
timeout 1300 python -m pytest tests -m gpu -x -q --durations=60 2>&1 | tail -90 > "$OUT/pytest_gpu.log"
echo "pytest wall: $(( $(date +%s) - t0 )) s" >> "$OUT/pytest_gpu.log"
tail -5 "$OUT/pytest_gpu.log"
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3 | tee "$OUT/smoke.log"
timeout 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full 2>"$OUT/bench.err" | tail -1 > "$OUT/bench.json"
python - "$OUT/bench.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print("ms_per_step", d["ms_per_step"], "value", d["value"], "kernel_ms", d["roofline"]["kernel_ms"],
      "parity", d.get("parity_checked"), d.get("parity_ok"), "regions", d["repeated"]["region_ms"])
PY
