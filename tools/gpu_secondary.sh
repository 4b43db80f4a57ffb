#!/bin/bash
# tools/gpu_secondary.sh OUT_DIR -- the cfg2 and cfg5 lines with their per-kernel split and roofline (one JSON file per workload)
cd "$(dirname "$0")/.."; export HSA_ENABLE_IPC_MODE_LEGACY=0
OUT=${1:?usage: tools/gpu_secondary.sh OUT_DIR}; mkdir -p "$OUT"
for w in cfg2 cfg5; do
  P=f16x3; S=6; [ $w = cfg5 ] && P=bf16 && S=2
  timeout 600 python bench.py --workload $w --precision $P --steps $S --warmup 1 --full --no-cpu-baseline --no-secondary --no-tokenizer-leg > "$OUT/$w.json" 2> "$OUT/$w.err"
  python - <<PY
import json
d=json.loads(open("$OUT/$w.json").read().strip().splitlines()[-1])
print("$w", round(d["ms_per_step"],2), round(d["value"]), {k: round(v,2) for k,v in d["kernel_ms_per_step"].items()}, d["roofline"]["kernel"], round(d["roofline"]["frac"],3), d["config"]["workload"])
PY
done
