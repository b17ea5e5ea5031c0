#!/bin/bash
# Final check of the tree on a GPU machine: the GPU suite, smoke() and the full benchmark line, logged into OUTPUT_DIR.
OUT=$(realpath -m "${1:?usage: tools/final_check.sh OUTPUT_DIR}")
cd "$(dirname "$0")/.."
mkdir -p "$OUT"
( time timeout 2000 python -m pytest tests -m gpu -x -q ) > "$OUT/r06_suite_final.log" 2>&1
tail -5 "$OUT/r06_suite_final.log"
( time python -c "import __graft_entry__ as g; g.smoke()" ) > "$OUT/r06_smoke_final.log" 2>&1
tail -2 "$OUT/r06_smoke_final.log"
( time python bench.py --full ) > "$OUT/r06_bench_final.json" 2> "$OUT/r06_bench_final.err"
BENCH_LINE="$OUT/r06_bench_final.json" python - <<'PY'
import json, os
s=[l for l in open(os.environ['BENCH_LINE']).read().splitlines() if l.startswith('{')][-1]
d=json.loads(s)
print('headline', d['ms_per_step'], d['roofline']['frac'], d['roofline'].get('traffic_measured'))
for q,c in d['configs'].items(): print(q, c.get('ms_per_step'), c.get('frac'), c.get('error'))
PY
