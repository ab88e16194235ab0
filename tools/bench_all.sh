#!/bin/bash
# One full bench.py line per BASELINE config into OUTDIR/<tag>_bench_<workload>.json, each step
# under its own time limit; stops at the first failure.  usage: tools/bench_all.sh TAG [OUTDIR]
set -o pipefail
TAG=${1:?tag}
OUT=${2:-bench_out}
mkdir -p "$OUT"
for w in kaggle-d128-b2048 kaggle-d16-b2048 kaggle-d128-b8192-bf16 terabyte-d128-bf16-zipf pooled-64x256-l10; do
  timeout -k 10 300 python bench.py --full --workload $w > "$OUT/${TAG}_bench_$w.json" || { echo "bench $w failed"; exit 1; }
  python -c "import json;d=json.load(open('$OUT/${TAG}_bench_$w.json'));s=d['sustained'];print('$w',d['value'],s and s['value'],d['ms_per_step'],{k:v['us'] for k,v in d['roofline']['stages'].items()})"
done
