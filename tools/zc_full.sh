#!/bin/bash
# tools/zc_full.sh -- z-chunk length of the fused kernels on the whole 513^3 grid (one GPU): MG_J2_ZC forced
set -eo pipefail
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${OUT:-$ROOT/bench_out/zcfull}
cd "$ROOT"; mkdir -p "$OUT"
for zc in 0 24 26 29 31 35 37 40 47; do
  MG_J2_ZC=$zc python3 bench.py --full --no-cpu-baseline --steps 20 --warmup 3 > "$OUT/zc$zc.json"
  python3 - "$zc" "$OUT" <<'PY'
import json,sys
d=json.load(open(f'{sys.argv[2]}/zc{sys.argv[1]}.json'))
k={x['kernel'][:4]:x['launch_ms'] for x in d['kernels']}
print(f"zc={sys.argv[1]:>2} cycle {d['ms_per_step']:.3f} ms  pair {d['roofline']['launch_ms']*1e3:.1f} us  corr/rr {[round(v*1e3,1) for v in k.values()]}")
PY
done
