#!/bin/bash
# A/B of the config-5 decode (tools/bench_prior.py --only sample, 16 samples x LEN positions, one window per launch)
# between this tree and a built checkout of another commit, on one box in one run: ROUNDS alternating process pairs
# of the default path, then the primed positions alone (logits not asked for), temperature 0.8 and top-k 64 of this
# tree. Every launch runs under its own time limit and the script ends at the first failure.
# Usage: tools/ab_decode.sh OTHER_TREE [ROUNDS=5] [LEN=1024] [OUTDIR=ab_out]; results in OUTDIR/ab_decode.txt
set -o pipefail
cd "$(dirname "$0")/.."
ROOT=$(pwd)
OTHER=$1; ROUNDS=${2:-5}; LEN=${3:-1024}; OUTDIR=${4:-ab_out}
mkdir -p "$OUTDIR"
export OUT="$OUTDIR/ab_decode.txt"
: > "$OUT"
ms() { python -c 'import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d["ms_per_position"], d.get("ms_per_position_repeats", ""))'; }
run() {  # run TREE LABEL [bench_prior options]
  local tree=$1 label=$2; shift 2
  local out
  out=$(cd "$tree" && timeout -k 10 120 python tools/bench_prior.py --only sample --sample-len $LEN "$@" 2>>"$ROOT/$OUTDIR/ab_decode.err") || { echo "$label failed" | tee -a "$OUT"; exit 1; }
  echo "$label $(echo "$out" | ms)" | tee -a "$OUT"
}
for r in $(seq $ROUNDS); do
  run "$OTHER" other
  run . this
done
run . primed_no_logits --prime-len $LEN --repeats 5
run . temperature_0.8 --temperature 0.8 --repeats 5
run . top_k_64 --top-k 64 --repeats 5
python - <<'EOF' | tee -a "$OUT"
import os
import statistics as st
rows = [l.split() for l in open(os.environ["OUT"])]
o = [float(r[1]) for r in rows if r[0] == "other"]
t = [float(r[1]) for r in rows if r[0] == "this"]
print(f"other median {st.median(o):.4f} spread {max(o) - min(o):.4f} | this median {st.median(t):.4f} "
      f"spread {max(t) - min(t):.4f} | this - other {st.median(t) - st.median(o):+.4f} ms per position")
EOF
