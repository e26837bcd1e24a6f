#!/bin/bash
# round 4: same-box A/B of experiment builds of the library (make p16v TAG=...) on the whole step: bench line + per-op table,
# alternating libraries.  Usage: r4_lib_ab.sh <name> <tag> [<tag> ...]   ("base" = the product library)
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
res=${RESULTS_DIR:-results}; mkdir -p $res     # where the results go
export TMPDIR=/tmp
NAME=$1; shift
TAGS=${@:-base}
for rep in 1 2; do
for tag in $TAGS; do
  if [ $tag = base ]; then unset LP_HIP_LIB; else export LP_HIP_LIB=$GRAFT_REPO_ROOT/yolo-lp_amd/libyololp_hip_p16v_$tag.so; fi
  timeout -k 10 300 python bench.py --full --steps 50 --warmup 5 --no-cpu-baseline --detail $res/r4_${NAME}_perop_${tag}_$rep.txt > $res/r4_${NAME}_bench_${tag}_$rep.json 2> $res/r4_${NAME}_bench_${tag}_$rep.err || exit 1
  python - <<PY
import json
d=json.loads(open('$res/r4_${NAME}_bench_${tag}_$rep.json').read().strip().splitlines()[-1]); r=d['roofline']
print('$tag', 'value', d['value'], 'inflight1', d['value_inflight1'], 'frac_event', r['frac_event'], 'backbone', r.get('backbone_frac'), 'fwd_ms', r['forward_device_ms'])
PY
done
done
