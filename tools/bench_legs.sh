#!/bin/bash
# the full bench line (every leg) on the GPU host, timed, with a per-leg summary: bash tools/bench_legs.sh <tag>
# (writes $BENCH_OUT/<tag>.json and .err; BENCH_OUT defaults to bench_out/ in the repository root)
set +e
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
tag=${1:-b}; out=${BENCH_OUT:-bench_out}; mkdir -p "$out"
t0=$(date +%s)
timeout -k 10 700 python bench.py --full > "$out/${tag}.json" 2> "$out/${tag}.err"; rc=$?
echo "bench rc=$rc, $(( $(date +%s) - t0 )) s"; [ $rc -ne 0 ] && { tail -5 "$out/${tag}.err"; exit $rc; }
tail -1 "$out/${tag}.json" | python3 -c "
import json, sys
d = json.loads(sys.stdin.read())
print('value', d['value'], 'frac', d['roofline']['frac'], 'seal', d['seal_GiBps'], 'open', d['open_GiBps'])
for k, v in d['extra'].items():
    print(k, v['value'], v.get('seal_GiBps'), v.get('open_GiBps'), v.get('verified'))
"
