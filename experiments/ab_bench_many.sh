#!/bin/bash
# bench.py over several library builds (round robin, twice): bash experiments/ab_bench_many.sh "libA libB ..." bench args...
export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT}" || exit 2
LIBS=$1; shift
for rep in 1 2; do
for L in $LIBS; do
  O=${BENCH_OUT:-bench_out}; mkdir -p "$O"
  ADAPTSEG_LIBRARY=adaptsegnet_amd/lib/$L timeout -k 10 300 python -u bench.py --full --no-cpu-baseline "$@" > "$O/abb.json" 2>/dev/null || exit 4
  python -c "import json,sys; d=json.loads(open(sys.argv[2]).read().strip().splitlines()[-1]); r=d.get('roofline',{}); print(sys.argv[1], d['config']['workload'][:3], round(d['value'],3), 'img/s', round(d['ms_per_step'],2), 'ms frac', r.get('frac'))" $L "$O/abb.json"
done
done
