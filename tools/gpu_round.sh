#!/bin/bash
# Round-end style evidence run: GPU tests, bench lines c2..c5, the default bench line (with the
# CPU baseline), per-shape conv table.  Each step under its own limit; stops at the first failure.
export TMPDIR=/tmp
TAG=${1:-r2}
cd "${GRAFT_REPO_ROOT}" || exit 2
mkdir -p gpurun_out
bash tools/gpu_run.sh $TAG "tests -m gpu" "c2 c3 c4 c5" || exit $?
O=${BENCH_OUT:-bench_out}; mkdir -p "$O"   # the default bench line goes here (BENCH_OUT overrides)
timeout -k 10 400 python -u bench.py --full > "$O/bench_default_$TAG.json" 2> "$O/bench_default_$TAG.err" || exit 5
timeout -k 10 300 python -u tools/conv_bench.py --math f32x3 > gpurun_out/conv_shapes_$TAG.txt 2>&1 || exit 6
timeout -k 10 300 python -u tools/conv_bench.py --math bf16 > gpurun_out/conv_shapes_bf16_$TAG.txt 2>&1 || exit 7
echo ROUND_OK
