#!/bin/bash
# Whole-tree check on the GPU box: GPU tests, smoke, the default bench with its parity leg and CPU
# baselines (--full), the plain-launched two-rank bench (bench.py spawns its ranks; gloo backend so
# both share the one GPU), and the config-4 two-rank bench with the default batched exchange.
# usage: bash tools/final_check.sh <tag>      (logs and lines go to $BENCH_OUT, default bench_out/)
set -u
TAG=$1
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${BENCH_OUT:-bench_out}
cd $R && mkdir -p $OUT
timeout -k 10 700 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1 || { echo "pytest failed"; tail -40 $OUT/pytest_$TAG.log; exit 10; }
tail -2 $OUT/pytest_$TAG.log
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || { tail -20 $OUT/smoke_$TAG.log; exit 11; }
tail -2 $OUT/smoke_$TAG.log
timeout -k 10 300 python -u bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -20 $OUT/bench_$TAG.err; exit 12; }
cat $OUT/bench_$TAG.json
GGRS_BENCH_BACKEND=gloo timeout -k 10 300 python -u bench.py --gpus 2 --full --no-cpu-baseline > $OUT/bench2_$TAG.json 2> $OUT/bench2_$TAG.err || { tail -20 $OUT/bench2_$TAG.err; exit 13; }
cat $OUT/bench2_$TAG.json
GGRS_BENCH_BACKEND=gloo timeout -k 10 300 python -u bench.py --gpus 2 --config 4 --no-cpu-baseline > $OUT/bench2c4_$TAG.json 2> $OUT/bench2c4_$TAG.err || { tail -20 $OUT/bench2c4_$TAG.err; exit 14; }
cat $OUT/bench2c4_$TAG.json
echo final_check done
