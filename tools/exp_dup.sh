# timing experiments: bash tools/exp_dup.sh <variant>...  (ggrs_amd/exp/libggrs_amd_<variant>.so)
# lines (with the parity leg: --full) go to $BENCH_OUT, default bench_out/
set -u
cd ${GRAFT_REPO_ROOT}
OUT=${BENCH_OUT:-bench_out}
mkdir -p $OUT
for L in 3072 4096; do
  timeout -k 10 120 python bench.py --full --no-cpu-baseline --lanes $L > $OUT/exp_base_$L.json 2>/dev/null || exit 11
  for v in "$@"; do
    GGRS_AMD_EXP_LIB=libggrs_amd_$v.so timeout -k 10 120 python bench.py --full --no-cpu-baseline --lanes $L > $OUT/exp_${v}_$L.json 2>/dev/null || exit 12
  done
done
for f in $OUT/exp_*.json; do python3 -c "import json,sys;d=json.load(open('$f'));print('$f',d['value'],d['roofline']['avg_launch_ms'],d['parity'])"; done
