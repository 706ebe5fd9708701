cd $GRAFT_REPO_ROOT
OUT=${OUT:-results}; mkdir -p "$OUT"; export OUT  # where this script leaves its logs
timeout 1500 python -m pytest tests/test_hip_kernels.py -x -q -m gpu -k "three_mfma or absmax or fused_hop or test_gemm_nn or test_gemm_tn or edge_attention or gelu or bn_relu or column_stat or prepacked" 2>&1 | tail -25 > $OUT/r6_v2_tests.txt
cat $OUT/r6_v2_tests.txt
timeout 900 python bench.py --full > $OUT/r6_v2_bench.json 2> $OUT/r6_v2_bench.err; tail -c 600 $OUT/r6_v2_bench.err
python - <<'PY'
import json, os
d=json.loads(open(os.environ['OUT'] + '/r6_v2_bench.json').read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d.get('breakdown_ms_per_step'))
PY
