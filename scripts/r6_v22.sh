cd $GRAFT_REPO_ROOT
OUT=${OUT:-results}; mkdir -p "$OUT"; export OUT  # where this script leaves its logs
REPO=$PWD
mkdir -p "$OUT"; rm -rf /tmp/prof /tmp/lkt; mkdir -p /tmp/prof
( cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -o r6 -- python "$REPO/bench.py" --full --steps 20 --warmup 5 --no-cpu-baseline --no-pmc --no-configs ) > $OUT/r6_v22_prof.log 2>&1
tail -2 $OUT/r6_v22_prof.log | cut -c1-400
find /tmp/prof -name "*kernel_stats*.csv" -exec cp {} $OUT/r6_v22_kernel_stats.csv \;
head -25 $OUT/r6_v22_kernel_stats.csv | cut -c1-200
bash scripts/r6_prof.sh r6_v22_final 2 | tail -75
python scripts/sum_by_shape.py $OUT/r6_v22_final_by_shape.txt 15
