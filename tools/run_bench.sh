OUT=${1:?usage: bash tools/run_bench.sh OUTDIR}
mkdir -p $OUT
S=$(date +%s)
python3 bench.py --full > $OUT/p3_bench_default.json 2> $OUT/p3_bench_default.err
echo "bench wall seconds: $(( $(date +%s) - S ))"
tail -c 700 $OUT/p3_bench_default.json
