set -x
OUT=$(realpath -m ${1:?usage: bash tools/profile_round.sh OUTDIR})
mkdir -p $OUT && cd /tmp && export TMPDIR=/tmp
R=/root/repo
rocprofv3 -L > $OUT/counters.txt 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/kt -- python3 $R/bench.py --full --no-cpu-baseline --no-exact-fp32 > $OUT/bench_under_rocprof.json 2> $OUT/kt.err
B="python3 $R/bench.py --no-graph --steps 3 --warmup 1 --no-cpu-baseline --no-kernel-timing --no-exact-fp32"
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_fetch -- $B > $OUT/pmc_f.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_write -- $B > $OUT/pmc_w.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU SQ_WAIT_INST_LDS SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU -d $OUT/pmc_lds -- $B > $OUT/pmc_l.log 2>&1
rocprofv3 --kernel-trace --pmc SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU -d $OUT/pmc_mfma -- $B > $OUT/pmc_m.log 2>&1
cd $R
python tools/profile_summary.py $(ls $OUT/kt/*/*.db | head -1) $OUT/kernel_stats.csv > $OUT/fam.txt 2>&1
python tools/collect_traffic.py $OUT/pmc_fetch $OUT/pmc_write $OUT/traffic.json > $OUT/traffic.txt 2>&1
python tools/collect_pmc.py $OUT/pmc_lds $OUT/pmc_mfma $OUT/pmc_sq.json > $OUT/pmc_sq.txt 2>&1
rm -rf $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_lds $OUT/pmc_mfma $OUT/kt
echo done
