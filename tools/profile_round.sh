#!/bin/bash
# Profiling recipe of a round (run on a GPU machine):  tools/profile_round.sh <tag>   (results under $OUT, default out/)
# 1. bench.py --full with its defaults (detect + BA + CPU baseline + the traffic passes) -> $OUT/bench_<tag>.json
# 2. rocprofv3 --kernel-trace --stats of the same command -> $OUT/prof_<tag>/
# 3. two PMC passes (FETCH_SIZE, WRITE_SIZE; separate runs, kernel-trace only) -> $OUT/pmc_<tag>_{fetch,write}/   (SKIP_PMC=1 leaves them out)
tag=${1:-rX}
R=$(pwd)
OUT=${OUT:-$R/out}
export TMPDIR=/tmp
mkdir -p $OUT
python bench.py --full > $OUT/bench_${tag}.json 2> $OUT/bench_${tag}.err
tail -c 3000 $OUT/bench_${tag}.json
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${tag} -o prof -- python $R/bench.py --full --no-measure-traffic --steps 10 --warmup 2 --no-cpu-baseline --rp-frames 0 --latency-calls 0 --lines-images 0 > $OUT/bench_prof_${tag}.log 2>&1
if [ -z "$SKIP_PMC" ]; then
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_${tag}_fetch -o pmc -- python $R/bench.py --full --no-measure-traffic --steps 3 --warmup 1 --no-cpu-baseline --ba-iters 3 --inflight 1 --rp-frames 0 --latency-calls 0 --lines-images 0 > $OUT/pmc_${tag}_fetch.log 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_${tag}_write -o pmc -- python $R/bench.py --full --no-measure-traffic --steps 3 --warmup 1 --no-cpu-baseline --ba-iters 3 --inflight 1 --rp-frames 0 --latency-calls 0 --lines-images 0 > $OUT/pmc_${tag}_write.log 2>&1
cd $R
python tools/pmc_summary.py $OUT/pmc_${tag}_fetch $OUT/pmc_${tag}_write $OUT/pmc_${tag}_traffic.json > $OUT/pmc_${tag}_summary.csv
cat $OUT/pmc_${tag}_summary.csv | head -40
# the raw counter dumps are large; keep the summaries
find $OUT/pmc_${tag}_fetch $OUT/pmc_${tag}_write -name '*counter_collection.csv' -size +20M -delete
fi
cd $R
find $OUT/prof_${tag} -name '*kernel_trace.csv' -size +20M -delete
