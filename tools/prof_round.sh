#!/bin/bash
# usage: tools/prof_round.sh r04
# round-end evidence: bench line, rocprofv3 kernel stats, HBM traffic counters (separate passes,
# --pmc never combined with the hip/hsa/sys traces) under $PROF_OUT/<round> (default prof_out/<round>).
# Then: python tools/traffic.py r03
R=${1:-r04}
OUT=${PROF_OUT:-prof_out}/$R
set -x
export TMPDIR=/tmp
mkdir -p $OUT
python bench.py --full --steps 10 --warmup 2 > $OUT/bench.json 2> $OUT/bench.err
cat $OUT/bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python3 bench.py --steps 30 --warmup 2 --no-cpu-baseline --no-ceilings --no-check --no-other-modes --no-other-configs > $OUT/stats.log 2>&1
echo stats done
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/fetch -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-ceilings --no-check --no-other-modes --no-other-configs > $OUT/fetch.log 2>&1
echo fetch done
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/write -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-ceilings --no-check --no-other-modes --no-other-configs > $OUT/write.log 2>&1
echo write done
# config 5 (streamed, per GPU): the line with its spot check, and the kernel stats of the same command
python bench.py --config 5 --steps 5 --warmup 1 --full --no-cpu-baseline > $OUT/bench_config5.json 2> $OUT/bench_config5.err
cat $OUT/bench_config5.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats5 -- python3 bench.py --config 5 --steps 4 --warmup 1 --no-cpu-baseline --no-ceilings --no-check --sustain 0 > $OUT/stats5.log 2>&1
echo config5 done
