#!/bin/bash
# The round's evidence in one gpurun call (from the repo root on the GPU box; copy the results into profiles/ afterwards):
#   bash tools/refresh_profiles.sh <round tag, e.g. r04> [notraffic] [output directory]
# bench lines (default / --stage frontend / --mixed / --batch 1 --latency / --dtype bf16), rocprofv3 --kernel-trace --stats of the
# default workload and of the batch-1 latency run and, unless `notraffic`, the two PMC passes of tools/collect_traffic.sh and the
# matrix-pipe busy pass of tools/collect_mfma_util.sh
# (write `git rev-parse --short HEAD > .build_commit` before the call).
# The bench lines are --full runs (roofline, CPU baseline, parity, transfer-inclusive region); results go to the directory
# given as the third argument (default bench_out/).
set -e
TAG=${1:-r04}
ROOT=$(pwd)
OUT=${3:-bench_out}
mkdir -p $OUT
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
tail -c 400 $OUT/${TAG}_bench.json; echo
python bench.py --full --stage frontend > $OUT/${TAG}_bench_frontend.json 2> $OUT/${TAG}_bench_frontend.err
python bench.py --full --mixed > $OUT/${TAG}_bench_mixed.json 2> $OUT/${TAG}_bench_mixed.err
python bench.py --full --batch 1 --latency > $OUT/${TAG}_bench_b1.json 2> $OUT/${TAG}_bench_b1.err
python bench.py --full --dtype bf16 --no-transfers --cpu-clips 4 --cpu-warm 1 > $OUT/${TAG}_bench_bf16.json 2> $OUT/${TAG}_bench_bf16.err
echo benches done
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_${TAG} -o bench -- python3 $ROOT/bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-transfers > $ROOT/$OUT/${TAG}_bench_under_rocprof.json 2>&1)
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $ROOT/$OUT/prof_${TAG}_b1 -o bench -- python3 $ROOT/bench.py --full --batch 1 --latency --requests 50 > $ROOT/$OUT/${TAG}_bench_b1_under_rocprof.json 2>&1)
echo rocprof done
if [ "$2" != "notraffic" ]; then
  bash tools/collect_traffic.sh $OUT/${TAG}_traffic.json 640
  echo traffic done
  bash tools/collect_mfma_util.sh $OUT/${TAG}_mfma_util.json 640
  echo mfma util done
fi
