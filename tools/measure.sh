#!/bin/bash
# Measurement pass on one box (no test suite): the default bench line, the stream line,
# the configs[3] line and the per-rank sharded probe at configs[3].  Each step has its
# own time limit; the chain stops at the first failure.
#   bash tools/measure.sh TAG
set -o pipefail
R=$(pwd); mkdir -p bench_out
T=${1:-m}
timeout -k 10 300 python -u bench.py --full > bench_out/${T}_bench.json 2> bench_out/${T}_bench.err || { tail -20 bench_out/${T}_bench.err; exit 3; }
cat bench_out/${T}_bench.json
timeout -k 10 300 python -u bench.py --full --workload stream --no-cpu-baseline > bench_out/${T}_stream.json 2> bench_out/${T}_stream.err || { tail -20 bench_out/${T}_stream.err; exit 4; }
cat bench_out/${T}_stream.json
timeout -k 10 300 python -u bench.py --full --workload cfg3 --no-cpu-baseline > bench_out/${T}_cfg3.json 2> bench_out/${T}_cfg3.err || { tail -20 bench_out/${T}_cfg3.err; exit 5; }
cat bench_out/${T}_cfg3.json
timeout -k 10 400 python -u tools/shard_probe.py --workload cfg3 --reps 20 --gated > bench_out/${T}_shard_cfg3.log 2>&1 || { tail -20 bench_out/${T}_shard_cfg3.log; exit 6; }
cat bench_out/${T}_shard_cfg3.log
