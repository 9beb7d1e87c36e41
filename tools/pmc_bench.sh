#!/bin/bash
# GPU box: one rocprofv3 --pmc pass (+ kernel trace) of a bench.py run, per-kernel counter averages.
#   PMC="<counters>" tools/pmc_bench.sh TAG [bench args]   -> bench_out/pmcb_TAG/
set -o pipefail
R=$(pwd); mkdir -p bench_out
T=$1; shift
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 150 rocprofv3 --kernel-trace --pmc $PMC --output-format csv -d $R/bench_out/pmcb_$T -o run -- \
    python3 $R/bench.py --full --no-cpu-baseline --no-host-observed "$@" > $R/bench_out/pmcb_$T.json 2> $R/bench_out/pmcb_$T.err || { tail -5 $R/bench_out/pmcb_$T.err; exit 1; }
python3 $R/tools/pmc_kernels.py $R/bench_out/pmcb_$T
