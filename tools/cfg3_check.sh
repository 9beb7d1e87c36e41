#!/bin/bash
# One-GPU configs[3] path (k_plan2 / k_logscan / k_emit2 after k_plan2): the plan-path and
# full-size parity tests, then the configs[3] bench line twice.
set -o pipefail
R=$(pwd); mkdir -p bench_out
T=${1:-c3}
timeout -k 10 900 python -u -m pytest tests/test_gpu_parity.py -k "plan or config3 or logscan or fill_levels" \
    "tests/test_full_size.py" -m gpu -x -q --timeout 300 --timeout-method thread > bench_out/${T}_pytest.log 2>&1 \
    || { tail -40 bench_out/${T}_pytest.log; exit 1; }
tail -2 bench_out/${T}_pytest.log
for i in 1 2; do
  timeout -k 10 300 python -u bench.py --full --workload cfg3 --no-cpu-baseline --no-host-observed > bench_out/${T}_cfg3_$i.json 2> bench_out/${T}_cfg3_$i.err || { tail -20 bench_out/${T}_cfg3_$i.err; exit 3; }
  python -c "import json; d=json.load(open('bench_out/${T}_cfg3_$i.json')); print(round(d['ms_per_step']*1e3,2), 'us/tick', {k: round(v*1e3,2) for k,v in d['tick']['kernels_avg_ms'].items()}, round(d['roofline']['tick_frac'],3))"
done
