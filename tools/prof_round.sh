#!/bin/bash
# A round's measurement pass: the default bench line, stamps of the configs[2] tick, then
# kernel traces + FETCH / WRITE passes of configs[2], configs[3] and the configs[4] stream
# (tools_profile.sh; summaries into profiles/<tag>_* and profiles/traffic.json, which the
# bench lines read back as roofline.traffic), then the configs[3] and stream bench lines.
#   bash tools/prof_round.sh TAG   (then: python tools/prof_summary.py bench_out/prof_TAG_xx TAG_xx)
set -o pipefail
R=$(pwd); mkdir -p bench_out
T=${1:-r05}
timeout -k 10 300 python -u bench.py --full > bench_out/${T}_bench.json 2> bench_out/${T}_bench.err || { tail -20 bench_out/${T}_bench.err; exit 3; }
cat bench_out/${T}_bench.json
timeout -k 10 180 python -u tools/stamps.py --reps 50 > bench_out/${T}_stamps.txt 2>&1 || { tail -20 bench_out/${T}_stamps.txt; exit 4; }
bash tools_profile.sh ${T}_c2 > bench_out/${T}_prof_c2.log 2>&1 || { tail -20 bench_out/${T}_prof_c2.log; exit 5; }
bash tools_profile.sh ${T}_c3 --workload cfg3 > bench_out/${T}_prof_c3.log 2>&1 || { tail -20 bench_out/${T}_prof_c3.log; exit 6; }
bash tools_profile.sh ${T}_st --workload stream --no-pcie-pass > bench_out/${T}_prof_st.log 2>&1 || { tail -20 bench_out/${T}_prof_st.log; exit 7; }
timeout -k 10 300 python -u bench.py --full --workload cfg3 --no-cpu-baseline > bench_out/${T}_cfg3.json 2> bench_out/${T}_cfg3.err || { tail -20 bench_out/${T}_cfg3.err; exit 8; }
cat bench_out/${T}_cfg3.json
timeout -k 10 300 python -u bench.py --full --workload stream --no-cpu-baseline > bench_out/${T}_stream.json 2> bench_out/${T}_stream.err || { tail -20 bench_out/${T}_stream.err; exit 9; }
cat bench_out/${T}_stream.json
