# A/B/C of library builds on configs[2], alternated: tools/ab3.sh A.so B.so C.so ...
set -o pipefail
R=$(pwd); mkdir -p bench_out
for rep in 1 2 3; do
  for L in "$@"; do
    FAASBAL_LIB=$R/$L timeout -k 10 150 python -u bench.py --full --no-cpu-baseline --no-host-observed --steps 400 $AB_ARGS > bench_out/ab.json 2> bench_out/ab.err || { tail -5 bench_out/ab.err; exit 3; }
    python -c "import json,sys; d=json.load(open('bench_out/ab.json')); print('$(basename $L)', 'us/tick %.2f' % (d['ms_per_step']*1e3), {k: round(v*1e3,2) for k,v in d['tick']['kernels_avg_ms'].items()}, 'dom %s frac %.3f' % (d['roofline']['kernel'], d['roofline']['frac']))"
  done
done
