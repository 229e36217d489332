# GLL(p+1) headline (with the reporting legs) and the config-4 sweep in both quadratures: bash tools/probes/gll_lines.sh [out dir]
set -e
out=${1:-bench_out/gll_lines}
mkdir -p $out
python3 bench.py --full --quadrature gll --no-cpu-baseline > $out/bench_gll_116.json 2> $out/bench_gll_116.err || tail -5 $out/bench_gll_116.err
python3 bench.py --full --config 4 --no-cpu-baseline --no-traffic-pass --sustained-iters 0 > $out/bench_config4_both_quadratures.json 2> $out/bench_config4.err || tail -5 $out/bench_config4.err
python3 - "$out" <<'P'
import json, sys
out = sys.argv[1]
d=json.loads(open(f'{out}/bench_gll_116.json').read().strip().splitlines()[-1])
print('GLL 116^3', d['value']/1e9, d['ms_per_step'], d['roofline']['kernel'], d['roofline']['avg_launch_ms'], d['roofline']['frac'])
d=json.loads(open(f'{out}/bench_config4_both_quadratures.json').read().strip().splitlines()[-1])
for e in d['sweep']:
    print(e['degree'], e['quadrature'], round(e['value']/1e9,2), round(e['frac_of_hbm_peak'],3), e['kernel'], '| gll', round(e['gll']['value']/1e9,2), round(e['gll']['frac_of_hbm_peak'],3), e['gll']['kernel'])
P
