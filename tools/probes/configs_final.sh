# the other BASELINE configurations with the reporting legs (--full: sustained solves, config-4 sweep, CPU baseline): bash tools/probes/configs_final.sh [out dir]
out=${1:-bench_out/configs_final}
mkdir -p $out
python3 bench.py --full --config 2 --no-cpu-baseline --no-traffic-pass > $out/bench_config2.json 2> $out/c2.err
python3 bench.py --full --config 5 --no-cpu-baseline --no-traffic-pass > $out/bench_config5.json 2> $out/c5.err
python3 bench.py --full --config 4 --no-cpu-baseline --no-traffic-pass --sustained-iters 0 > $out/bench_config4.json 2> $out/c4.err
python3 bench.py --full --config 1 --no-traffic-pass > $out/bench_config1.json 2> $out/c1.err
python3 bench.py --full --operator helmholtz --degree 3 --cells 122 122 122 --no-cpu-baseline --no-traffic-pass > $out/bench_helmholtz_p3.json 2> $out/h.err
python3 - "$out" <<'P'
import json, sys
out = sys.argv[1]
for f in ('bench_config2','bench_config5','bench_config1','bench_helmholtz_p3'):
    try:
        d=json.loads(open(f'{out}/{f}.json').read().strip().splitlines()[-1])
        print(f, round(d['value']/1e9,3),'GDoF/s', round(d['ms_per_step'],4),'ms frac', round(d['roofline_cg']['frac_of_hbm_peak'],3), 'sustained', d.get('sustained') and round(d['sustained']['value']/1e9,2), d['roofline']['kernel'])
    except Exception as e: print(f,'failed',e)
d=json.loads(open(f'{out}/bench_config4.json').read().strip().splitlines()[-1])
for e in d['sweep']:
    print(e['degree'], e['quadrature'], round(e['value']/1e9,2), round(e['frac_of_hbm_peak'],3), e['kernel'], '| gll', round(e['gll']['value']/1e9,2), round(e['gll']['frac_of_hbm_peak'],3))
P
