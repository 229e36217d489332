# headline on 116^3 / 128x96x128 / 128^3 (with the sustained solves: --full), slab of rank 3 of 8, p = 1 both quadratures: bash tools/probes/mesh_ab.sh [out dir]
out=${1:-bench_out/mesh_ab}
mkdir -p $out
python3 bench.py --full --no-cpu-baseline --no-traffic-pass > $out/bench_116.json 2>$out/bench_116.err
python3 bench.py --full --cells 128 96 128 --no-cpu-baseline --no-traffic-pass > $out/bench_128x96x128.json 2>$out/bench_128.err
python3 bench.py --full --cells 128 128 128 --no-cpu-baseline --no-traffic-pass > $out/bench_128cubed.json 2>$out/bench_128c.err
python3 tools/halo_overhead_self.py --cell-block 4 4 2 --modes auto,none --iters 100 > $out/halo_116.txt 2>&1
python3 tools/halo_overhead_self.py --cell-block 4 4 2 --modes auto,none --iters 100 --cells 128 96 128 > $out/halo_128x96x128.txt 2>&1
python3 bench.py --degree 1 --cells 367 367 367 --steps 50 --no-cpu-baseline --no-traffic-pass --sustained-iters 0 > $out/p1_gauss.json 2>/dev/null
python3 bench.py --degree 1 --cells 367 367 367 --steps 50 --quadrature gll --no-cpu-baseline --no-traffic-pass --sustained-iters 0 > $out/p1_gll.json 2>/dev/null
python3 - "$out" <<'P'
import json, sys
out = sys.argv[1]
for f in ('bench_116','bench_128x96x128','bench_128cubed','p1_gauss','p1_gll'):
    try:
        d=json.loads(open(f'{out}/{f}.json').read().strip().splitlines()[-1])
        print(f, round(d['value']/1e9,3), round(d['ms_per_step'],4), d['roofline']['avg_launch_ms'], d.get('sustained',{}) and round(d['sustained']['value']/1e9,3), d['roofline_cg']['frac_of_hbm_peak'])
    except Exception as e: print(f,'failed',e)
P
tail -4 $out/halo_116.txt $out/halo_128x96x128.txt
timeout -k 10 900 python -m pytest tests/ -x -q -m gpu > $out/gputests.log 2>&1; tail -5 $out/gputests.log
