"""bench.py's one-line JSON contract, on a small workload (child process, one GPU) and through the
torch.distributed.run launcher with one rank."""
import json
import os
import subprocess
import sys

import pytest

import bp5_pkg

pytestmark = pytest.mark.gpu
BENCH = os.path.join(bp5_pkg.ROOT, "bench.py")
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline", "cpu_baseline", "sustained"}


def _check(line, steps, warmup):
    d = json.loads(line)
    assert KEYS <= set(d)
    assert d["unit"] == "DoF/s" and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    assert d["higher_is_better"] is True and d["scaling"] == "strong" and d["vs_baseline"] is None and d["dtype"] == "f64"
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["config"]["dofs_per_gpu"] * steps / (d["ms_per_step"] * 1e-3 * steps)) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["launches"] == steps
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["achieved"] > 0 and r["avg_launch_ms"] > 0
    assert r["operator_ms"] >= r["avg_launch_ms"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "DoF/s" and c["value"] > 0 and c["cores"] >= 1 and "sample" in c
    assert f"{d['config']['dofs_per_gpu']} DoFs" in c["sample"]          # the CPU leg runs on the bench's own mesh
    s = d["sustained"]
    assert s["unit"] == "DoF/s" and s["value"] > 0 and s["iterations"] >= 1 and s["repetitions"] >= 1
    # round 3: the kernel name comes from the solve itself, the whole-iteration figure says what it is based on, the moved-bytes fractions
    # stand beside the contract figures, the host set-up time is reported
    assert r["kernel"].startswith("apply_") and 0 < r["frac_moved"] <= r["frac"] + 1e-12 and r["bytes_moved_per_dof"] <= r["bytes_per_dof"]
    assert "contract formula" in d["roofline_cg"]["basis"] and d["roofline_cg"]["frac_moved_of_hbm_peak"] <= d["roofline_cg"]["frac_of_hbm_peak"]
    assert d["host_setup_s"] > 0 and d["config"]["exchange_schedule"] == "none (one rank)"
    assert d["post_processing"]["completed"] is True and d["post_processing"]["stage_reached"] is None
    sc = d["solve_check"]
    assert sc["iterations"] == steps and sc["residual_after_timed_solve"] > 0 and sc["initial_residual"] > 0
    return d


def test_bench_json_line_small_workload():
    r = subprocess.run([sys.executable, BENCH, "--full", "--cells", "12", "12", "12", "--steps", "7", "--warmup", "2", "--sustained-iters", "20", "--sustained-reps", "2",
                        "--cpu-budget", "2"], capture_output=True, text=True,
                       timeout=900, cwd=bp5_pkg.ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                              # ONE JSON line
    d = _check(lines[0], 7, 2)
    # roofline.traffic is measured by the invocation itself: two rocprofv3 --pmc child passes (FETCH_SIZE, WRITE_SIZE) of this workload
    # (not when this test itself runs under a profiler: bench.py then starts no nested one and reports null for an unprofiled workload)
    import shutil
    profiled = "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith(("ROCP_", "ROCPROF")) for k in os.environ)
    r = d["roofline"]
    if shutil.which("rocprofv3") and not profiled:
        assert isinstance(r["traffic"], int) and r["traffic"] > 0 and "child passes of this bench invocation" in r["traffic_source"]
    else:
        assert r["traffic"] is None or r["traffic"] > 0


def test_bench_quotes_the_committed_pmc_passes_when_the_live_ones_are_switched_off():
    r = subprocess.run([sys.executable, BENCH, "--full", "--cells", "12", "12", "12", "--steps", "3", "--warmup", "1", "--sustained-iters", "0", "--no-cpu-baseline",
                        "--no-traffic-pass"], capture_output=True, text=True, timeout=900, cwd=bp5_pkg.ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["roofline"]["traffic"] is None and d["roofline"]["traffic_source"] is None      # (no committed passes for this small workload)


def test_bench_baseline_config_aliases():
    """`--config N`: every BASELINE.json configuration as one flag (1: p = 2, 8^3 cells, 10 iterations -- the plumbing case, run here; 2: 54^3; 4: the degree
    sweep; 5: p = 6 deformed -- checked through --dry-run on the host: sizes only)."""
    r = subprocess.run([sys.executable, BENCH, "--config", "1", "--no-cpu-baseline", "--no-traffic-pass", "--sustained-iters", "0"], capture_output=True,
                       text=True, timeout=600, cwd=bp5_pkg.ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["steps"] == 10 and d["config"]["baseline_config"] == 1 and "p=2" in d["config"]["workload"] and "8x8x8 hex cells, 4913 DoFs" in d["config"]["workload"]
    for cfg, want in ((2, (54, 54, 54, 10218313)), (5, (61, 61, 61, 49430863))):
        r = subprocess.run([sys.executable, BENCH, "--config", str(cfg), "--dry-run"], capture_output=True, text=True, timeout=600, cwd=bp5_pkg.ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert tuple(d["cells"]) == want[:3] and d["n_global_dofs"] == want[3]


def test_bench_under_the_distributed_launcher_one_rank():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29731", BENCH, "--gpus", "1", "--steps", "4", "--warmup", "1", "--cells", "8", "8", "8",
                        "--no-cpu-baseline", "--no-traffic-pass"], capture_output=True, text=True, timeout=900, cwd=bp5_pkg.ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 4 and "cpu_baseline" not in d


def test_bench_watchdog_prints_the_line_when_the_reporting_legs_overrun():
    """the legs behind the timed region (sustained solves, exchange A/B, copy stream, traffic passes, CPU baseline) run under a watchdog: when they take longer than
    --post-budget the line is printed with what is there and the process exits with code 4 -- a hang in a diagnostic leg must not cost a run its measurement, and
    must not pass for a clean run either"""
    r = subprocess.run([sys.executable, BENCH, "--full", "--cells", "24", "24", "24", "--steps", "5", "--warmup", "1", "--sustained-iters", "20000", "--sustained-reps", "100",
                        "--post-budget", "2"], capture_output=True, text=True, timeout=900, cwd=bp5_pkg.ROOT)
    assert r.returncode == 4, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["value"] > 0 and d["steps"] == 5 and d["roofline"]["achieved"] > 0 and d["roofline"]["frac"] > 0
    assert d["post_processing"]["completed"] is False and d["post_processing"]["stage_reached"] == "sustained solves"
    assert "cpu_baseline" not in d and "sustained" not in d and d["roofline_cg"]["stream_copy_GBs"] is None
    assert "post-processing exceeded" in r.stderr


def _run_dump(out_dir, cells, steps, *extra):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--cells", *[str(c) for c in cells], "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=600, cwd=bp5_pkg.ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    import numpy as np
    assert sorted(os.listdir(out_dir)) == ["residual_norms.npy", "solution.npy", "solution_dofs.npy"]
    arrs = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    assert all(a.dtype == np.float64 for a in arrs.values()) and sum(a.nbytes for a in arrs.values()) <= 64 << 20
    return json.loads(lines[0]), arrs


def _same_up_to_rounding(a, b):
    import numpy as np
    assert np.array_equal(a["solution_dofs"], b["solution_dofs"])
    for k in ("solution", "residual_norms"):
        assert np.linalg.norm(a[k] - b[k]) <= 1e-12 * np.linalg.norm(a[k]), k


def test_bench_plain_run_is_lean_and_dumps_what_the_timed_solve_computed(tmp_path):
    """A plain run (no --full) times the steps and prints the line, no reporting leg after the timed region; --dump-outputs writes the
    solution of the timed solve (x0 = 0, exactly --steps iterations) in the lexicographic DoF numbering: the same DoFs and the same values up to
    rounding from run to run (the solver's reductions are not bitwise reproducible), the oracle's merged CG on the same mesh, and a fixed, seeded
    sample of the DoFs once the problem is larger than that sample."""
    import numpy as np
    import bp5_oracle as O
    runs = [_run_dump(tmp_path / f"run{k}", (8, 8, 8), 6) for k in range(2)]
    d, a = runs[0]
    assert d["steps"] == 6 and d["ms_per_step"] > 0 and d["post_processing"]["completed"] is True
    assert not {"cpu_baseline", "sustained", "mesh_116_cubed", "exchange_ab", "sweep"} & set(d)
    assert d["roofline_cg"]["stream_copy_GBs"] is None and d["roofline"]["operator_kernel_unfused"] is None and d["roofline"]["traffic"] is None
    _same_up_to_rounding(a, runs[1][1])
    n = 33 ** 3
    assert np.array_equal(a["solution_dofs"], np.arange(n, dtype=np.float64))
    sc = d["solve_check"]
    assert a["residual_norms"].tolist() == [sc["initial_residual"], sc["residual_after_timed_solve"]]
    pr = O.Problem(4, (8, 8, 8), O.QUAD_GAUSS, h=1.0 / 8, kappa=O.kappa_step64)
    xr, k, _ = O.cg_merged(pr.vmult, pr.rhs(), 6)
    assert k == 6 and np.linalg.norm(a["solution"] - xr) / np.linalg.norm(xr) < 1e-11
    # larger than the sample (137^3 DoFs): the same seeded sample every run, sorted, unique, inside the problem
    big = [_run_dump(tmp_path / f"big{k}", (34, 34, 34), 3)[1] for k in range(2)]
    ids = big[0]["solution_dofs"]
    assert len(ids) == 2 ** 21 and np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < 137 ** 3
    _same_up_to_rounding(*big)
    assert np.all(np.isfinite(big[0]["solution"]))
