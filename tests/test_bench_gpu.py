"""bench.py as the driver runs it: a child process, one JSON line with the contract's fields (the workloads at reduced
sizes so that the test stays short; the numbers themselves are not asserted).  A plain run carries the headline figure
only; what is measured beside it (sub-records, CPU baselines, the Monte-Carlo single-instance run) comes with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ["cpu_baseline", "gpu_over_cpu_single_core", "per_call", "per_call_steps_per_sec", "dropin", "immediate_mode",
             "reference_loop", "reference_loop_ref_exact", "ref_exact_healthy", "single_instance", "concurrency_gain"]
CONTRACT = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline"]


def _run(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.strip().split("\n") if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _dumped(d, finite=True):
    arrays = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and (np.all(np.isfinite(a)) or not finite), name
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    return arrays


def test_bench_driver_shape_prints_the_contract_line(gpu_required):
    d = _run(["--gpus", "1", "--steps", "20", "--warmup", "5", "--landmarks", "1500", "--cpu-baseline-seconds", "2",
              "--preheat-ms", "50", "--full"])
    for k in CONTRACT + ["cpu_baseline", "per_call", "dropin", "immediate_mode", "reference_loop", "ref_exact_healthy"]:
        assert k in d, k
    assert d["roofline"]["bracketed_pass"]["launches"] > 0
    assert d["metric"] == "ekf_update_steps_per_sec" and d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5
    assert d["value"] > 0 and d["higher_is_better"] is True and d["vs_baseline"] is None and d["dtype"] == "f32"
    assert "workload" in d["config"] and d["factor_flags"] == 0
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] <= 1.0 and r["unit"] in ("GB/s", "TFLOP/s")
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1


def test_bench_plain_run_measures_the_headline_only(gpu_required):
    """Without --full the line has the contract's fields and none of the records that take a run of their own."""
    d = _run(["--gpus", "1", "--steps", "20", "--warmup", "5", "--landmarks", "1500", "--preheat-ms", "5"])
    for k in CONTRACT + ["trace_P_end", "cold_steps_per_sec"]:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert "bracketed_pass" not in d["roofline"]
    assert d["metric"] == "ekf_update_steps_per_sec" and d["steps"] == 20 and d["warmup"] == 5 and d["preheat_steps"] > 0
    assert d["value"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f32" and d["factor_flags"] == 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) <= 1e-6 * 1e3


@pytest.mark.parametrize("args,steps", [
    (["--workload", "mc", "--instances", "3", "--landmarks", "400", "--steps", "12", "--warmup", "4"], 12),
    (["--workload", "mc", "--mc-engine", "handles", "--instances", "3", "--landmarks", "400", "--steps", "12", "--warmup", "4"],
     12),
    (["--workload", "pf", "--particles", "64", "--features", "100", "--steps", "6", "--warmup", "2"], 6),
], ids=["mc-batch", "mc-handles", "pf"])
def test_bench_plain_run_of_the_other_workloads(gpu_required, args, steps):
    """The same for --workload mc (both engines) and pf: no --no-cpu-baseline here, so a CPU baseline or a single-instance
    run that came back into the plain run would show."""
    d = _run(args)
    for k in CONTRACT:
        assert k in d, k
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["steps"] == steps and d["value"] > 0 and d["ms_per_step"] > 0


def test_bench_dump_outputs_repeat_from_run_to_run(gpu_required, tmp_path):
    """--dump-outputs at the driver's shape (a short warm-up, so the GPU is first preheated) writes the filter state after
    the last timed step -- its covariance trace is the line's trace_P_end -- and a second run with the same arguments
    writes the same arrays."""
    args = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--landmarks", "1500", "--no-cpu-baseline", "--no-extras",
            "--preheat-ms", "50"]
    runs = []
    for r in range(2):
        d = _run(args + ["--dump-outputs", str(tmp_path / f"run{r}")])
        assert d["steps"] == 20 and d["ms_per_step"] > 0 and d["factor_flags"] == 0 and d["preheat_steps"] > 0
        a = _dumped(tmp_path / f"run{r}")
        n = 3 + 2 * 1500
        assert sorted(a) == ["P_diag", "P_pose", "P_sample", "X"]
        assert a["X"].shape == (n,) and a["P_diag"].shape == (n,) and a["P_pose"].shape == (n, 3)
        assert a["X"].dtype == np.float32 and 0 < a["P_sample"].size < n * n
        assert np.array_equal(np.diagonal(a["P_pose"][:3]), a["P_diag"][:3])
        tr = float(a["P_diag"].astype(np.float64).sum())
        assert abs(tr - d["trace_P_end"]) <= 1e-5 * abs(d["trace_P_end"]), (tr, d["trace_P_end"])
        runs.append(a)
    for name in runs[0]:
        b = runs[0][name]
        np.testing.assert_allclose(runs[1][name], b, rtol=1e-5, atol=1e-6 * float(np.abs(b).max()), err_msg=name)


def test_bench_batched_monte_carlo_mode(gpu_required, tmp_path):
    d = _run(["--workload", "mc", "--instances", "3", "--landmarks", "400", "--steps", "12", "--warmup", "4", "--no-cpu-baseline",
              "--full", "--dump-outputs", str(tmp_path)])
    for k in CONTRACT:
        assert k in d, k
    assert "cpu_baseline" not in d and d["concurrency_gain"] > 0
    assert d["config"]["instances_per_gpu"] == 3 and "cslam_ekf_batch" in d["config"]["engine"]
    assert d["factor_flags"] == [0, 0, 0] and d["value"] > 0 and d["single_instance"]["value"] > 0
    a = _dumped(tmp_path)
    n = 3 + 2 * 400
    assert a["X"].shape == (3, n) and a["P_diag"].shape == (3, n) and a["P_pose"].shape == (3, n, 3)
    assert a["P_sample"].shape[0] == 3 and not np.array_equal(a["X"][0], a["X"][1])  # (each instance has its own seed)


def test_bench_particle_filter_dump_outputs(gpu_required, tmp_path):
    """The particle store after the last timed step.  (The synthetic PF inputs drive some feature covariances to NaN
    within a few steps -- the CPU oracle's restatement of the reference does the same -- so only the weights, which the
    line reports on, are checked for finiteness.)"""
    d = _run(["--workload", "pf", "--particles", "64", "--features", "100", "--steps", "6", "--warmup", "2", "--no-cpu-baseline",
              "--dump-outputs", str(tmp_path)])
    for k in CONTRACT:
        assert k in d, k
    assert d["steps"] == 6 and d["weights_finite"] is True
    a = _dumped(tmp_path, finite=False)
    assert np.all(np.isfinite(a["weights"]))
    assert sorted(a) == ["feature_cov", "features", "pose", "pose_cov", "weights"]
    assert a["weights"].shape == (64,) and a["pose"].shape == (64, 3) and a["pose_cov"].shape == (64, 3, 3)
    assert a["features"].shape == (64, 2, 100) and a["feature_cov"].shape == (64, 4, 100)
