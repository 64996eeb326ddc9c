"""The device-side score through the reference-side binding: HipPF::scoreReset / scoreTruth / score / scores
(include/cslam_adapter.hpp) built with g++ against the Eigen-free stand-in, linked against libcslam_hip.so and run on a
short replay (predict, score, three times); compared with the Python path on the same inputs -- counts exact, sums
within the bounds of the restatement (tests/pf_score_ref.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from pf_builders import Q_CTRL, shard_from
from pf_score_ref import PfScoreRef, values_case
from score_ref import COUNTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WB, DT = np.float32(2.83), np.float32(0.025)


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_score")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_score.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("estimator", ["mean", "best"])
def test_score_a_short_replay_through_the_adapter(gpu_required, tmp_path, estimator):
    dtype, npart, nf = np.float32, 65, 1
    case = values_case(npart, nf, dtype, estimator)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731 -- the adapter's types are float
    truth = f32(case.truth).astype(np.float64)
    steps = [(f32(x).astype(np.float64), np.float32(3.0 + i), np.float32(0.02 * i)) for i, x in enumerate(case.xv_trues)]
    src = tmp_path / "replay.txt"
    with open(src, "w") as out:
        out.write(f"{npart} {nf} {0 if estimator == 'mean' else 1} {len(steps)}\n")
        for w, Xv, Pv, XF, PF in case.parts:
            out.write(f"{_fmt([w])} {_fmt(Xv)} {_fmt(Pv)} {_fmt(XF)} {_fmt(PF)}\n")
        out.write(_fmt(truth.T) + "\n")
        for x, v, swa in steps:
            out.write(f"{_fmt(x)} {_fmt([v])} {_fmt([swa])}\n")
    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
    got = json.loads(r.stdout)
    # the Python path on the same inputs
    sh = shard_from(case.parts, nf, dtype)
    sh.score_reset(estimator, len(steps))
    sh.score_set_truth(truth)
    ref = PfScoreRef(dtype, estimator, len(steps))
    Q = np.asfortranarray(Q_CTRL.astype(dtype))
    for x, v, swa in steps:
        sh.predict(v, swa, Q, WB, DT)
        ref.add(sh.estimate() if estimator == "mean" else sh.best_particle("max"), truth, x)
        sh.score(x)
    py = sh.scores()
    ref.check(py, "python path")
    totals = np.array(got["totals"], dtype=np.float64)
    assert got["calls"] == py.calls == len(steps)
    assert np.array_equal(totals[list(COUNTS)], py.totals[list(COUNTS)]), (totals, py.totals)
    assert np.all(np.abs(totals - py.totals) <= ref.acc.B[0]), (totals, py.totals, ref.acc.B[0])
    series = np.array(got["series"], dtype=np.float32).reshape(len(steps), 4)
    track = np.array(got["track"], dtype=np.float64).reshape(len(steps), 5)
    assert series.tobytes() == py.series.tobytes() and track.tobytes() == py.track.tobytes()
    sh.close()
