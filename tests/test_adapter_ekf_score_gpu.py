"""The single handle's device-side score through the reference-side binding: HipEKF::scoreReset / scoreTruth / score /
scores / pose (include/cslam_adapter.hpp), built with g++ against the Eigen-free stand-in, linked against libcslam_hip.so
and run on a short scored loop (predict, batch update, score; three times).  The Python path makes the same calls -- the
binding refreshes the caller's X after every hot-path call, so the Python loop reads get_x() at the same points -- on the
same device code: counts exact, sums, series, track and the pose read bitwise."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from ekf_score_ref import SingleRef
from helpers import make_obs, make_scenario
from score_ref import COUNTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = np.diag([0.18, 6e-4]).astype(np.float32)
R = np.diag([0.08, 0.0024]).astype(np.float32)


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_ekf_score")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_ekf_score.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_score_a_short_loop_through_the_adapter(gpu_required, tmp_path):
    from conan_slam_amd import EKF

    N, m, dtype = 20, 6, np.float32
    X, P = make_scenario(N, np.dtype(dtype), seed=77, corr=0.1)
    rng = np.random.default_rng(77)
    truth = (X[3:].reshape(N, 2) + rng.normal(size=(N, 2))).astype(np.float32)
    steps = []
    for t in range(3):
        idf = (rng.permutation(N)[:m] + 1).astype(np.int32)
        xt = np.array([1.0 + 0.1 * t, -2.0, 0.3 + 0.01 * t], np.float32)
        steps.append((xt, np.float32(83.33), np.float32(0.01 * t), idf, make_obs(X, idf, dtype, seed=t)))
    src = tmp_path / "run.txt"
    with open(src, "w") as out:
        out.write(f"{N} {len(steps)} {m}\n{_fmt(X)}\n{_fmt(P)}\n{_fmt(truth.T)}\n")
        for xt, v, swa, idf, Z in steps:
            out.write(f"{_fmt(xt)} {_fmt([v])} {_fmt([swa])} {' '.join(str(int(i)) for i in idf)} {_fmt(Z)}\n")
    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
    got = json.loads(r.stdout)
    # the Python path: the same calls on the same inputs
    e = EKF(N, dtype=dtype)
    e.set_state(X, P)
    e.score_reset(len(steps))
    e.score_set_truth(truth)
    ref = SingleRef(len(steps))
    for xt, v, swa, idf, Z in steps:
        e.predict(v, swa, Q, 73.0, 0.01)
        e.get_x()
        e.update(Z, R, idf, True)
        e.get_x()
        e.score(xt)
        ref.add(e, truth, xt)
    py = e.scores()
    ref.check(py, "python path")
    x, pvv = e.pose()
    e.close()
    totals = np.array(got["totals"], dtype=np.float64)
    assert got["calls"] == py[3] == len(steps)
    assert np.array_equal(totals[list(COUNTS)], py[0][list(COUNTS)]), (totals, py[0])
    assert totals.tobytes() == py[0].tobytes(), (totals, py[0])
    series = np.array(got["series"], dtype=np.float32).reshape(len(steps), 4)
    track = np.array(got["track"], dtype=np.float64).reshape(len(steps), 5)
    assert series.tobytes() == py[1].tobytes() and track.tobytes() == py[2].tobytes()
    assert np.array(got["x"], np.float32).tobytes() == x.tobytes()
    assert np.array(got["pvv"], np.float32).reshape(3, 3).T.tobytes() == np.ascontiguousarray(pvv).tobytes()
