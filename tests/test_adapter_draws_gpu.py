"""The device-side draws through the reference-side binding: a HipPF seeded with seedDraws (include/cslam_adapter.hpp) runs
ten steps -- predictAll, sampleProposalAll(Z, idf, R) without normals, featureUpdateAll, resampleParticles without strata --
next to an unseeded HipPF that is handed the same draws through the `normals` overload and setStrata; the two particle
sets must be bit-equal and finite after every step, and every forced resample must happen (between steps both sets go back
with the covariances they started with, see tests/adapter/adapter_draws.cpp).  Built with g++ against the Eigen-free
stand-in and linked against libcslam_hip.so."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from pf_builders import PREDICT, Q_CTRL, R_OBS, TRUE_POSE, advance_pose, tight_obs, tight_particles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_draws")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_draws.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_seeded_adapter_equals_the_one_handed_the_same_draws(gpu_required, tmp_path):
    dtype, npart, nf, m, steps = np.float32, 70, 12, 8, 10
    parts, base = tight_particles(npart, nf, dtype, seed=31)
    rng = np.random.default_rng(32)
    src = tmp_path / "draws_input.txt"
    with open(src, "w") as out:
        out.write(f"{npart} {nf} 424242 {steps}\n")
        for w, Xv, Pv, XF, PF in parts:
            out.write(f"{_fmt([w])} {_fmt(Xv)} {_fmt(Pv)} {_fmt(XF)} {_fmt(PF)}\n")
        pose = TRUE_POSE
        for t in range(steps):
            pose = advance_pose(pose, *PREDICT)
            idf = (rng.permutation(nf)[:m] + 1).astype(np.int32)
            Z = tight_obs(base, idf, dtype, seed=200 + t, pose=pose)
            nmin = npart + 1 if t % 2 == 0 else 0   # every other step asks for a resample
            out.write(f"{_fmt([PREDICT[0], PREDICT[1], PREDICT[2], PREDICT[3]])} {_fmt(Q_CTRL.astype(dtype))} {m} {_fmt(Z)} "
                      f"{' '.join(str(int(i)) for i in idf)} {_fmt(R_OBS.astype(dtype))} {nmin}\n")
    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
    got = json.loads(r.stdout)
    # after every one of the ten steps the two sets are bit-equal and the seeded one is finite; the five even steps
    # resample (four of them at a step other than 0: each consumes its own step's strata); 0.83 m of travel per step
    assert (got["steps"], got["equal_steps"], got["finite_steps"]) == (steps, steps, steps), got
    assert (got["resamples"], got["late_resamples"]) == (5, 4), got
    assert 5.0 < got["moved"] < 12.0, got
