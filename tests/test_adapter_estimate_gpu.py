"""The read path through the reference-side binding: HipPF::extractStates / extractFeatures / extractMap
(include/cslam_adapter.hpp) built with g++ against the Eigen-free stand-in, linked against libcslam_hip.so and run on
a small particle set; compared with the numpy helper (tests/pf_estimate_ref.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from pf_builders import random_particles
from pf_estimate_ref import all_features_ref, best_ref, estimate_ref, mean_errors, stack

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_estimate")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_estimate.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_extract_states_features_and_map_through_the_adapter(gpu_required, tmp_path):
    dtype, npart, nf = np.float32, 9, 3
    parts = random_particles(npart, nf, dtype, seed=909)
    src = tmp_path / "particles.txt"
    with open(src, "w") as out:
        out.write(f"{npart} {nf}\n")
        for w, Xv, Pv, XF, PF in parts:
            out.write(f"{_fmt([w])} {_fmt(Xv)} {_fmt(Pv)} {_fmt(XF)} {_fmt(PF)}\n")
    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
    got = json.loads(r.stdout)
    w, X, P, XF, PF = stack(parts)
    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731 -- %.9g round-trips a float exactly
    assert best_ref(w, "max") != best_ref(w, "min")
    assert f32(got["states_max"]).tobytes() == f32(X[best_ref(w, "max")]).tobytes()
    assert f32(got["states_min"]).tobytes() == f32(X[best_ref(w, "min")]).tobytes()
    feat = f32(got["features"]).reshape(2, npart * nf, order="F")
    assert feat.tobytes() == f32(all_features_ref(XF)).tobytes()
    err, bound = mean_errors(f32(got["map"]).reshape(2, nf, order="F"), estimate_ref(w, X, P, XF, PF).XF, dtype)
    assert np.all(err <= bound), (float(err.max()), float(bound.min()))
