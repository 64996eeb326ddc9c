"""The reference's unknown-association branch (test/main.cpp:193-196: dataAssociate, update, augment every observation
step) through std::shared_ptr<Slam> bound to HipEKF (include/cslam_adapter.hpp), three steps, with
HipEKF::setDeferredAssociation on and off: built with g++ against the Eigen-free stand-in, linked against libcslam_hip.so.
On a decisive scan (assoc_deferred_ref.split_scan: 30 associated, 5 new, 5 dropped observations) idf and the ZF columns of
every step are equal between the two, and the first step's are the reference's decisions."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from assoc_builders import GATES
from assoc_deferred_ref import SPLIT_NF, split_scan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_assoc_deferred")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_assoc_deferred.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_unknown_association_branch_with_the_switch_on_and_off(gpu_required, tmp_path):
    case = split_scan()
    g1, g2 = GATES[0]
    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    got = {}
    for deferred in (0, 1):
        src = tmp_path / f"run{deferred}.txt"
        with open(src, "w") as out:
            out.write(f"{SPLIT_NF} {STEPS} {case.m} {deferred} {g1} {g2}\n{_fmt(case.X)}\n{_fmt(case.P)}\n{_fmt(case.R)}\n")
            for t in range(STEPS):
                out.write(f"1 {0.001 * t:.9g} {_fmt(case.Z)}\n")     # (v = 1 m/s: the pose moves a centimetre per step)
        r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
        got[deferred] = json.loads(r.stdout)
        assert got[deferred]["deferred"] == deferred
    off, on = got[0], got[1]
    idf_r, kind_r, _ = case.decisions(GATES[0])
    assert on["idf"][0] == [int(j) for j in idf_r[kind_r == 1]]
    assert np.array_equal(np.array(on["zf"][0], np.float32).reshape(2, -1, order="F"), case.Z[:, kind_r == 1])
    for t in range(STEPS):
        assert len(on["idf"][t]) == 30
        assert on["idf"][t] == off["idf"][t], t
        assert np.array(on["zf"][t], np.float32).tobytes() == np.array(off["zf"][t], np.float32).tobytes(), t
    assert on["zn_cols"] == off["zn_cols"] == [0] * STEPS     # (EKF.cpp:307: the reference returns an empty ZN)
    assert on["n"] == off["n"] == case.n
