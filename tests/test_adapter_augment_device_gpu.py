"""HipEKF::augmentAssociated / augmentDevice (include/cslam_adapter.hpp): one step of the reference's unknown-association
branch (test/main.cpp:193-196) through std::shared_ptr<Slam> bound to HipEKF with the deferred association on -- predict,
dataAssociate, update -- and then the augment from the ZN the association left on the device, against the same step
with the host ZN through the virtual HipEKF::augment: X and P bit for bit.  Built with g++ against the Eigen-free stand-in,
linked against libcslam_hip.so, on the decisive scan of assoc_deferred_ref.split_scan (30 associated, 5 new, 5 dropped)."""
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


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_augment_device")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_augment_device.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_augment_from_the_device_list_equals_the_host_path(gpu_required, tmp_path):
    case = split_scan()
    g1, g2 = GATES[0]
    _, kind_r, _ = case.decisions(GATES[0])
    ZN = np.asfortranarray(case.Z[:, kind_r == 2])
    q = ZN.shape[1]
    assert q == 5
    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    got = {}
    for device in (0, 1):
        src = tmp_path / f"run{device}.txt"
        with open(src, "w") as out:
            out.write(f"{SPLIT_NF} {case.m} {device} {g1} {g2} {q}\n{_fmt(case.X)}\n{_fmt(case.P)}\n{_fmt(case.R)}\n")
            out.write(f"1 0.001 {_fmt(case.Z)}\n{_fmt(ZN)}\n")
        r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
        got[device] = json.loads(r.stdout)
        assert got[device]["device"] == device and got[device]["new"] == q
    host, dev = got[0], got[1]
    n = 3 + 2 * (SPLIT_NF + q)
    assert host["n"] == dev["n"] == n and len(dev["x"]) == n and len(dev["p"]) == n * n
    assert np.array(dev["x"], np.float32).tobytes() == np.array(host["x"], np.float32).tobytes()
    assert np.array(dev["p"], np.float32).tobytes() == np.array(host["p"], np.float32).tobytes()
    P = np.array(dev["p"], np.float64).reshape(n, n, order="F")
    assert np.all(np.isfinite(P)) and np.all(np.diag(P)[3 + 2 * SPLIT_NF:] > 0)   # (the new blocks are there)
