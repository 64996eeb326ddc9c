"""The control run and the whole-cycle calls through the reference-side binding: HipPF::controlRunAll, cycleAll and
cycleUnknownAll of include/cslam_adapter.hpp run, in tests/adapter/adapter_cycle.cpp, a 17-step control run, the five
heading-known cycles of tests/pf_control_ref.py from an empty map and one unknown-correspondence cycle, and must end bit
for bit where ParticleShard.control_run / cycle_drawn / assoc_cycle_drawn end.  Built with g++ against the Eigen-free
stand-in and linked against libcslam_hip.so."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pf_control_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE1, GATE2, FRAC, MISS = 4.0, 25.0, 0.5, float(np.float32(1e-3))
FAR = np.array([[25.0], [-12.0]])  # a sixth landmark nobody has mapped: the unknown-correspondence cycle adds it


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_cycle")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_cycle.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _script(dtype):
    """[(mode, step, v, swa, phi, ZF, idf, ZN)]: a run of 17 steps, the five cycles from where it ends, and one cycle with
    unknown correspondences that sees every landmark and the far one"""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rng = np.random.default_rng(99)
    v0, s0 = f32(3.0 + rng.uniform(-0.2, 0.2, 17)), f32(rng.uniform(-0.05, 0.05, 17))
    pose, phi0 = CR.advance(np.zeros(3), v0, s0, 17, rng)
    none, noidf = np.zeros((2, 0), dtype), np.zeros(0, np.int32)
    lines = [(0, 0, v0, s0, f32(phi0), none, noidf, none)]
    for c, (v, swa, phi, idf, ZF, ZN, pose) in enumerate(CR.loop_cycles(dtype, pose)):
        lines.append((1, 1 + c, v, swa, phi, ZF, idf, ZN))
    v1, s1 = f32(3.0 + rng.uniform(-0.2, 0.2, 6)), f32(rng.uniform(-0.1, 0.1, 6))
    pose, phi1 = CR.advance(pose, v1, s1, 6, rng)
    lms = np.concatenate([CR.LANDMARKS, FAR], axis=1)
    Z = CR.observe(pose, range(6), dtype, landmarks=lms)
    lines.append((2, 7, v1, s1, f32(phi1), Z, np.zeros(6, np.int32), none))  # (the driver reads an idf per column)
    return lines


def test_adapter_cycles_end_where_the_python_path_ends(gpu_required, tmp_path):
    from conan_slam_amd.pf import ParticleShard
    from test_pf_edges_gpu import _bulk_read, _same_bits

    dtype, npart, cap, seed = np.float32, 17, 6, 5
    Q, R = CR.LOOP_Q.astype(dtype), CR.LOOP_R.astype(dtype)
    wb, dt = float(np.float32(CR.LOOP_WB)), float(np.float32(CR.LOOP_DT))
    lines = _script(dtype)
    src = tmp_path / "cycle_input.txt"
    with open(src, "w") as out:
        out.write(f"{npart} {cap} {seed} {len(lines)} {GATE1:.9g} {GATE2:.9g} {FRAC:.9g} {MISS:.9g} {npart + 1}\n")
        for mode, step, v, swa, phi, ZF, idf, ZN in lines:
            out.write(f"{mode} {step} {len(v)} {_fmt(v)} {_fmt(swa)} {_fmt(phi)} 1 {wb:.9g} {dt:.9g} {_fmt(Q)} "
                      f"{ZF.shape[1]} {_fmt(ZF)} {' '.join(str(int(i)) for i in idf)} {ZN.shape[1]} {_fmt(ZN)} {_fmt(R)}\n")

    sh = ParticleShard(npart, cap, dtype=dtype)
    sh.seed_draws(seed)
    added = []
    for mode, step, v, swa, phi, ZF, idf, ZN in lines:
        if mode == 0:
            sh.control_run(v, swa, Q, wb, dt, phi=phi, use_heading=True)
        elif mode == 1:
            sh.cycle_drawn(v, swa, Q, wb, dt, ZF, idf, ZN, R, step, npart + 1, True, phi=phi, use_heading=True)
        else:
            added.append(sh.assoc_cycle_drawn(v, swa, Q, wb, dt, ZF, R, GATE1, GATE2, step, npart + 1, True, phi=phi,
                                              use_heading=True, new_fraction=FRAC, miss_likelihood=MISS))
    want, nf, launches = _bulk_read(sh), sh.n_features, sh.control_launches()
    sh.close()
    assert launches == 2 + 5 + 1 and nf == 5 + added[0] and added[0] >= 1, (launches, nf, added)

    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
    got = json.loads(r.stdout)
    assert got["nf"] == nf and got["added"] == added, (got["nf"], got["added"], added)
    rec = np.array(got["records"], dtype=np.float64).astype(dtype)
    assert np.all(np.isfinite(rec)) and rec.shape == want.shape
    assert _same_bits(rec, want)
