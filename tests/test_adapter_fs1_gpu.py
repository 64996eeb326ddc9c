"""The FastSLAM-1 step through the reference-side binding: HipPF::controlRunSampledAll, cycleFastSlam1All and
likelihoodUpdateAll of include/cslam_adapter.hpp run, in tests/adapter/adapter_fs1.cpp, a 17-step sampled control run, the
five cycles of tests/pf_control_ref.py from an empty map (heading known) and one more likelihood update, and must end bit
for bit where ParticleShard.control_run_sampled / fs1_cycle_drawn / likelihood_update end.  Built with g++ against the
Eigen-free stand-in and linked against libcslam_hip.so."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pf_control_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fmt(a):
    return " ".join("%.9g" % float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1, order="F"))


def _build(tmp_path):
    from conan_slam_amd import _capi

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "adapter_fs1")
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "adapter"), os.path.join(ROOT, "tests", "adapter", "adapter_fs1.cpp"),
           "-L" + libdir, "-lcslam_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _script(dtype):
    """[(mode, step, ctl_step, v, swa, phi, ZF, idf, ZN)]: a sampled run of 17 steps, the five cycles from where the
    noise-free run ends (control steps counted on), and a likelihood update on the last cycle's known features"""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    rng = np.random.default_rng(98)
    v0, s0 = f32(3.0 + rng.uniform(-0.2, 0.2, 17)), f32(rng.uniform(-0.05, 0.05, 17))
    pose, phi0 = CR.advance(np.zeros(3), v0, s0, 17, rng)
    none, noidf = np.zeros((2, 0), dtype), np.zeros(0, np.int32)
    lines = [(0, 0, 0, v0, s0, f32(phi0), none, noidf, none)]
    ctl = 17
    for c, (v, swa, phi, idf, ZF, ZN, pose) in enumerate(CR.loop_cycles(dtype, pose)):
        lines.append((1, 1 + c, ctl, v, swa, phi, ZF, idf, ZN))
        ctl += len(v)
    _, _, _, v, swa, phi, ZF, idf, _ = lines[-1]
    lines.append((2, 9, ctl, v, swa, phi, ZF, idf, none))
    return lines


def test_adapter_fs1_ends_where_the_python_path_ends(gpu_required, tmp_path):
    from conan_slam_amd.pf import ParticleShard
    from test_pf_edges_gpu import _bulk_read, _same_bits

    dtype, npart, cap, seed = np.float32, 17, 5, 6
    nmin = 12  # (inside [1, np]: whether a scan resamples is decided on the device, alike on both paths)
    Q, R = CR.LOOP_Q.astype(dtype), CR.LOOP_R.astype(dtype)
    wb, dt = float(np.float32(CR.LOOP_WB)), float(np.float32(CR.LOOP_DT))
    lines = _script(dtype)
    src = tmp_path / "fs1_input.txt"
    with open(src, "w") as out:
        out.write(f"{npart} {cap} {seed} {len(lines)} {nmin}\n")
        for mode, step, ctl, v, swa, phi, ZF, idf, ZN in lines:
            out.write(f"{mode} {step} {ctl} {len(v)} {_fmt(v)} {_fmt(swa)} {_fmt(phi)} 1 {wb:.9g} {dt:.9g} {_fmt(Q)} "
                      f"{ZF.shape[1]} {_fmt(ZF)} {' '.join(str(int(i)) for i in idf)} {ZN.shape[1]} {_fmt(ZN)} {_fmt(R)}\n")

    sh = ParticleShard(npart, cap, dtype=dtype)
    sh.seed_draws(seed)
    for mode, step, ctl, v, swa, phi, ZF, idf, ZN in lines:
        if mode == 0:
            sh.control_run_sampled(v, swa, Q, wb, dt, ctl, phi=phi, use_heading=True)
        elif mode == 1:
            sh.fs1_cycle_drawn(v, swa, Q, wb, dt, ctl, ZF, idf, ZN, R, step, nmin, True, phi=phi, use_heading=True)
        else:
            sh.likelihood_update(ZF, idf, R, True, True)
    want, nf, launches = _bulk_read(sh), sh.n_features, sh.control_launches()
    stats = sh.resample_stats()
    sh.close()
    assert launches == 2 + 5 and nf == 5 and stats[0] == 4, (launches, nf, stats)
    assert np.all(np.isfinite(want)) and len(set(want[:, 1].tolist())) > 1, "the particles did not spread"

    exe = _build(tmp_path)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert len(r.stdout.splitlines()) == 1, "the adapter printed errors: " + r.stdout[:2000]
    got = json.loads(r.stdout)
    assert got["nf"] == nf, (got["nf"], nf)
    rec = np.array(got["records"], dtype=np.float64).astype(dtype)
    assert rec.shape == want.shape and np.all(np.isfinite(rec))
    assert _same_bits(rec, want)
