"""CPU side of the scan that observes only new features (test/main.cpp:314-328): the entry points are declared, cited,
listed and mirrored; the host check of their arguments; the reference helper tests/pf_new_feature_ref.py on the oracle
alone; and the statistical case of the GPU file run on synth.pf_draw_normals, so that its seed is known to pass with
margin before it reaches a GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pf_new_feature_ref as ref
from conan_slam_amd import _capi, synth
from pf_builders import DTYPES, PREDICT, Q_CTRL, R_OBS, TOL, random_particles
from pyoracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = ("cslam_pf_sample_pose", "cslam_pf_sample_pose_drawn", "cslam_pf_new_feature_step", "cslam_pf_new_feature_step_drawn")


def test_entry_points_are_declared_cited_and_exported():
    names = _capi.declared_symbols()
    assert set(NEED) == set(_capi.PF_NEW_FEATURE_SYMBOLS)
    for s in NEED:
        assert s in names, s
        assert s in _capi._PROTOTYPES, s
    assert os.path.exists(_capi.LIB_PATH), "build the engine first: python -m conan_slam_amd.build"
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert not [s for s in NEED if not hasattr(lib, s)]
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    for cite in ("test/main.cpp:314-328", "slam.h:753-764", "slam.h:413-436", "PF.cpp:9-60", "PF.cpp:419-471"):
        assert cite in text, cite
    # the declarations sit behind the comment that cites them
    block = text[text.index("test/main.cpp:314-328"):text.index("int cslam_pf_new_feature_step_drawn")]
    for cite in ("slam.h:753-764", "slam.h:413-436", "PF.cpp:9-60", "PF.cpp:419-471"):
        assert cite in block, cite


def test_the_wrappers_mirror_the_calls():
    from conan_slam_amd.pf import ParticleShard

    for name in ("sample_pose", "sample_pose_drawn", "new_feature_step", "new_feature_step_drawn", "scan_step_drawn"):
        assert callable(getattr(ParticleShard, name, None)), name
    adapter = open(os.path.join(ROOT, "include", "cslam_adapter.hpp")).read()
    for name in ("sampleNewFeaturePoseAll", "addNewFeaturesSampledAll", "scanStepAll", "cslam_pf_sample_pose_drawn",
                 "cslam_pf_new_feature_step_drawn"):
        assert name in adapter, name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEED + ("scanStepAll", "test/main.cpp:303-328"):
        assert name in doc, name
    kernels = open(os.path.join(ROOT, "conan_slam_amd", "csrc", "pf_new_feature_kernels.hpp")).read()
    for name in ("pf_sample_pose_state", "pf_sample_pose_kernel", "pf_new_feature_step_kernel", "fp contract(off)"):
        assert name in kernels, name


def test_host_check_of_the_arguments(tmp_path):
    """pf_new_feature_check of pf_host_parts.hpp (no HIP include) as a stand-alone program under the address and
    undefined-behaviour sanitizers."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = os.path.join(ROOT, "tests", "host", "pf_new_feature_check.cpp")
    exe = str(tmp_path / "pf_new_feature_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I" + os.path.join(ROOT, "conan_slam_amd", "csrc"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)


def test_adapter_driver_compiles_and_links(tmp_path):
    gxx = shutil.which("g++")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "adapter")]
    libdir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror"] + inc +
                       [os.path.join(ROOT, "tests", "adapter", "adapter_new_features.cpp"), "-L" + libdir, "-lcslam_hip",
                        "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined",
                        "-o", str(tmp_path / "adapter_new_features")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the reference helper
@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_reproduces_an_spd_covariance(dtype):
    o = Oracle(dtype)
    tol = TOL[np.dtype(dtype)]
    for p in random_particles(16, 0, dtype, seed=5):
        L, _ = o.cholesky_decomposition(p[2])
        back = L.astype(np.float64) @ L.astype(np.float64).T
        assert np.abs(back - p[2].astype(np.float64)).max() <= tol * max(1.0, float(np.abs(p[2]).max()))
        assert np.all(np.triu(L, 1) == 0)  # the LLT branch


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_and_indefinite_covariances_keep_the_pose(dtype):
    """slam.h:425-434: a zero factor (Pv = 0) or a non-finite one (a negative eigenvalue), zeroed: X + 0 z = X."""
    parts = random_particles(6, 2, dtype, seed=6)
    parts[1][2] = np.zeros((3, 3), dtype=dtype, order="F")
    parts[4][2] = ref.indefinite_pv(dtype)
    assert np.linalg.eigvalsh(parts[4][2].astype(np.float64)).min() < -0.01
    normals = np.random.default_rng(7).normal(size=(3, 6)).astype(dtype)
    out = ref.new_feature_step(parts, dtype, normals)
    for i, (a, b) in enumerate(zip(parts, out)):
        assert b[0] == a[0] and np.array_equal(b[3], a[3]) and np.array_equal(b[4], a[4]), i   # w, the map: untouched
        assert b[2].tobytes() == np.zeros((3, 3), dtype).tobytes(), i                          # exact zeros
        if i in (1, 4):
            assert b[1].tobytes() == a[1].tobytes(), i
        else:
            assert not np.array_equal(b[1], a[1]), i


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_step_composes_predict_sample_and_add(dtype):
    o = Oracle(dtype)
    parts = random_particles(5, 3, dtype, seed=8)
    normals = np.random.default_rng(9).normal(size=(3, 5)).astype(dtype)
    Z = np.asfortranarray(np.array([[20.0, 35.0], [0.3, -1.1]], dtype=dtype))
    R, Q = R_OBS.astype(dtype), Q_CTRL.astype(dtype)
    out = ref.new_feature_step(parts, dtype, normals, Z, R, predict=PREDICT, Q=Q)
    for i, (a, b) in enumerate(zip(parts, out)):
        X, P = a[1].copy(), np.array(a[2], order="F")
        o.pf_predict(X, P, PREDICT[0], PREDICT[1], Q, PREDICT[2], PREDICT[3])
        L, _ = o.cholesky_decomposition(P)
        want = (L.astype(np.float64) @ normals[:, i].astype(np.float64)) + X
        assert np.abs(b[1] - want).max() <= TOL[np.dtype(dtype)] * max(1.0, np.abs(want).max()), i
        assert b[3].shape == (2, 5) and np.array_equal(b[3][:, :3], a[3]) and np.array_equal(b[4][:, :3], a[4])
        # the features sit at range / bearing Z from the SAMPLED pose
        d = b[3][:, 3:].astype(np.float64) - b[1][:2, None]
        assert np.allclose(np.hypot(d[0], d[1]), Z[0], rtol=1e-5)
        assert b[0] == a[0]


def test_the_loop_case_is_well_conditioned():
    """The loop from an empty map that the GPU file runs (pf_new_feature_ref.loop_*): the Pv that scan 1 samples from and
    scan 2 inverts is positive definite with a condition number below 10^3 -- nowhere near the singular positive-
    semidefinite case, whose factor is not unique -- the f32 oracle's sampled poses are within a tenth of the f32
    tolerance of the f64 oracle's, the poses are pairwise distinct, and scan 2's weights are finite and positive."""
    res = {}
    for dtype in DTYPES:
        n1 = synth.pf_draw_normals(ref.SEED, 2, 0, ref.LOOP_NP, dtype)
        n2 = synth.pf_draw_normals(ref.SEED, 5, 0, ref.LOOP_NP, dtype)
        after1, pv1, w, pv2 = ref.loop_reference(dtype, n1, n2)
        for P in pv1 + pv2:
            ev = np.linalg.eigvalsh(P.astype(np.float64))
            assert ev[0] > 0 and ev[-1] / ev[0] < 1e3, ev
        assert np.all(np.isfinite(w)) and np.all(w > 0), w
        X = np.array([p[1] for p in after1], dtype=np.float64)
        d = np.abs(X[:, None, :] - X[None, :, :]).max(axis=2) + np.eye(ref.LOOP_NP)
        assert d.min() > 1e-3, d.min()
        assert all(p[3].shape == (2, 3) and np.all(np.isfinite(p[3])) for p in after1)
        res[np.dtype(dtype)] = X
    assert np.abs(res[np.dtype(np.float32)] - res[np.dtype(np.float64)]).max() <= 0.1 * TOL[np.dtype(np.float32)]


# ------------------------------------------------------------------------------------------------ the statistical case
@pytest.mark.parametrize("dtype", DTYPES)
def test_distribution_of_the_sampled_poses(dtype):
    """The GPU file's statistical case on the restated draws, at 4 sigma: the GPU test runs the same seed at 5."""
    o = Oracle(dtype)
    normals = synth.pf_draw_normals(ref.SEED, 0, 0, ref.STAT_N, dtype)
    X, P = ref.STAT_X.astype(dtype), np.asfortranarray(ref.STAT_PV.astype(dtype))
    S = np.stack([ref.sample_pose(o, X, P, normals[:, i])[0] for i in range(ref.STAT_N)])
    ref.assert_distribution(S, 4.0, f"cpu {np.dtype(dtype).name}")
    # ... and the check does catch the transposed factor
    L, _ = o.cholesky_decomposition(P)
    bad = (L.T.astype(np.float64) @ normals.astype(np.float64)).T + ref.STAT_X
    with pytest.raises(AssertionError):
        ref.assert_distribution(bad, 5.0, "transposed factor")
