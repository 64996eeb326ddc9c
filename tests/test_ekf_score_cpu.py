"""The single handle's device-side score and pose read without a GPU: include/cslam.h declares the five calls and cites the
reference, the built library exports them, each answers CSLAM_ERR_NO_DEVICE where there is no GPU (there is no handle to
pass then, and no CPU fallback), the Python class and the reference-side binding reach them, and the restatement's trace
bound is as tight as the GPU tests need."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

import conan_slam_amd
from conan_slam_amd import EKF, _capi
from ekf_score_ref import trace_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cslam_ekf_get_pose", "cslam_ekf_score_reset", "cslam_ekf_score_set_truth", "cslam_ekf_score", "cslam_ekf_get_scores")


def test_header_declares_the_calls_and_cites_the_reference():
    names = _capi.declared_symbols()
    assert set(NEW) <= set(names) and tuple(_capi.EKF_SCORE_SYMBOLS) == NEW
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    for name in NEW:
        at = text.index("int " + name + "(")
        comment = text[text.rindex("/*", 0, at):at]
        for cite in ("test/main.cpp:136", "EKF.cpp:131-144", "slam.h:841-847"):
            assert cite in comment, (name, cite)
        assert re.search(r"\*/\s*$", comment), (name, "the comment must end right above the declaration")
        assert name in _capi._PROTOTYPES, name
    assert "int cslam_ekf_get_pose(cslam_ekf_t h, void* x /* [3] */, void* pvv /* [9] */);" in text
    assert "int cslam_ekf_score(cslam_ekf_t h, const double* xv_true /* host [3] */, int with_map);" in text
    assert "f32 batch only" not in text and "have no scorer" not in text


def test_library_exports_the_calls():
    assert os.path.exists(_capi.LIB_PATH), "build the engine first: python -m conan_slam_amd.build"
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for s in NEW:
        assert hasattr(lib, s), s
    L = _capi.lib()
    for s, nargs in zip(NEW, (3, 4, 3, 3, 7)):
        assert getattr(L, s).restype is ctypes.c_int and len(getattr(L, s).argtypes) == nargs, s
    for member in ("pose", "score_reset", "score_set_truth", "score", "scores"):
        assert callable(getattr(EKF, member, None)), member


def test_no_device_no_score():
    """Without a GPU no handle can exist: every call says CSLAM_ERR_NO_DEVICE.  (Where a GPU is visible the same calls
    refuse the null handle as a bad argument.)"""
    L = _capi.lib()
    want = _capi.ERR_NO_DEVICE if conan_slam_amd.device_count() == 0 else _capi.ERR_BAD_ARG
    buf = np.zeros(16, np.float64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    rec, calls = ctypes.c_int(0), ctypes.c_longlong(0)
    assert L.cslam_ekf_get_pose(None, p, p) == want
    assert L.cslam_ekf_score_reset(None, 4, 0.0, 0.0) == want
    assert L.cslam_ekf_score_set_truth(None, p, 2) == want
    assert L.cslam_ekf_score(None, p, 1) == want
    assert L.cslam_ekf_get_scores(None, p, None, None, 0, ctypes.byref(rec), ctypes.byref(calls)) == want
    assert not np.any(buf)
    if want == _capi.ERR_NO_DEVICE:
        assert "no CPU fallback" in L.cslam_last_error().decode()


def test_adapter_program_compiles_and_links(tmp_path):
    """tests/adapter/adapter_ekf_score.cpp (run on the GPU by tests/test_adapter_ekf_score_gpu.py) against the stand-in."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tests", "adapter"),
                        os.path.join(ROOT, "tests", "adapter", "adapter_ekf_score.cpp"), "-L" + libdir, "-lcslam_hip",
                        "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o",
                        str(tmp_path / "adapter_ekf_score")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "include", "cslam_adapter.hpp")).read()
    ekf = text[text.index("class HipEKF"):text.index("class HipPF")]
    for member in ("void pose(", "void scoreReset(", "void scoreTruth(", "void score(", "long long scores("):
        assert member in ekf, member


def test_trace_bound_is_tight():
    """2 (n - 1) u sum |d| at the sizes the GPU tests use: far below a relative 1e-9, and it holds for a sum in the
    device's order (pairs, a tree of 64, four waves, blocks, then the pose) against the exact one."""
    rng = np.random.default_rng(0)
    for N in (1, 257, 5000):
        d = rng.uniform(0.5, 3.0, size=3 + 2 * N)
        exact, b = trace_ref(d)
        assert b < 1e-9 * abs(exact) / 100
        lanes = np.zeros(-(-N // 256) * 256)
        lanes[:N] = d[3:3 + N] + d[3 + N:]
        tree = lanes.reshape(-1, 4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            tree = tree[..., :off] + tree[..., off:2 * off]
        waves = tree[..., 0]
        blocks = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
        lm = 0.0
        for v in blocks:
            lm += v
        assert abs((((d[0] + d[1]) + d[2]) + lm) - exact) <= b
