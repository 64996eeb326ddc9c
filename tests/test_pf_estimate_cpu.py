"""The particle filter's read path without a GPU: the ABI is declared and exported, and the expected values that
test_pf_estimate_gpu.py judges the kernels by (tests/pf_estimate_ref.py) are well posed on the inputs used there."""
import ctypes as C
import os

import numpy as np
import pytest

from conan_slam_amd import _capi
from pf_builders import DTYPES, random_particles
from pf_estimate_cases import offset_cloud, wrap_cloud
from pf_estimate_ref import (best_ref, cov_errors, estimate_blocks_ref, estimate_raw_ref, estimate_ref, pi2pi, stack)

NEW = ("cslam_pf_best_particle", "cslam_pf_estimate", "cslam_pf_get_all_features", "cslam_pf_best_particle_sharded",
       "cslam_pf_estimate_sharded")


def test_the_read_path_is_declared_exported_and_cited():
    assert set(NEW) == set(_capi.PF_ESTIMATE_SYMBOLS)
    declared = _capi.declared_symbols()
    raw = C.CDLL(_capi.LIB_PATH) if os.path.exists(_capi.LIB_PATH) else _capi.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(raw, name), name
    text = open(_capi.HEADER_PATH).read()
    for cite in ("slam.h:493-511", "slam.h:505-506", "slam.h:513-539", "CSLAM_PF_PICK_MAX 0", "CSLAM_PF_PICK_MIN 1"):
        assert cite in text, cite


def test_null_handles_are_refused_before_any_device_work():
    L = _capi.lib()
    assert L.cslam_pf_best_particle(None, 0, None, None, None, None, None, None) == _capi.ERR_BAD_ARG
    assert L.cslam_pf_estimate(None, None, None, None, None, None, None) == _capi.ERR_BAD_ARG
    assert L.cslam_pf_get_all_features(None, None) == _capi.ERR_BAD_ARG
    assert L.cslam_pf_best_particle_sharded(None, None, 0, None, None, None, None, None, None) == _capi.ERR_BAD_ARG
    assert L.cslam_pf_estimate_sharded(None, None, None, None, None, None, None, None) == _capi.ERR_BAD_ARG


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blocks", [2, 4, 8])
@pytest.mark.parametrize("cloud", ["random", "offset"])
def test_block_summaries_merged_in_order_give_the_two_pass_moments(dtype, blocks, cloud):
    """The sharded expectation is well posed: per-block summaries merged in block order (Chan) reproduce the two-pass
    moments of the whole set within 1e-10 of the largest covariance entry -- on 65 particles per block, as the GPU test
    shards them."""
    n = 65 * blocks
    parts = random_particles(n, 3, dtype, seed=31) if cloud == "random" else offset_cloud(n, 3, dtype)
    arrs = stack(parts)
    ref, got = estimate_ref(*arrs), estimate_blocks_ref(*arrs, blocks)
    assert abs(got.w_sum - ref.w_sum) <= 1e-13 * ref.w_sum and abs(got.neff - ref.neff) <= 1e-12 * ref.neff
    for name in ("Pv", "PF"):
        a, b = getattr(got, name), getattr(ref, name)
        assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (name, float(np.abs(a - b).max()), float(np.abs(b).max()))
    assert np.abs(got.Xv[:2] - ref.Xv[:2]).max() <= 1e-12 * max(1.0, np.abs(ref.Xv).max())
    assert abs(pi2pi(got.Xv[2] - ref.Xv[2])) <= 1e-12
    assert np.abs(got.XF - ref.XF).max() <= 1e-12 * max(1.0, np.abs(ref.XF).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_heading_mean_is_circular(dtype):
    arrs = stack(wrap_cloud(64, 1, dtype))
    phi = arrs[1][:, 2]
    assert phi.min() < -3.0 and phi.max() > 3.0, "the cloud must straddle +-pi"
    ref = estimate_ref(*arrs)
    assert abs(pi2pi(ref.Xv[2] - 3.1)) < 0.05, ref.Xv[2]
    assert abs(np.average(phi, weights=arrs[0])) < 2.5, "(the arithmetic mean is nowhere near)"
    assert 1e-3 < ref.Pv[2, 2] < 2e-2, ref.Pv[2, 2]


@pytest.mark.parametrize("npart", [65, 257])
def test_raw_moments_in_f64_miss_the_f32_tolerance_on_the_offset_cloud(npart):
    """The GPU case can tell a centred kernel from an uncentred one: sum w x x^T / W - xbar xbar^T accumulated in float64
    on the f32 handle's values is outside the f32-handle covariance tolerance; the block-merged form is inside."""
    arrs = stack(offset_cloud(npart, 2, np.float32))
    ref = estimate_ref(*arrs)
    raw = estimate_raw_ref(*arrs)
    for name in ("Pv", "PF"):
        err, bound = cov_errors(getattr(raw, name), getattr(ref, name), np.float32)
        print(f"raw {name} np={npart}: worst err/bound {float((err / bound).max()):.3g}, "
              f"relative to the covariance {float(err.max() / np.abs(getattr(ref, name)).max()):.3g}")
        assert np.any(err > bound), name


def test_best_ref_rules():
    assert best_ref([0.25, 0.25, 0.25], "max") == 0 and best_ref([0.25, 0.25, 0.25], "min") == 0
    w = np.full(320, 0.1)
    w[[70, 300]] = 0.9
    assert best_ref(w, "max") == 70 and best_ref(w, "min") == 0
    w[3] = np.nan
    assert best_ref(w, "max") == 70 and best_ref(w, "min") == 0
    assert best_ref([np.nan, np.nan], "max") == 0 and best_ref([np.nan, 2.0, 1.0], "min") == 2


def test_adapter_estimate_driver_compiles_and_links(tmp_path):
    """tests/adapter/adapter_estimate.cpp (HipPF::extractStates / extractFeatures / extractMap), which
    test_adapter_estimate_gpu.py builds and runs on the GPU box: the same compile and link here."""
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    libdir = os.path.dirname(os.path.abspath(_capi.LIB_PATH))
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
           "-I" + os.path.join(root, "tests", "adapter"), os.path.join(root, "tests", "adapter", "adapter_estimate.cpp"),
           "-L" + libdir, "-lcslam_hip", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined",
           "-o", str(tmp_path / "adapter_estimate")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
