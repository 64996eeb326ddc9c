"""The particle filter's draws as conan_slam_amd/synth.py states them (pf_draw_key, pf_draw_normals, pf_draw_select):
the counters never collide, the streams are standard normal and uncorrelated, the strata are pf.py's stratified_random
bit for bit -- and the entry points that draw them on the device are declared and exported.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from conan_slam_amd import _capi, synth
from conan_slam_amd.pf import stratified_keep, stratified_random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]
SELECT_N = [1, 63, 64, 65, 513, 8193]


def test_keys_are_distinct_and_wrap_in_uint64():
    step = np.arange(4, dtype=np.uint64)[:, None, None]
    e = np.arange(4, dtype=np.uint64)[None, :, None]
    g = np.arange(4096, dtype=np.uint64)[None, None, :]
    keys = synth.pf_draw_key(step, e, g)
    assert keys.dtype == np.uint64 and keys.shape == (4, 4, 4096)
    assert np.unique(keys).size == keys.size
    assert int(synth.pf_draw_key(1, 2, 5)) == ((1 * 4 + 2) << 32) | 5
    assert int(synth.pf_draw_key(0, 3, 2**32 - 1)) == (3 << 32) | (2**32 - 1)
    big = 2**31 + 5  # (step * 4 + e) << 32 leaves uint64: it wraps, silently
    assert int(synth.pf_draw_key(big, 1, 7)) == ((((big * 4 + 1) << 32) | 7) & (2**64 - 1))


def test_normals_layout_and_rounding():
    for dtype in DTYPES:
        n = synth.pf_draw_normals(11, 3, 1000, 65, dtype)
        assert n.shape == (3, 65) and n.dtype == dtype
        for e in range(3):
            ref = synth.normal(11, synth.pf_draw_key(3, e, 1000 + np.arange(65, dtype=np.uint64)))
            assert n[e].tobytes() == ref.astype(dtype).tobytes()
    # a shard's slots are a slice of the whole set's
    whole = synth.pf_draw_normals(11, 3, 0, 66, np.float32)
    assert np.array_equal(synth.pf_draw_normals(11, 3, 33, 33, np.float32), whole[:, 33:])


def test_normal_moments():
    x = np.concatenate([synth.pf_draw_normals(12345, t, 0, 4096, np.float64).reshape(-1) for t in range(4)])
    K = x.size
    z_mean, z_var = x.mean() * np.sqrt(K), (x.var() - 1.0) * np.sqrt(K / 2.0)
    print(f"[draws] {K} normals: mean z {z_mean:+.2f}, variance z {z_var:+.2f}")
    assert K == 49152 and abs(z_mean) < 5 and abs(z_var) < 5


def test_streams_and_steps_are_uncorrelated():
    """Sample correlations between the three streams of one step and between two steps of one stream, over 40 seeds:
    each times sqrt(K) is a standard-normal z-score."""
    K, zs = 4096, []
    for seed in range(40):
        a = synth.pf_draw_normals(seed, 5, 0, K, np.float64)
        b = synth.pf_draw_normals(seed, 6, 0, K, np.float64)
        for x, y in ((a[0], a[1]), (a[0], a[2]), (a[1], a[2]), (a[0], b[0]), (a[1], b[1]), (a[2], b[2])):
            zs.append(np.corrcoef(x, y)[0, 1] * np.sqrt(K))
    zs = np.array(zs)
    print(f"[draws] {zs.size} correlation z-scores: std {zs.std():.2f}, largest {np.abs(zs).max():.2f}")
    assert np.abs(zs).max() < 5 and 0.7 < zs.std() < 1.3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SELECT_N)
def test_select_is_stratified_random_of_the_strata_uniforms(n, dtype):
    u = synth.uniform01(77, np.uint64(2) * synth.pf_draw_key(9, 3, np.arange(n, dtype=np.uint64)))
    assert np.array_equal(u, synth.pf_draw_uniforms(77, 9, n)) and np.all((u >= 0) & (u < 1))
    sel = synth.pf_draw_select(77, 9, n, dtype)
    assert sel.dtype == dtype and sel.tobytes() == stratified_random(n, u, dtype).tobytes()
    assert np.all(np.diff(sel) > 0)
    assert abs(u.mean() - 0.5) * np.sqrt(12.0 * n) < 5
    # Uniform weights: slot i keeps particle i.  The strata (k/2, +k, ...) and the weights' running sum (k, +k, ...) are
    # two sequential sums in the particle dtype whose roundings differ (in f32 at n = 8193 each drifts by 0.75 of a
    # stratum, together but not in step), so the identity is certain only for a slot whose draw keeps more distance from
    # both ends of its stratum than the two sums differ by; a slot nearer than that may take a neighbour.
    w = np.full(n, dtype(1) / dtype(n), dtype=dtype)
    keep = stratified_keep(w, sel)
    k = float(dtype(1) / dtype(n))
    steps = np.full(n, dtype(k), dtype=dtype)
    steps[0] = dtype(k) / dtype(2)
    di = np.cumsum(steps, dtype=dtype).astype(np.float64)
    cum = np.cumsum(w, dtype=dtype).astype(np.float64)
    margin = np.abs(di - (cum - k / 2)).max() + 4 * float(np.finfo(dtype).eps)
    safe = (u * k > margin) & ((1.0 - u) * k > margin)
    slots = np.arange(n, dtype=np.int32)
    print(f"[draws] n={n} {np.dtype(dtype).name}: the two running sums differ by {margin / k:.2e} of a stratum, "
          f"{int((~safe).sum())} slots nearer than that to an end, {int((keep != slots).sum())} keep a neighbour")
    assert np.array_equal(keep[safe], slots[safe])
    near = np.nonzero(~safe)[0]
    assert near.size <= max(1, n // 100)  # (a bound of its own, not the sums': fewer than 1 % of the slots are that near)
    assert all(keep[i] in (i - 1, i, i + 1 if i + 1 < n else 0) for i in near)
    if np.dtype(dtype) == np.float64:  # (the sums differ by parts in 10^12 of a stratum: no draw of these is that near)
        assert near.size == 0


def test_entry_points_are_declared_and_exported():
    names = _capi.declared_symbols()
    need = ("cslam_pf_seed_draws", "cslam_pf_get_draws", "cslam_pf_sample_proposal_drawn",
            "cslam_pf_sample_proposal_assoc_drawn", "cslam_pf_resample_local_drawn", "cslam_pf_resample_sharded_drawn",
            "cslam_pf_observation_step_drawn", "cslam_pf_stage_copies")
    assert set(need) == set(_capi.PF_DRAW_SYMBOLS)
    for s in need:
        assert s in names, s
    assert os.path.exists(_capi.LIB_PATH), "build the engine first: python -m conan_slam_amd.build"
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert not [s for s in need if not hasattr(lib, s)]
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    for cite in ("slam.h:753-764", "PF.cpp:557", "PF.cpp:579-596", "slam.h:587-594"):
        assert cite in text, cite


def test_device_header_restates_the_generator_once():
    """pf_draw_kernels.hpp and cslam_sim_batch.hip draw from ONE definition of splitmix64 / uniform01 / counter_normal
    (counter_rng.hpp), in synth.normal's operation order."""
    csrc = os.path.join(ROOT, "conan_slam_amd", "csrc")
    rng = open(os.path.join(csrc, "counter_rng.hpp")).read()
    assert "(2.0 * kPi) * u2" in rng and "log(1.0 - u1)" in rng
    for f in ("pf_draw_kernels.hpp", "cslam_sim_batch.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert '#include "counter_rng.hpp"' in txt and "0x9E3779B97F4A7C15" not in txt, f
    draw = open(os.path.join(csrc, "pf_draw_kernels.hpp")).read()
    assert "pf_stage_draw_kernel" in draw and "fp contract(off)" in draw


def test_adapter_driver_of_the_draws_compiles_and_links(tmp_path):
    """tests/adapter/adapter_draws.cpp -- HipPF::seedDraws / setStep, sampleProposalAll without normals -- built against
    the Eigen-free stand-in and linked against the library, as tests/test_adapter_draws_gpu.py builds it before it runs."""
    import shutil
    import subprocess

    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "adapter")]
    libdir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror"] + inc +
                       [os.path.join(ROOT, "tests", "adapter", "adapter_draws.cpp"), "-L" + libdir, "-lcslam_hip",
                        "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,--allow-shlib-undefined",
                        "-o", str(tmp_path / "adapter_draws")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
