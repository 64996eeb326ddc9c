"""CPU side of the FastSLAM-1 step: the refusal rules as a stand-alone program (plain and under the address and
undefined-behaviour sanitizers); the entry points declared, cited, bound, exported and mirrored; the control stream of
conan_slam_amd.synth; the weight range of every likelihood case the GPU file uses; and the committed draw seeds of the
FastSLAM-1 drive (tests/pf_fs1_ref.py), found by a CPU search, with everything the search looked for asserted here.  Run
with -s to see the figures."""
import ctypes
import os

import numpy as np
import pytest

import pf_drive_ref as D
import pf_fs1_ref as F
from test_host_parts_cpu import build_and_run

from conan_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = ("cslam_pf_control_run_sampled", "cslam_pf_get_control_draws", "cslam_pf_likelihood_update",
        "cslam_pf_fs1_cycle_drawn")


def test_fs1_check_builds_and_passes(tmp_path):
    build_and_run("pf_fs1_check", tmp_path)


def test_entry_points_declared_cited_bound_and_exported():
    from conan_slam_amd import _capi

    names = _capi.declared_symbols()
    assert _capi.PF_FS1_SYMBOLS == NEED
    for n in NEED:
        assert n in names and n in _capi._PROTOTYPES, n
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    block = text[text.index("---- the FastSLAM-1.0 step"):text.index("int cslam_pf_fs1_cycle_drawn")]
    for cite in ("slam.h:102", "slam.h:149-159", "PF.cpp:343-359", "PF.cpp:279-317", "PF.cpp:222-277", "PF.cpp:473-500",
                 "PF.cpp:9-60", "test/main.cpp:277-286", "test/main.cpp:249-334", "PF.cpp:419-471", "PF.cpp:382-417",
                 "PF.cpp:537", "0x4354524C"):
        assert cite in block, cite
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for n in NEED:
        assert hasattr(lib, n), n
    # the prototypes take what the header declares: the control arguments and ctl_step, 4, 7 and 19 arguments
    assert [len(_capi._PROTOTYPES[n]) for n in NEED] == [10, 4, 7, 19]


def test_python_layer_has_the_methods():
    from conan_slam_amd.pf import ParticleShard

    for n in ("control_run_sampled", "control_draws", "likelihood_update", "fs1_cycle_drawn"):
        assert callable(getattr(ParticleShard, n)), n
    for n in ("pf_control_seed", "pf_control_normals", "pf_control_noise"):
        assert callable(getattr(synth, n)), n
    adapter = open(os.path.join(ROOT, "include", "cslam_adapter.hpp")).read()
    for n in ("controlRunSampledAll", "likelihoodUpdateAll", "cycleFastSlam1All"):
        assert n in adapter, n


# ------------------------------------------------------------------------------------------------ the control stream
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_control_stream(dtype):
    seed, step, k, n = 77, 5, 17, 130
    a = synth.pf_control_normals(seed, step, k, 0, n, dtype)
    assert a.shape == (k, 2, n) and a.dtype == dtype
    # reproducible; a pure function of (seed, step, component, slot): a later start or a shard sees the whole's values
    assert a.tobytes() == synth.pf_control_normals(seed, step, k, 0, n, dtype).tobytes()
    assert a[3:].tobytes() == synth.pf_control_normals(seed, step + 3, k - 3, 0, n, dtype).tobytes()
    for first, count in ((0, 65), (65, 65), (129, 1)):
        part = synth.pf_control_normals(seed, step, k, first, count, dtype)
        assert part.tobytes() == np.ascontiguousarray(a[:, :, first:first + count]).tobytes(), (first, count)
    assert synth.pf_control_normals(seed, step, 0, 0, n, dtype).shape == (0, 2, n)
    # independent of the proposal stream: different everywhere from pf_draw_normals of the same (seed, step, slot)
    for j in range(k):
        prop = synth.pf_draw_normals(seed, step + j, 0, n, dtype)
        assert not np.any(a[j] == prop[:2]), j
    assert not np.any(a == synth.pf_control_normals(seed + 1, step, k, 0, n, dtype))
    assert synth.pf_control_seed(seed) == int(synth.splitmix64(seed, 0x4354524C)) != seed
    # every value distinct and plausible
    assert len(set(a.reshape(-1).tolist())) == a.size and np.all(np.isfinite(a)) and np.abs(a).max() < 6.0
    assert abs(float(a.mean())) < 5.0 / np.sqrt(a.size) and abs(float(a.std()) - 1.0) < 5.0 / np.sqrt(2 * a.size)
    # the large control step of the GPU test: pf_draw_key keeps the low 32 bits of 4 step + c above the slot and the
    # normal's two uniforms double the key, so the stream repeats every 2^29 steps -- step 2^31 + 5 is step 5 again
    # (a property of the shared key that the device must reproduce, wrap included); 2^29 - 1 steps on it does not
    big = synth.pf_control_normals(seed, 2 ** 31 + 5, 1, 0, n, dtype)
    assert big[0].tobytes() == a[0].tobytes()
    assert not np.any(synth.pf_control_normals(seed, 2 ** 29 + 4, 1, 0, n, dtype)[0] == a[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_control_noise_arithmetic(dtype):
    T = np.dtype(dtype).type
    Q = np.diag([0.09, 3e-3])
    n = synth.pf_control_normals(3, 0, 4, 0, 9, dtype)
    v, swa = np.array([3.0, 3.1, 2.9, 3.05]), np.array([0.1, -0.2, 0.3, 0.0])
    vn, swan = synth.pf_control_noise(n, v, swa, Q, dtype)
    assert vn.shape == swan.shape == (4, 9) and vn.dtype == swan.dtype == dtype
    s0, s1 = np.sqrt(T(0.09)), np.sqrt(T(3e-3))
    for j in range(4):
        for p in range(9):
            assert vn[j, p] == T(T(v[j]) + T(n[j, 0, p] * s0)) and swan[j, p] == T(T(swa[j]) + T(n[j, 1, p] * s1))
    # a scalar control is broadcast over the steps
    v1, s1_ = synth.pf_control_noise(n, 3.0, 0.1, Q, dtype)
    assert v1[0].tobytes() == vn[0].tobytes() and s1_[0].tobytes() == swan[0].tobytes()
    # Q = 0: the nominal controls bit for bit
    v0, s0_ = synth.pf_control_noise(n, v, swa, np.zeros((2, 2)), dtype)
    assert v0.tobytes() == np.repeat(v.astype(dtype)[:, None], 9, axis=1).tobytes()
    assert s0_.tobytes() == np.repeat(swa.astype(dtype)[:, None], 9, axis=1).tobytes()
    if dtype == np.float32:  # control_noise's arithmetic (slam.h:149-159), fed the same normals
        g0, g1 = n[:, 0, :], n[:, 1, :]
        f = np.float32
        assert vn.tobytes() == (v.astype(f)[:, None] + (g0 * np.sqrt(f(0.09))).astype(f)).astype(f).tobytes()
        assert swan.tobytes() == (swa.astype(f)[:, None] + (g1 * np.sqrt(f(3e-3))).astype(f)).astype(f).tobytes()


# ------------------------------------------------------------------------------------------------ the likelihood cases
def test_likelihood_weights_stay_inside_the_range():
    """Every (m, np) of the GPU file's likelihood test, m <= 17: the f64 oracle's w * like of every particle lies within
    2^+-100, far from the ends of f32; the f32 oracle agrees to 1.7e-4 (measured; held to 5e-4).  The m = 64, 65 cases are
    used in f64 only: they are finite and positive there.  This test guards the INPUTS of the GPU file: it runs the
    reference code and the oracle alone, so it passes on the parent as well and shows nothing about the engine."""
    lo_all, hi_all, worst = np.inf, 0.0, 0.0
    for key in F.likelihood_case_keys():
        for name in ("float32", "float64"):
            case = F.likelihood_case(key, name)
            assert len(set(case.idf.tolist())) == case.m and case.idf.min() >= 1 and case.idf.max() <= case.nf
            if case.m >= 2:
                assert 1 in case.idf and case.nf in case.idf
            wh = case.weights(np.float64).astype(np.float64)
            assert np.all(wh > 2.0 ** -100) and np.all(wh < 2.0 ** 100), (key, name, wh.min(), wh.max())
            lo_all, hi_all = min(lo_all, wh.min() * case.np_), max(hi_all, wh.max() * case.np_)
            if name == "float32":
                wc = case.weights(np.float32).astype(np.float64)
                assert np.all(np.isfinite(wc)) and np.all(wc > 0)
                worst = max(worst, float((np.abs(wc - wh) / wh).max()))
    print(f"likelihoods of the GPU cases (m <= 17): [{lo_all:.3e}, {hi_all:.3e}]; f32 oracle within {worst:.2e} of f64")
    assert worst < 5e-4
    for m in (64, 65):
        case = F.LikelihoodCase(m, F.STAGING_NP, np.float64, nf=F.STAGING_NF)
        wh = case.weights(np.float64)
        assert np.all(np.isfinite(wh)) and np.all(wh > 0), m


# ------------------------------------------------------------------------------------------------ the drive's seeds
def test_the_committed_seeds_give_decisive_drives():
    """What the search looked for: every resample decision of the FastSLAM-1 drives decisive against rounding (in f32:
    the f32 oracle decides as the f64 one on the same inputs, by a factor of 64), at least one scan that resamples and one
    that does not, and every scan kind of the drive present."""
    d = D.committed_drive()
    assert set(d.kinds()) == {D.KNOWN, D.NEW, D.MIXED, D.EMPTY}
    lo, hi, h64 = F.reference("f32"), F.reference("f32hi"), F.reference("f64")
    assert len(lo) == len(hi) == len(h64) == len(d.scans)
    for tag, ms, runs in (("f32", D.margins(hi, lo), hi), ("f64", D.margins(h64), h64)):
        res = [r.resampled for r in runs if r.norm is not None]
        print(f"{tag}: {sum(res)} of {len(res)} scans resample; smallest select gap "
              f"{min(m.select_gap for m in ms):.2e}, Neff gap {min(m.neff_gap for m in ms):.2e}")
        assert D.decisive(ms), tag
        assert any(res) and not all(res), (tag, res)
        assert {r.scan.kind for r in runs} == {D.KNOWN, D.NEW, D.MIXED, D.EMPTY}
        assert runs[-1].nf == d.max_features
        for r in runs:
            assert np.all(np.isfinite(r.rec)) and np.all(r.rec[:, 0] > 0), (tag, r.scan.step)
    amp = D.amplification(lo, hi)
    print(f"amplification of the f32 drive: {amp:.2f} eps32 -> f64 bound {D.f64_bound(amp):.2e}")
    assert amp < 1e3
