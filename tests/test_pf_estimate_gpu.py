"""The particle filter's read path on the device: cslam_pf_best_particle (slam.h:493-511), cslam_pf_estimate (the mixture
moments), cslam_pf_get_all_features (slam.h:513-539) and the sharded forms, against the float64 two-pass numpy helper
(tests/pf_estimate_ref.py) applied to the values the handle stores.  Selections must match bit for bit; moments within
the tolerances derived in pf_estimate_ref.mean_errors / cov_errors."""
import numpy as np
import pytest

from pf_builders import DTYPES, PREDICT, ProposalCase, random_particles, shard_from
from pf_estimate_cases import offset_cloud, wrap_cloud
from pf_estimate_ref import (all_features_ref, assert_moments, best_ref, cov_errors, download, estimate_raw_ref,
                             estimate_ref, pi2pi, stack)
from test_pf_gpu import _run_ranks

pytestmark = pytest.mark.gpu

NFCAP = 5
CHUNK = 1024  # kEstChunk of pf_estimate_kernels.hpp: particles one workgroup covers
EDGE_NP = [1, 2, 63, 64, 65, 255, 256, 257, CHUNK + 1]
EDGE_NF = [0, 1, 2, NFCAP]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_bits(a, b):
    """Two named tuples of the read path: every field identical bit for bit (None fields alike)."""
    for x, y in zip(a, b):
        if x is None or y is None:
            if x is not y:
                return False
        elif _bits(np.asarray(x)) != _bits(np.asarray(y)):
            return False
    return True


def _assert_best(tag, got, arrs, pick, dtype, offset=0):
    w, X, P, XF, PF = arrs
    i = best_ref(w, pick)
    assert got.index == i + offset, (tag, pick, got.index, i + offset)
    for name, a, b in (("w", got.w, w[i]), ("Xv", got.Xv, X[i]), ("Pv", got.Pv, P[i]), ("XF", got.XF, XF[i]),
                       ("PF", got.PF, PF[i])):
        assert _bits(np.asarray(a, dtype=dtype)) == _bits(np.asarray(b).astype(dtype)), (tag, pick, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf", EDGE_NF)
@pytest.mark.parametrize("npart", EDGE_NP)
def test_edges_of_the_dispatch(gpu_required, npart, nf, dtype):
    """Below, at and above one wave (64), one workgroup's threads (256) and one workgroup's chunk (1024), with no map, one
    feature, two, and the handle's capacity: estimate, both picks and the transposing gather against the helper, and
    the store bit-identical afterwards."""
    parts = random_particles(npart, nf, dtype, seed=100 * npart + nf)
    sh = shard_from(parts, NFCAP, dtype)
    arrs = stack(parts)
    tag = f"np={npart} nf={nf} {np.dtype(dtype).name}"
    est = sh.estimate()
    assert est.XF.shape == (2, nf) and est.PF.shape == (4, nf)
    assert_moments(tag, est, estimate_ref(*arrs), dtype)
    for pick in ("max", "min"):
        _assert_best(tag, sh.best_particle(pick), arrs, pick, dtype)
    allf = sh.all_features()
    after = download(sh)
    assert allf.shape == (2, npart * nf) and allf.dtype == np.dtype(dtype)
    assert _bits(allf) == _bits(all_features_ref(after[3]).astype(dtype)), tag
    for name, a, b in zip("w X P XF PF".split(), after, arrs):
        assert np.array_equal(a, b), (tag, "the store changed", name)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npart", [65, 257])
def test_offset_tight_cloud_needs_centred_moments(gpu_required, npart, dtype):
    """5 km from the origin with 5 cm of scatter: the covariances meet the tolerance, which float64 raw moments
    (sum w x x^T / W - xbar xbar^T) on the same values do not."""
    parts = offset_cloud(npart, 2, dtype)
    sh = shard_from(parts, 2, dtype)
    arrs = stack(parts)
    ref, raw = estimate_ref(*arrs), estimate_raw_ref(*arrs)
    for name in ("Pv", "PF"):
        err, bound = cov_errors(getattr(raw, name), getattr(ref, name), dtype)
        assert np.any(err > bound), ("the case cannot tell raw moments from centred ones", name)
    assert_moments(f"offset np={npart} {np.dtype(dtype).name}", sh.estimate(), ref, dtype)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_heading_across_pi(gpu_required, dtype):
    parts = wrap_cloud(64, 2, dtype)
    sh = shard_from(parts, 2, dtype)
    arrs = stack(parts)
    assert arrs[1][:, 2].min() < -3.0 and arrs[1][:, 2].max() > 3.0
    ref, est = estimate_ref(*arrs), sh.estimate()
    assert_moments(f"wrap {np.dtype(dtype).name}", est, ref, dtype)
    assert abs(pi2pi(float(est.Xv[2]) - 3.1)) < 0.05, est.Xv
    assert 1e-3 < float(est.Pv[2, 2]) < 2e-2, est.Pv  # (an arithmetic variance would be near pi^2)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_and_bad_weights(gpu_required, dtype):
    npart, nf = 320, 2
    parts = random_particles(npart, nf, dtype, seed=77)
    sh = shard_from(parts, nf, dtype)
    arrs = list(stack(parts))

    def with_weights(w):
        w = np.asarray(w, dtype=dtype)
        sh.set_weights(w)
        arrs[0] = w.astype(np.float64)

    with_weights(np.full(npart, 1.0 / npart))
    assert sh.best_particle("max").index == 0 and sh.best_particle("min").index == 0
    w = np.full(npart, 0.001)
    w[[70, 300]] = 0.25
    with_weights(w)
    _assert_best("two maxima", sh.best_particle("max"), arrs, "max", dtype)
    assert sh.best_particle("max").index == 70 and sh.best_particle("min").index == 0
    w[3] = np.nan
    w[5] = 1e-6  # (the minimum proper)
    with_weights(w)
    assert sh.best_particle("max").index == 70 and sh.best_particle("min").index == 5
    est = sh.estimate()
    assert np.isnan(est.w_sum) and np.isnan(est.Xv).all() and np.isnan(est.PF).all()
    w[:] = np.nan
    with_weights(w)
    for pick in ("max", "min"):
        _assert_best("all NaN", sh.best_particle(pick), arrs, pick, dtype)
        assert sh.best_particle(pick).index == 0
    with_weights(np.zeros(npart))
    est = sh.estimate()
    assert est.w_sum == 0.0 and np.isnan(est.neff)
    for a in (est.Xv, est.Pv, est.XF, est.PF):
        assert np.isnan(a).all()
    for pick in ("max", "min"):
        _assert_best("all zero", sh.best_particle(pick), arrs, pick, dtype)
    # a bad pick is refused
    import ctypes as C

    from conan_slam_amd import _capi

    assert _capi.lib().cslam_pf_best_particle(sh._h, C.c_int(2), None, None, None, None, None, None) == _capi.ERR_BAD_ARG
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_estimate_is_ordered_behind_queued_work(gpu_required, dtype):
    """One fused observation step (asynchronous) and the estimate right behind it, with no synchronise in between: the
    estimate is that of the advanced store; a second call returns identical bits."""
    from conan_slam_amd.pf import stratified_random

    case = ProposalCase(4, 73, dtype, nf=6, predict=True)
    sh = shard_from(case.parts, 6, dtype)
    sel = stratified_random(73, np.random.default_rng(5).uniform(size=73), dtype)
    sh.observation_step(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3], case.Z, case.idf, case.R, case.normals,
                        sel, 0.0, False)
    est = sh.estimate()
    again = sh.estimate()
    arrs = download(sh)
    assert not np.array_equal(arrs[1], stack(case.parts)[1]), "the step must have moved the poses"
    assert np.ptp(arrs[0]) > 0, "the step must have left non-uniform weights"
    assert_moments(f"stream order {np.dtype(dtype).name}", est, estimate_ref(*arrs), dtype)
    assert _same_bits(est, again)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npart", [65, CHUNK + 1])
def test_null_map_outputs_leave_the_pose_alone(gpu_required, npart, dtype):
    parts = random_particles(npart, 3, dtype, seed=8)
    sh = shard_from(parts, 3, dtype)
    full, pose = sh.estimate(), sh.estimate(want_map=False)
    assert pose.XF is None and pose.PF is None
    assert _same_bits(full[:4], pose[:4])
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("world", [1, 2, 4])
def test_sharded_estimate_and_best_particle_loopback(gpu_required, world, dtype):
    """65 particles per rank, 3 features, one host thread per rank behind the loopback communicator: every rank returns
    the same bits; they agree with the helper on the concatenated set and with one handle holding all particles; the
    best particle is the single handle's, with its GLOBAL index -- also when ranks 1 and 3 hold equal maxima.  A world
    of one equals the unsharded call bit for bit."""
    from conan_slam_amd.pf import LoopbackComm

    L, nf = 65, 3
    n = world * L
    parts = random_particles(n, nf, dtype, seed=40 + world)
    if world == 4:
        parts[1 * L + 10][0] = parts[3 * L + 5][0] = dtype(0.5)  # equal maxima: rank 1's (global 75) must win
    arrs = stack(parts)
    tag = f"world={world} {np.dtype(dtype).name}"
    whole = shard_from(parts, nf, dtype)
    shards = [shard_from(parts[r * L:(r + 1) * L], nf, dtype) for r in range(world)]
    comms = LoopbackComm.create(world)

    def rank(r):
        return (shards[r].estimate_sharded(comms[r]), shards[r].estimate_sharded(comms[r], want_map=False),
                shards[r].best_particle_sharded(comms[r], "max"), shards[r].best_particle_sharded(comms[r], "min"))

    res = _run_ranks([(lambda r=r: rank(r)) for r in range(world)])
    ref = estimate_ref(*arrs)
    single, single_pose = whole.estimate(), whole.estimate(want_map=False)
    for r in range(world):
        est, pose, bmax, bmin = res[r]
        for k in range(4):
            assert _same_bits(res[r][k], res[0][k]), (tag, "ranks differ", r, k)
        assert _same_bits(est[:4], pose[:4]), (tag, "want_map changed the pose", r)
    est, pose, bmax, bmin = res[0]
    assert_moments(tag + " vs helper", est, ref, dtype)
    assert_moments(tag + " vs single handle", est, single, dtype)
    for pick, got in (("max", bmax), ("min", bmin)):
        _assert_best(tag, got, arrs, pick, dtype)
        assert _same_bits(got, whole.best_particle(pick)), (tag, pick)
    if world == 4:
        assert bmax.index == 1 * L + 10
    if world == 1:
        assert _same_bits(est, single) and _same_bits(pose, single_pose), tag
    for c in comms:
        c.close()
    for sh in shards + [whole]:
        sh.close()
