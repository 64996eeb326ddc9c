"""The scan that observes only new features (test/main.cpp:314-328) on the device: pf_sample_pose_kernel and
pf_new_feature_step_kernel (conan_slam_amd/csrc/pf_new_feature_kernels.hpp) behind cslam_pf_sample_pose,
cslam_pf_new_feature_step and their _drawn forms, and the scan dispatcher ParticleShard.scan_step_drawn.

Parity is against tests/pf_new_feature_ref.py (the CPU oracle composed) within pf_builders.TOL; weights, the existing
features and the zeros of Pv are held bit for bit; the fused kernel against the separate calls, every _drawn call against
its host-array twin and a sharded set against the whole one are bit for bit on the whole store."""
import ctypes as C

import numpy as np
import pytest

import pf_new_feature_ref as ref
from pf_builders import DTYPES, PREDICT, Q_CTRL, R_OBS, TOL, compare, random_particles, shard_from
from test_pf_edges_gpu import _assert_shards_bit_equal, _bulk_read, _bulk_shard, _same_bits

pytestmark = pytest.mark.gpu

CAP = 8
NP_CASES = [1, 63, 64, 65, 130]
NF_Q_CASES = [(0, 1), (0, 2), (5, 3), (CAP - 2, 2)]  # the last one writes the last slot of the store


def _new_obs(q, dtype, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.stack([rng.uniform(10.0, 60.0, q), rng.uniform(-3.0, 3.0, q)]).astype(dtype))


def _normals(npart, dtype, seed):
    return np.random.default_rng(seed).normal(size=(3, npart)).astype(dtype)


def _assert_untouched(sh, parts, nf0, dtype, tag):
    """Weights and the features 0 .. nf0 - 1 bitwise as uploaded, Pv exact zeros (one bulk read of the store)."""
    rec = _bulk_read(sh)
    nf = sh.n_features
    assert rec.shape == (len(parts), 13 + 6 * nf), tag
    assert _same_bits(rec[:, 0], np.array([p[0] for p in parts], dtype=dtype)), (tag, "weights")
    assert rec[:, 4:13].tobytes() == np.zeros((len(parts), 9), dtype).tobytes(), (tag, "Pv")
    if nf0:
        xf = np.array([p[3].reshape(-1, order="F") for p in parts], dtype=dtype)
        pf = np.array([p[4].reshape(-1, order="F") for p in parts], dtype=dtype)
        assert _same_bits(rec[:, 13:13 + 2 * nf0], xf), (tag, "XF")
        assert _same_bits(rec[:, 13 + 2 * nf:13 + 2 * nf + 4 * nf0], pf), (tag, "PF")


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf0,q", NF_Q_CASES)
@pytest.mark.parametrize("npart", NP_CASES)
def test_parity_with_the_reference(gpu_required, npart, nf0, q, dtype):
    parts = random_particles(npart, nf0, dtype, seed=100 + npart + nf0)
    normals = _normals(npart, dtype, 200 + npart)
    Z, R, Q = _new_obs(q, dtype, 300 + q), R_OBS.astype(dtype), Q_CTRL.astype(dtype)
    tag = f"np={npart} nf0={nf0} q={q}"
    # sample_pose alone
    sh = shard_from(parts, CAP, dtype)
    sh.sample_pose(normals)
    compare(sh, ref.new_feature_step(parts, dtype, normals), dtype, tag + " sample_pose", wtol=0.0)
    assert sh.n_features == nf0
    _assert_untouched(sh, parts, nf0, dtype, tag + " sample_pose")
    sh.close()
    # the whole branch, without and with the predict
    for predict in (None, PREDICT):
        sh = shard_from(parts, CAP, dtype)
        sh.new_feature_step(*(PREDICT[:2] if predict else (0.0, 0.0)), Q if predict else None,
                            *(PREDICT[2:] if predict else (0.0, 0.0)), Z, R, normals)
        want = ref.new_feature_step(parts, dtype, normals, Z, R, predict=predict, Q=Q)
        assert sh.n_features == nf0 + q, tag
        compare(sh, want, dtype, f"{tag} step predict={predict is not None}", wtol=0.0)
        _assert_untouched(sh, parts, nf0, dtype, f"{tag} step predict={predict is not None}")
        sh.close()


# ------------------------------------------------------------------------------------------------ 2. the fallback branch
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_and_indefinite_covariances_beside_spd_ones(gpu_required, dtype):
    """One wave of 64: particles with Pv = 0 and with one negative eigenvalue between SPD neighbours.  The factor of the
    former is zero, of the latter not finite and zeroed (slam.h:425-434): their poses come back bit for bit, and the
    divergent lanes leave their neighbours as the reference has them."""
    npart, nf0, q = 64, 2, 2
    parts = random_particles(npart, nf0, dtype, seed=41)
    zero, indef = [0, 17, 31, 32, 63], [1, 16, 33, 62]
    for i in zero:
        parts[i][2] = np.zeros((3, 3), dtype=dtype, order="F")
    for i in indef:
        parts[i][2] = ref.indefinite_pv(dtype)
    normals = _normals(npart, dtype, 42)
    Z, R = _new_obs(q, dtype, 43), R_OBS.astype(dtype)
    a, b = shard_from(parts, CAP, dtype), shard_from(parts, CAP, dtype)
    a.sample_pose(normals)
    b.new_feature_step(0.0, 0.0, None, 0.0, 0.0, Z, R, normals)
    compare(a, ref.new_feature_step(parts, dtype, normals), dtype, "fallback sample_pose", wtol=0.0)
    compare(b, ref.new_feature_step(parts, dtype, normals, Z, R), dtype, "fallback step", wtol=0.0)
    for sh in (a, b):
        for i in zero + indef:
            assert _same_bits(sh.get_particle(i)[1], parts[i][1]), i
        moved = [i for i in range(npart) if not _same_bits(sh.get_particle(i)[1], parts[i][1])]
        assert moved == [i for i in range(npart) if i not in zero + indef]
        _assert_untouched(sh, parts, nf0, dtype, "fallback")
        sh.close()


# ------------------------------------------------------------------------------------------------ 3. fused vs unfused
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_against_the_separate_calls(gpu_required, dtype):
    """new_feature_step(Q = NULL) against sample_pose + add_features on a twin: xv, Pv, w bit for bit (both kernels
    inline pf_sample_pose_state, contraction off); the new features within TOL (their expressions sit in two kernels)."""
    npart, nf0, q = 130, 5, 3
    parts = random_particles(npart, nf0, dtype, seed=51)
    normals = _normals(npart, dtype, 52)
    Z, R = _new_obs(q, dtype, 53), R_OBS.astype(dtype)
    a, b = shard_from(parts, CAP, dtype), shard_from(parts, CAP, dtype)
    a.new_feature_step(0.0, 0.0, None, 0.0, 0.0, Z, R, normals)
    b.sample_pose(normals)
    b.add_features(Z, R)
    ra, rb = _bulk_read(a), _bulk_read(b)
    assert a.n_features == b.n_features == nf0 + q
    assert _same_bits(ra[:, :13], rb[:, :13])
    tol = TOL[np.dtype(dtype)]
    err = np.abs(ra[:, 13:].astype(np.float64) - rb[:, 13:].astype(np.float64)).max()
    scale = max(1.0, float(np.abs(rb[:, 13:]).max()))
    print(f"[new-feature] fused vs separate {np.dtype(dtype).name}: features differ by {err:.3e} (tolerance {tol * scale:.3e})")
    assert err <= tol * scale
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. drawn vs host arrays
DRAW_SEED = 424242


@pytest.mark.parametrize("dtype", DTYPES)
def test_drawn_calls_against_their_host_array_twins(gpu_required, dtype):
    """A shard seeded for slots 1000.. of 2000 (any shard serves: no collective in this branch).  Each _drawn call
    against its twin fed get_draws(step): the whole store bit for bit; no staged copy up to 32 new observations, one at 33."""
    npart, nf0, cap = 65, 3, 40
    parts = random_particles(npart, nf0, dtype, seed=61)
    R, Q = R_OBS.astype(dtype), Q_CTRL.astype(dtype)
    a, b = shard_from(parts, cap, dtype), shard_from(parts, cap, dtype)
    a.seed_draws(DRAW_SEED, 1000, 2000)
    step = 7
    normals, _ = a.draws(step, select=False)
    copies = a.stage_copies()
    a.sample_pose_drawn(step)
    b.sample_pose(normals)
    assert a.stage_copies() == copies
    _assert_shards_bit_equal(a, b, "sample_pose_drawn")
    assert not _same_bits(a.get_particle(0)[1], parts[0][1])
    a.close()
    b.close()
    for q in (1, 32, 33):
        a, b = shard_from(parts, cap, dtype), shard_from(parts, cap, dtype)
        a.seed_draws(DRAW_SEED, 1000, 2000)
        Z = _new_obs(q, dtype, 62 + q)
        step = 10 + q
        normals, _ = a.draws(step, select=False)
        copies = a.stage_copies()
        a.new_feature_step_drawn(PREDICT[0], PREDICT[1], Q, PREDICT[2], PREDICT[3], Z, R, step)
        b.new_feature_step(PREDICT[0], PREDICT[1], Q, PREDICT[2], PREDICT[3], Z, R, normals)
        assert a.stage_copies() - copies == (1 if q > 32 else 0), q
        assert a.n_features == b.n_features == nf0 + q
        _assert_shards_bit_equal(a, b, f"new_feature_step_drawn q={q}")
        assert _same_bits(a.draws(step, select=False)[0], normals)  # get_draws returns what the call consumed
        a.close()
        b.close()


def test_unseeded_handle_is_refused(gpu_required):
    from conan_slam_amd import CslamError, _capi

    dtype = np.float32
    parts = random_particles(9, 2, dtype, seed=71)
    a, twin = shard_from(parts, CAP, dtype), shard_from(parts, CAP, dtype)
    copies = a.stage_copies()
    for call in (lambda: a.sample_pose_drawn(0),
                 lambda: a.new_feature_step_drawn(*PREDICT[:2], Q_CTRL, *PREDICT[2:], _new_obs(2, dtype, 1), R_OBS, 0)):
        with pytest.raises(CslamError) as ei:
            call()
        assert ei.value.code == _capi.ERR_BAD_ARG and str(ei.value).strip()
    assert a.n_features == 2 and a.stage_copies() == copies
    _assert_shards_bit_equal(a, twin, "unseeded, refused")
    a.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 5. sharding
@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_equal_the_whole_set(gpu_required, dtype):
    """130 particles on one handle seeded (seed, 0, 130) against the same particles on handles of 64 and 66 seeded
    (seed, 0, 130) and (seed, 64, 130): a draw depends on the GLOBAL slot, so every record is the whole set's."""
    N, cut, nf0, q, step = 130, 64, 2, 2, 5
    parts = random_particles(N, nf0, dtype, seed=81)
    Z, R, Q = _new_obs(q, dtype, 82), R_OBS.astype(dtype), Q_CTRL.astype(dtype)
    whole = shard_from(parts, CAP, dtype)
    lo, hi = shard_from(parts[:cut], CAP, dtype), shard_from(parts[cut:], CAP, dtype)
    whole.seed_draws(DRAW_SEED, 0, N)
    lo.seed_draws(DRAW_SEED, 0, N)
    hi.seed_draws(DRAW_SEED, cut, N)
    for sh in (whole, lo, hi):
        sh.new_feature_step_drawn(PREDICT[0], PREDICT[1], Q, PREDICT[2], PREDICT[3], Z, R, step)
    rw = _bulk_read(whole)
    assert np.all(np.isfinite(rw))
    assert _same_bits(np.concatenate([_bulk_read(lo), _bulk_read(hi)]), rw)
    for sh in (whole, lo, hi):
        sh.close()


# ------------------------------------------------------------------------------------------------ 6. the distribution
@pytest.mark.parametrize("dtype", DTYPES)
def test_distribution_of_the_sampled_poses(gpu_required, dtype):
    """4096 particles with one common SPD (X, Pv), sample_pose_drawn: the sample mean within 5 sqrt(Pii / N) of X and
    every sample covariance entry within 5 sqrt((Pii Pjj + Pij^2) / N) of Pv -- the sampling error of a Gaussian's
    moments, at the seed the CPU test showed inside 4 sigma.  A transposed factor is off by hundreds of sigmas."""
    n = ref.STAT_N
    rec = np.zeros((n, 19), dtype)
    rec[:, 0] = 1.0 / n
    rec[:, 1:4] = ref.STAT_X
    rec[:, 4:13] = ref.STAT_PV.reshape(-1, order="F")
    rec[:, 13:15], rec[:, 15], rec[:, 18] = (5.0, 6.0), 0.3, 0.3
    sh = _bulk_shard(rec, dtype)
    sh.seed_draws(ref.SEED, 0, n)
    sh.sample_pose_drawn(0)
    out = _bulk_read(sh)
    assert _same_bits(out[:, 0], rec[:, 0]) and _same_bits(out[:, 13:], rec[:, 13:])
    assert out[:, 4:13].tobytes() == np.zeros((n, 9), dtype).tobytes()
    ref.assert_distribution(out[:, 1:4], 5.0, f"device {np.dtype(dtype).name}")
    sh.close()


# ------------------------------------------------------------------------------------------------ 7. errors
@pytest.mark.parametrize("dtype", DTYPES)
def test_refused_calls_change_nothing(gpu_required, dtype):
    from conan_slam_amd import _capi

    npart, nf0 = 9, CAP - 2
    parts = random_particles(npart, nf0, dtype, seed=91)
    a, twin = shard_from(parts, CAP, dtype), shard_from(parts, CAP, dtype)
    a.seed_draws(DRAW_SEED)
    L, h = a._L, a._h
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    Z3, Z2 = _new_obs(3, dtype, 92).reshape(-1, order="F").copy(), _new_obs(2, dtype, 93).reshape(-1, order="F").copy()
    R = np.asfortranarray(R_OBS.astype(dtype))
    Q = np.asfortranarray(Q_CTRL.astype(dtype))
    nrm = np.ascontiguousarray(_normals(npart, dtype, 94))
    ctl = lambda: (C.c_double(PREDICT[0]), C.c_double(PREDICT[1]), vp(Q), C.c_double(PREDICT[2]), C.c_double(PREDICT[3]))
    step, drawn = L.cslam_pf_new_feature_step, L.cslam_pf_new_feature_step_drawn
    copies = a.stage_copies()
    cases = [
        ("capacity", _capi.ERR_CAPACITY, lambda: step(h, *ctl(), vp(Z3), 3, vp(R), vp(nrm))),
        ("capacity drawn", _capi.ERR_CAPACITY, lambda: drawn(h, *ctl(), vp(Z3), 3, vp(R), 4)),
        ("q < 0", _capi.ERR_BAD_ARG, lambda: step(h, *ctl(), vp(Z2), -1, vp(R), vp(nrm))),
        ("q < 0 drawn", _capi.ERR_BAD_ARG, lambda: drawn(h, *ctl(), vp(Z2), -1, vp(R), 4)),
        ("null R", _capi.ERR_BAD_ARG, lambda: step(h, *ctl(), vp(Z2), 2, None, vp(nrm))),
        ("null R drawn", _capi.ERR_BAD_ARG, lambda: drawn(h, *ctl(), vp(Z2), 2, None, 4)),
        ("null Z", _capi.ERR_BAD_ARG, lambda: step(h, *ctl(), None, 2, vp(R), vp(nrm))),
        ("null Z drawn", _capi.ERR_BAD_ARG, lambda: drawn(h, *ctl(), None, 2, vp(R), 4)),
        ("null normals", _capi.ERR_BAD_ARG, lambda: step(h, *ctl(), vp(Z2), 2, vp(R), None)),
        ("null normals, q = 0", _capi.ERR_BAD_ARG, lambda: step(h, *ctl(), None, 0, None, None)),
        ("sample_pose null normals", _capi.ERR_BAD_ARG, lambda: L.cslam_pf_sample_pose(h, None)),
    ]
    for name, code, call in cases:
        assert call() == code, name
        assert L.cslam_last_error().decode().strip(), name
        assert a.n_features == nf0 and a.stage_copies() == copies, name
    _assert_shards_bit_equal(a, twin, "refused calls")
    # ... and the same store takes the two features that fit: the last slot is written
    assert step(h, *ctl(), vp(Z2), 2, vp(R), vp(nrm)) == _capi.OK
    assert a.n_features == CAP and a.stage_copies() == copies + 1
    want = ref.new_feature_step(parts, dtype, nrm, Z2.reshape(2, 2, order="F"), R, predict=PREDICT, Q=Q)
    compare(a, want, dtype, "after the refusals", wtol=0.0)
    # q = 0 with neither Z nor R: [predict +] sample_pose
    assert step(twin._h, *ctl(), None, 0, None, vp(nrm)) == _capi.OK
    compare(twin, ref.new_feature_step(parts, dtype, nrm, predict=PREDICT, Q=Q), dtype, "q = 0", wtol=0.0)
    assert twin.n_features == nf0
    a.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 8. the loop from an empty map
def run_loop(sh, dtype):
    """The loop case of pf_new_feature_ref on a fresh shard (X = 0, Pv = 0, w = 1/np): two predicts, the all-new scan
    (step 2), two predicts, the mixed scan (step 5).  -> the records after scan 1."""
    controls, (ZN1,), (ZF, idf, ZN2) = ref.loop_inputs(dtype)
    Q, R = ref.LOOP_Q.astype(dtype), ref.LOOP_R.astype(dtype)
    none, noidf = np.zeros((2, 0), dtype, order="F"), np.zeros(0, np.int32)
    for v, swa in controls[:2]:
        sh.predict(v, swa, Q, ref.LOOP_WB, ref.LOOP_DT)
    sh.scan_step_drawn(*controls[2], Q, ref.LOOP_WB, ref.LOOP_DT, none, noidf, ZN1, R, 2, 0.0, True)
    after1 = _bulk_read(sh)
    for v, swa in controls[3:5]:
        sh.predict(v, swa, Q, ref.LOOP_WB, ref.LOOP_DT)
    sh.scan_step_drawn(*controls[5], Q, ref.LOOP_WB, ref.LOOP_DT, ZF, idf, ZN2, R, 5, 0.0, True)
    return after1


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_loop_from_an_empty_map(gpu_required, dtype):
    from conan_slam_amd.pf import ParticleShard

    sh = ParticleShard(ref.LOOP_NP, ref.LOOP_CAP, dtype=dtype)
    sh.seed_draws(ref.SEED)
    assert sh.n_features == 0
    normals1, _ = sh.draws(2, select=False)
    sh_after1 = run_loop(sh, dtype)
    # scan 1: the particles have left the common pose, each to its own, where the reference puts them
    X = sh_after1[:, 1:4].astype(np.float64)
    d = np.abs(X[:, None, :] - X[None, :, :]).max(axis=2) + np.eye(ref.LOOP_NP)
    assert d.min() > 1e-3, d.min()
    want, _, _, _ = ref.loop_reference(dtype, normals1)
    tol = TOL[np.dtype(dtype)]
    assert sh_after1.shape == (ref.LOOP_NP, 13 + 6 * 3)
    for i, p in enumerate(want):
        got = sh_after1[i].astype(np.float64)
        refrec = np.concatenate([[p[0]], p[1], p[2].reshape(-1, order="F"), p[3].reshape(-1, order="F"),
                                 p[4].reshape(-1, order="F")]).astype(np.float64)
        assert got[0] == refrec[0], i
        assert np.abs(got - refrec).max() <= tol * max(1.0, np.abs(refrec).max()), (i, np.abs(got - refrec).max())
    assert sh_after1[:, 4:13].tobytes() == np.zeros((ref.LOOP_NP, 9), dtype).tobytes()
    # scan 2: the known features were observed, the new one added
    assert sh.n_features == 4
    rec = _bulk_read(sh)
    w = rec[:, 0].astype(np.float64)
    assert np.all(np.isfinite(rec)) and np.all(w >= 0)
    assert abs(w.sum() - 1.0) <= 50 * tol, w.sum()
    assert rec[:, 4:13].tobytes() == np.zeros((ref.LOOP_NP, 9), dtype).tobytes()
    sh.close()
