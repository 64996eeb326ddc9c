"""The FastSLAM-2 particle kernels at the edges of their dispatch (conan_slam_amd/csrc/pf_kernels.hpp, cslam_pf.hip),
through the C ABI (conan_slam_amd.pf.ParticleShard), against the CPU oracle at the same dtype with the f64 oracle as the
high-precision reference.  The inputs come from pf_builders.py; test_pf_edges_cpu.py proves on the oracle alone that
every particle's weight stays in range (no particle is left out of a comparison here) and that the resample inputs are
exact, so that keep[] is compared bit for bit with nothing left to luck.  Each docstring names the branch it is for."""
import numpy as np
import pytest

from helpers import assert_close
from pf_builders import (DECISION_NP, DTYPES, FUSED_M, FUSED_NP, PREDICT, PROPOSAL_M, PROPOSAL_NP, RESAMPLE_END_NP,
                         RESAMPLE_NP, SHARDED, STAGING_M, STAGING_NF, STAGING_NP, TOL, TRUE_POSE, ExactResampleCase,
                         advance_pose, assert_weights_fair, compare, copy_parts, obs_for, oracle_chain, proposal_case,
                         random_particles, shard_from, tagged_records, tight_obs)
from pyoracle import Oracle, REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu


def _tol(dtype, m):
    """TOL of test_pf_gpu.py (2e-5 / 1e-12) at every m: the f64 chains of 16 to 65 sequential pose updates stayed two
    orders below 1e-12 on the device, so the wider helpers.P_RTOL is not called on."""
    return TOL[np.dtype(dtype)]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_shards_bit_equal(a, b, tag, skip_features=()):
    """Every particle of two shards, every field, bit for bit (columns of the listed 0-based features excepted)."""
    assert _same_bits(a.get_weights(), b.get_weights()), (tag, "weights")
    for i in range(a.n_local):
        pa, pb = a.get_particle(i), b.get_particle(i)
        assert _same_bits(pa[1], pb[1]) and _same_bits(pa[2], pb[2]), (tag, "pose", i)
        cols = np.setdiff1d(np.arange(pa[3].shape[1]), np.asarray(skip_features, dtype=int))
        assert _same_bits(pa[3][:, cols], pb[3][:, cols]) and _same_bits(pa[4][:, cols], pb[4][:, cols]), (tag, "map", i)


def _errs(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


def _compare_hi(sh, ref, hi, tol, tag):
    """Every particle's pose, pose covariance and map against the same-dtype oracle (`hi`: the f64 oracle)."""
    worst = 0.0
    for i, (p, h) in enumerate(zip(ref, hi)):
        _, gX, gP, gXF, gPF = sh.get_particle(i)
        worst = max(worst, _errs(gX, p[1]), _errs(gP, p[2]), _errs(gXF, p[3]), _errs(gPF, p[4]))
    print(f"[state] {tag}: largest error against the same-dtype oracle {worst:.3e} (tolerance {tol:.1e})")
    for i, (p, h) in enumerate(zip(ref, hi)):
        _, gX, gP, gXF, gPF = sh.get_particle(i)
        assert_close(f"{tag} Xv[{i}]", gX, p[1], tol, h[1])
        assert_close(f"{tag} Pv[{i}]", gP, p[2], tol, h[2])
        assert_close(f"{tag} XF[{i}]", gXF, p[3], tol, h[3])
        assert_close(f"{tag} PF[{i}]", gPF, p[4], tol, h[4])


def _weights(parts):
    return np.array([p[0] for p in parts], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ 1. proposal
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npart", PROPOSAL_NP)
@pytest.mark.parametrize("m", PROPOSAL_M)
def test_proposal_at_chunk_edges(gpu_required, m, npart, dtype):
    """pf_sample_proposal_kernel around its chunk of kObsChunk = kPfSubLanes = 8 observations: m = 8 (one full chunk),
    9 and 17 (a last chunk of ONE observation: the clamped index min(base + j, m - 1), sub-lanes beyond m whose factor
    must stay out of the product), 16 (two full chunks).  m > 8 takes the reload of the chunk in the likelihood loop
    (`if (m > kObsChunk)`) and forms the product from the shuffled factors of more than one chunk.  np = 1, 7, 8, 9, 17:
    a workgroup of 64 lanes holds 8 particles, so a partly filled one, exactly one, and more than one."""
    case = proposal_case((m, npart, None, False), dtype)
    sh = shard_from(case.parts, case.nf, dtype)
    sh.sample_proposal(case.Z, case.idf, case.R, case.normals)
    ref, hi = oracle_chain(case, dtype), oracle_chain(case, np.float64)
    tag = f"proposal m={m} np={npart}"
    assert_weights_fair(tag, sh.get_weights(), _weights(ref), _weights(hi), dtype)
    _compare_hi(sh, ref, hi, _tol(dtype, m), tag)
    for i, p0 in enumerate(case.parts):
        _, _, gP, gXF, gPF = sh.get_particle(i)
        assert not gP.any() and not ref[i][2].any(), (tag, "Pv is zeroed, PF.cpp:537", i)
        assert _same_bits(gXF, p0[3]) and _same_bits(gPF, p0[4]), (tag, "the proposal must not touch the map", i)
    sh.close()


# ------------------------------------------------------------------------------------------------ 2. staging
@pytest.mark.parametrize("dtype", DTYPES)
def test_staging_growth_on_one_shard(gpu_required, dtype):
    """cslam_pf.hip ensure_m / stage / off_idf() / off_normals(): the staging buffer starts at mcap = 64.  On ONE shard:
    sampleProposal + featureUpdate at m = 64 (fills it), at m = 65 (dObs and dIdx are reallocated, the idf and normals
    offsets move, the record of what is staged is dropped), at m = 8 (one chunk again, inside the grown buffer).  Also the
    proposal kernel at 8 and 9 chunks and pf_feature_update_kernel with grid.y = 65."""
    from conan_slam_amd.pf import ParticleShard

    sh = ParticleShard(STAGING_NP, STAGING_NF, dtype=dtype)
    for m in STAGING_M:
        case = proposal_case((m, STAGING_NP, STAGING_NF, False), dtype)
        for i, (w, Xv, Pv, XF, PF) in enumerate(case.parts):
            sh.set_particle(i, w, Xv, Pv, XF, PF)
        sh.sample_proposal(case.Z, case.idf, case.R, case.normals)
        sh.feature_update(case.Z, case.idf, case.R)
        ref = oracle_chain(case, dtype, feature_update=True)
        hi = oracle_chain(case, np.float64, feature_update=True)
        tag = f"staging m={m} np={STAGING_NP}"
        assert_weights_fair(tag, sh.get_weights(), _weights(ref), _weights(hi), dtype)
        _compare_hi(sh, ref, hi, _tol(dtype, m), tag)
        untouched = np.setdiff1d(np.arange(STAGING_NF), case.idf - 1)
        for i, p0 in enumerate(case.parts):
            _, _, _, gXF, gPF = sh.get_particle(i)
            assert _same_bits(gXF[:, untouched], p0[3][:, untouched]) and _same_bits(gPF[:, untouched], p0[4][:, untouched])
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_features_grows_the_staging_buffer(gpu_required, dtype):
    """cslam_pf.hip add_features -> stage(Z, q, nullptr) with q = 65 > mcap = 64 on a fresh shard (3 features, capacity
    68): ensure_m grows inside the call; pf_add_features_kernel with grid.y = 65 fills the store to its capacity."""
    o = Oracle(dtype)
    npart, nf0, q = 33, 3, 65
    parts = random_particles(npart, nf0, dtype, seed=71)
    sh = shard_from(parts, nf0 + q, dtype)
    rng = np.random.default_rng(72)
    Zn = np.asfortranarray(np.stack([rng.uniform(5.0, 300.0, q), rng.uniform(-3.1, 3.1, q)]).astype(dtype))
    R = np.diag([0.08, 0.0024]).astype(dtype)
    sh.add_features(Zn, R)
    assert sh.n_features == nf0 + q
    for p in parts:
        XF = np.zeros((2, nf0 + q), dtype=dtype, order="F")
        PF = np.zeros((4, nf0 + q), dtype=dtype, order="F")
        XF[:, :nf0], PF[:, :nf0] = p[3], p[4]
        assert o.pf_add_features(p[1], XF, PF, nf0, Zn, R) == nf0 + q
        p[3], p[4] = XF, PF
    compare(sh, parts, dtype, "add_features q=65", wtol=0.0)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("quirks", [REF_EXACT, TEXTBOOK])
def test_feature_update_alone_grows_the_staging_buffer(gpu_required, dtype, quirks):
    """cslam_pf.hip feature_update -> stage(Z, m, idf) with m = 65 on a fresh shard: the growth (and the new off_idf())
    happens in the call whose kernel reads the list; pf_feature_update_kernel with grid.y = 65."""
    case = proposal_case((65, STAGING_NP, STAGING_NF, False), dtype)
    sh = shard_from(case.parts, STAGING_NF, dtype, quirks)
    sh.feature_update(case.Z, case.idf, case.R)
    ref, hi = copy_parts(case.parts, dtype), copy_parts(case.parts, np.float64)
    for ps, dt in ((ref, dtype), (hi, np.float64)):
        o = Oracle(dt, quirks)
        for p in ps:
            o.pf_feature_update(p[1], p[3], p[4], np.asfortranarray(case.Z.astype(dt)), case.idf,
                                np.asfortranarray(case.R.astype(dt)))
    _compare_hi(sh, ref, hi, TOL[np.dtype(dtype)], f"feature_update m=65 quirks={quirks}")
    assert _same_bits(sh.get_weights(), np.array([p[0] for p in case.parts], dtype=dtype))
    sh.close()


# ------------------------------------------------------------------------------------------------ 3. fused step
def _separate_step(b, case, Z, idf, normals, sel, nmin):
    from conan_slam_amd.pf import SingleComm, resample_particles

    b.predict(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3])
    b.sample_proposal(Z, idf, case.R, normals)
    b.feature_update(Z, idf, case.R)
    return resample_particles(b, SingleComm(), nmin, True, select=sel)


def _fused_step(a, case, Z, idf, normals, sel, nmin):
    a.observation_step(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3], Z, idf, case.R, normals, sel, nmin, True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("quirks", [REF_EXACT, TEXTBOOK])
@pytest.mark.parametrize("m", FUSED_M)
def test_fused_step_beyond_one_chunk(gpu_required, m, quirks, dtype):
    """cslam_pf_observation_step with predict and the feature update inside pf_sample_proposal_kernel (pred.on,
    fu_mode 1 under REF_EXACT and fu_mode 2 under TEXTBOOK) at m = 9 and 17: the feature update of the second and third
    chunk uses the RELOADED features, and a sub-lane beyond m must store nothing (`base + sub < m`).  Step 0 does not
    resample and is compared with the oracle chain predict -> sampleProposal -> featureUpdate as well; steps 1 and 2
    resample.  All three steps must equal the separate calls bit for bit (same kernels, same inputs)."""
    from conan_slam_amd.pf import stratified_random

    case = proposal_case((m, FUSED_NP, None, True), dtype)
    npart = case.np_
    a = shard_from(case.parts, case.nf, dtype, quirks)
    b = shard_from(case.parts, case.nf, dtype, quirks)
    rng = np.random.default_rng(900 + m)
    sel = stratified_random(npart, rng.uniform(size=npart), dtype)
    _fused_step(a, case, case.Z, case.idf, case.normals, sel, 0)
    neff, did = _separate_step(b, case, case.Z, case.idf, case.normals, sel, 0)
    assert not did and np.isfinite(neff)
    tag = f"fused m={m} quirks={quirks}"
    _assert_shards_bit_equal(a, b, tag + " step 0")
    ref = oracle_chain(case, dtype, quirks, feature_update=True)
    hi = oracle_chain(case, np.float64, quirks, feature_update=True)
    _compare_hi(a, ref, hi, _tol(dtype, m), tag)
    wc, wh = _weights(ref), _weights(hi)
    assert_weights_fair(tag + " (normalised)", a.get_weights(), wc / wc.sum(), wh / wh.sum(), dtype)
    pose, n_res = advance_pose(TRUE_POSE, *PREDICT), 0
    for step in (1, 2):
        pose = advance_pose(pose, *PREDICT)
        idf = (rng.permutation(case.nf)[:m] + 1).astype(np.int32)
        Z = tight_obs(case.base, idf, dtype, seed=50 + step, pose=pose)
        nrm = rng.normal(size=(3, npart)).astype(dtype)
        sel = stratified_random(npart, rng.uniform(size=npart), dtype)
        _fused_step(a, case, Z, idf, nrm, sel, npart + 1)
        n_res += int(_separate_step(b, case, Z, idf, nrm, sel, npart + 1)[1])
        _assert_shards_bit_equal(a, b, f"{tag} step {step}")
    calls, resamples, _ = a.resample_stats()
    assert calls == 3 and resamples == n_res == 2, (calls, resamples, n_res)
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_without_observations(gpu_required, dtype):
    """cslam_pf_observation_step, the m = 0 leg: pf_predict_kernel, then the resample, with only select[] staged behind
    off_normals().  Must equal predict + resample_particles bit for bit (the resample is forced, so particles move)."""
    from conan_slam_amd.pf import SingleComm, resample_particles, stratified_random

    npart, nf = 70, 3
    parts = random_particles(npart, nf, dtype, seed=81)
    rng = np.random.default_rng(82)
    for p, wi in zip(parts, rng.uniform(0.0, 1.0, npart) ** 5):
        p[0] = dtype(wi)
    a, b = shard_from(parts, nf, dtype), shard_from(parts, nf, dtype)
    Q = np.diag([0.18, 6e-4]).astype(dtype)
    R = np.diag([0.08, 0.0024]).astype(dtype)
    sel = stratified_random(npart, rng.uniform(size=npart), dtype)
    nrm = rng.normal(size=(3, npart)).astype(dtype)
    a.observation_step(83.33, 0.03, Q, 73.0, 0.01, np.zeros((2, 0), dtype), np.zeros(0, np.int32), R, nrm, sel, npart + 1, True)
    b.predict(83.33, 0.03, Q, 73.0, 0.01)
    neff, did = resample_particles(b, SingleComm(), npart + 1, True, select=sel)
    assert did
    calls, resamples, last = a.resample_stats()
    assert (calls, resamples) == (1, 1) and last == neff
    _assert_shards_bit_equal(a, b, "fused m=0")
    # ... and the particles did move: the first slot's pose is some original particle's predicted pose, not always its own
    moved = sum(not _same_bits(a.get_particle(i)[3], parts[i][3]) for i in range(npart))
    assert moved > 0
    a.close()
    b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("quirks", [REF_EXACT, TEXTBOOK])
def test_fused_step_with_a_feature_named_twice(gpu_required, dtype, quirks):
    """cslam_pf_observation_step, the duplicate-feature fallback: idf names a feature twice (once in each chunk), so the
    proposal kernel runs with fu_mode = 0 and pf_feature_update_kernel follows.  The step must complete; weights and
    poses must equal predict + sampleProposal, every feature named once the separate featureUpdate, bit for bit.  (The
    feature named twice is left to the last writer on both paths and is not compared.)"""
    from conan_slam_amd.pf import stratified_random

    case = proposal_case((9, FUSED_NP, None, True), dtype)
    idf, Z = case.idf.copy(), case.Z.copy()
    idf[8] = idf[2]
    Z[:, 8] = Z[:, 2] + np.array([0.05, -0.002], dtype=dtype)
    a = shard_from(case.parts, case.nf, dtype, quirks)
    b = shard_from(case.parts, case.nf, dtype, quirks)
    sel = stratified_random(case.np_, np.random.default_rng(91).uniform(size=case.np_), dtype)
    _fused_step(a, case, Z, idf, case.normals, sel, 0)
    neff, did = _separate_step(b, case, Z, idf, case.normals, sel, 0)
    a.synchronize()
    assert not did and np.isfinite(neff) and neff > 1.0
    wa = a.get_weights()
    assert np.all(np.isfinite(wa)) and np.all(wa > 0)
    _assert_shards_bit_equal(a, b, "fused, duplicate feature", skip_features=[int(idf[2]) - 1])
    # the features named once did change, those not named at all did not
    once = np.setdiff1d(idf, [idf[2]]) - 1
    _, _, _, gXF, _ = a.get_particle(5)
    assert np.all(np.any(gXF[:, once] != case.parts[5][3][:, once], axis=0))
    rest = np.setdiff1d(np.arange(case.nf), idf - 1)
    assert _same_bits(gXF[:, rest], case.parts[5][3][:, rest])
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. launch edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npart", [1, 63, 64, 65])
def test_launch_edges_of_the_64_lane_kernels(gpu_required, npart, dtype):
    """pf_predict_kernel, pf_heading_kernel, pf_feature_update_kernel (m = 3) and pf_add_features_kernel (q = 2) with
    one particle, one lane short of a workgroup, exactly one workgroup and one lane into the second (`p >= s.np`); and
    observe_heading(..., False), which must return before any launch and leave pose and covariance bit-equal."""
    o = Oracle(dtype)
    nf = 4
    parts = random_particles(npart, nf, dtype, seed=100 + npart)
    sh = shard_from(parts, nf + 2, dtype)
    Q = np.diag([0.18, 6e-4]).astype(dtype)
    R = np.diag([0.08, 0.0024]).astype(dtype)
    sh.predict(83.33, 0.04, Q, 73.0, 0.01)
    for p in parts:
        o.pf_predict(p[1], p[2], 83.33, 0.04, Q, 73.0, 0.01)
    compare(sh, parts, dtype, f"predict np={npart}", wtol=0.0)
    before = [sh.get_particle(i) for i in range(npart)]
    sh.observe_heading(0.25, False)
    sh.synchronize()
    for i in range(npart):
        for x, y in zip(sh.get_particle(i), before[i]):
            assert _same_bits(np.asarray(x), np.asarray(y)), ("observe_heading(False) changed particle", i)
    sh.observe_heading(0.25, True)
    for p in parts:
        o.pf_observe_heading(p[1], p[2], 0.25, True)
    ptol = 2e-3 if dtype == np.float32 else 1e-9  # 1 - W[2] cancellation, as in test_pf_gpu.test_predict_and_heading
    for i, p in enumerate(parts):
        _, gX, gP, _, _ = sh.get_particle(i)
        assert_close(f"heading Xv np={npart}", gX, p[1], TOL[np.dtype(dtype)])
        assert_close(f"heading Pv np={npart}", gP, p[2], ptol)
        p[1], p[2] = gX.copy(), gP.copy()  # (the next steps start from the engine's own pose on both sides)
    idf = np.array([4, 1, 3], dtype=np.int32)
    Z = obs_for(parts, idf, dtype, seed=13)
    sh.feature_update(Z, idf, R)
    for p in parts:
        o.pf_feature_update(p[1], p[3], p[4], Z, idf, R)
    compare(sh, parts, dtype, f"feature_update np={npart}", wtol=0.0)
    Zn = np.asfortranarray(np.array([[120.0, 45.0], [0.3, 2.0]], dtype=dtype))
    sh.add_features(Zn, R)
    assert sh.n_features == nf + 2
    for p in parts:
        XF = np.zeros((2, nf + 2), dtype=dtype, order="F")
        PF = np.zeros((4, nf + 2), dtype=dtype, order="F")
        XF[:, :nf], PF[:, :nf] = p[3], p[4]
        assert o.pf_add_features(p[1], XF, PF, nf, Zn, R) == nf + 2
        p[3], p[4] = XF, PF
    compare(sh, parts, dtype, f"add_features np={npart}", wtol=0.0)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_features_fills_an_empty_map_to_capacity(gpu_required, dtype):
    """cslam_pf.hip add_features from nf = 0 with q = nfcap (pf_add_features_kernel writes the whole xf / pf store, the
    last feature at the far end of its strides), then one more: ERR_CAPACITY before anything is staged or launched, the
    store and n_features unchanged."""
    from conan_slam_amd import CslamError, _capi
    from conan_slam_amd.pf import ParticleShard

    o = Oracle(dtype)
    npart, cap = 65, 5
    parts = [[p[0], p[1], p[2], np.zeros((2, 0), dtype, order="F"), np.zeros((4, 0), dtype, order="F")]
             for p in random_particles(npart, 1, dtype, seed=111)]
    sh = ParticleShard(npart, cap, dtype=dtype)
    for i, (w, Xv, Pv, XF, PF) in enumerate(parts):
        sh.set_particle(i, w, Xv, Pv, XF, PF)
    assert sh.n_features == 0
    rng = np.random.default_rng(112)
    Zn = np.asfortranarray(np.stack([rng.uniform(5.0, 300.0, cap), rng.uniform(-3.1, 3.1, cap)]).astype(dtype))
    R = np.diag([0.08, 0.0024]).astype(dtype)
    sh.add_features(Zn, R)
    assert sh.n_features == cap
    for p in parts:
        XF = np.zeros((2, cap), dtype=dtype, order="F")
        PF = np.zeros((4, cap), dtype=dtype, order="F")
        assert o.pf_add_features(p[1], XF, PF, 0, Zn, R) == cap
        p[3], p[4] = XF, PF
    compare(sh, parts, dtype, "add_features to capacity", wtol=0.0)
    before = [sh.get_particle(i) for i in range(npart)]
    with pytest.raises(CslamError) as ei:
        sh.add_features(Zn[:, :1], R)
    assert ei.value.code == _capi.ERR_CAPACITY
    assert sh.n_features == cap
    for i in range(npart):
        for x, y in zip(sh.get_particle(i), before[i]):
            assert _same_bits(np.asarray(x), np.asarray(y)), i
    sh.close()


# ------------------------------------------------------------------------------------------------ 5. resample plan
def _bulk_shard(rec, dtype, nf=1):
    """A shard holding the packed records `rec`: one set_particle fixes the feature count, one unpack fills the rest
    (setting 16 000 particles one by one costs seconds)."""
    import torch

    from conan_slam_amd.pf import ParticleShard

    n = rec.shape[0]
    sh = ParticleShard(n, nf, dtype=dtype)
    sh.set_particle(0, rec[0, 0], rec[0, 1:4], rec[0, 4:13].reshape(3, 3, order="F"),
                    rec[0, 13:13 + 2 * nf].reshape(2, nf, order="F"), rec[0, 13 + 2 * nf:].reshape(4, nf, order="F"))
    sh.unpack(np.arange(n, dtype=np.int32), torch.from_numpy(np.ascontiguousarray(rec)).cuda())
    for i in {0, n // 2, n - 1}:  # the plain reader sees what was unpacked
        w, Xv, Pv, XF, PF = sh.get_particle(i)
        got = np.concatenate([[w], Xv, Pv.reshape(-1, order="F"), XF.reshape(-1, order="F"), PF.reshape(-1, order="F")])
        assert _same_bits(got.astype(dtype), rec[i]), i
    return sh


def _bulk_read(sh):
    return sh.pack(np.arange(sh.n_local, dtype=np.int32)).cpu().numpy()


def _assert_kept(got, rec, keep, n_total, dtype, tag):
    """Slot c holds a bit-exact copy of particle keep[c] (every particle carries its index in xv[0]); w = 1/N."""
    kept = got[:, 1].astype(np.int64)
    bad = np.nonzero(kept != keep)[0]
    assert bad.size == 0, (tag, f"{bad.size} slots differ; first: slot {bad[0]} holds {kept[bad[0]]}, keep = {keep[bad[0]]}")
    assert _same_bits(got[:, 1:], rec[keep, 1:]), tag
    assert np.all(got[:, 0] == dtype(1.0 / n_total)), tag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", [(n, False) for n in RESAMPLE_NP] + [(n, True) for n in RESAMPLE_END_NP],
                         ids=lambda k: f"np{k[0]}-{'end' if k[1] else 'in'}")
def test_resample_plan_edges_on_exact_inputs(gpu_required, key, dtype):
    """pf_resample_plan_kernel on exact inputs (pf_builders.ExactResampleCase): pf_running_sum with its first element,
    its loop unrolled by 8 and its scalar tail (np = 1, 2, 8, 9, 10), the 256-lane strides (255, 256, 257), one full LDS
    stage and the start of the next (8192, 8193), a later stage that is ONLY a scalar tail (8199 = 8192 + 7,
    16389 = 2 * 8192 + 5); pf_first_above in LDS (np <= 8192) and the global-memory search beyond it, with the strict
    `select < cum` decided on ties select[c] == cum[i]; `end`: a position of 1.0, not below cum[np-1], and trailing zero
    weights (`lo < np ? lo : 0`).  The device plan (cslam_pf_resample_local) and the host-planned path (weight_sums,
    scale_weights, stratified_keep, gather_local) must both reproduce the oracle's keep[] in EVERY slot."""
    from conan_slam_amd.pf import SingleComm, resample_particles

    n, end = key
    case = ExactResampleCase(n, end=end)
    w_raw, sel = case.raw_weights(dtype), case.select(dtype)
    rec = tagged_records(n, w_raw, dtype)
    w_o = w_raw.copy()
    _, did_o, keep = Oracle(dtype).pf_normalize_resample(w_o, n + 1, True, sel)
    assert did_o and np.array_equal(keep, case.keep) and np.all(w_o == dtype(1.0 / n))
    for host in (False, True):
        tag = f"{case} {'host-planned' if host else 'device plan'}"
        sh = _bulk_shard(rec, dtype)
        sh.host_resample = host
        neff, did = resample_particles(sh, SingleComm(), n + 1, True, select=sel)
        assert did, tag
        assert abs(neff - case.neff) <= 1e-12 * case.neff, (tag, neff, case.neff)
        got = _bulk_read(sh)
        _assert_kept(got, rec, keep, n, dtype, tag)
        assert _same_bits(sh.get_weights(), got[:, 0].copy())
        for c in {0, n - 1, min(n - 1, 8192)}:
            assert sh.get_particle(c)[1][0] == dtype(keep[c]), (tag, c)
        sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", DECISION_NP)
def test_resample_decision_edge(gpu_required, n, dtype):
    """pf_resample_plan_kernel `neff < n_effective` (PF.cpp:490) and the same comparison of the host-planned path, at
    the edge: uniform exact weights give Neff = np exactly (powers of two, so 1/np is exact as well), hence
    n_effective = np must only normalise and n_effective = np + 1 must resample."""
    from conan_slam_amd.pf import SingleComm, resample_particles

    case = ExactResampleCase(n, uniform=True)
    rec = tagged_records(n, case.raw_weights(dtype), dtype)
    for host in (False, True):
        for nmin, expect in ((n, False), (n + 1, True)):
            sh = _bulk_shard(rec, dtype)
            sh.host_resample = host
            neff, did = resample_particles(sh, SingleComm(), nmin, True, select=case.select(dtype))
            assert neff == float(n) and did == expect, (host, nmin, neff, did)
            got = _bulk_read(sh)
            assert np.all(got[:, 0] == dtype(1.0 / n)), (host, nmin)  # w / sum = 1/np, and 1/np after a resample
            assert _same_bits(got[:, 1:], rec[:, 1:]), (host, nmin)    # keep[] is the identity on these weights
            if not host:
                assert sh.resample_stats()[:2] == (1, int(expect))
            sh.close()


# ------------------------------------------------------------------------------------------------ 6. sharded plan
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("world,N", SHARDED)
def test_sharded_plan_above_one_lds_stage(gpu_required, world, N, dtype):
    """pf_keep_kernel (cslam_pf_resample_sharded) at N = 8192 -- the largest set searched in LDS -- and N = 16400, which
    runs pf_running_sum over three stages and the kernel's own global-memory search, over loopback worlds of 2 and 4 on
    exact inputs: the concatenated shards must be the oracle's keep[] bit for bit, and every rank's device-side exchange
    plan (pf_exchange_plan_kernel) the host planner's."""
    from conan_slam_amd.pf import LoopbackComm, plan_exchange
    from test_pf_gpu import _run_ranks

    case = ExactResampleCase(N)
    L = N // world
    assert L * world == N
    w_raw, sel = case.raw_weights(dtype), case.select(dtype)
    rec = tagged_records(N, w_raw, dtype)
    w_o = w_raw.copy()
    _, did_o, keep = Oracle(dtype).pf_normalize_resample(w_o, N + 1, True, sel)
    assert did_o and np.array_equal(keep, case.keep)
    shards = [_bulk_shard(rec[r * L:(r + 1) * L], dtype) for r in range(world)]
    comms = LoopbackComm.create(world)
    res = _run_ranks([(lambda r=r: shards[r].resample_sharded(comms[r], sel, N + 1, True)) for r in range(world)])
    for r in range(world):
        assert res[r][1] and abs(res[r][0] - case.neff) <= 1e-12 * case.neff, (r, res[r], case.neff)
    got = np.concatenate([_bulk_read(sh) for sh in shards])
    _assert_kept(got, rec, keep, N, dtype, f"{case} world={world}")
    for r in range(world):
        send_c, recv_c, send_idx = shards[r].debug_last_exchange(world)
        src_l, sc, _, rc_ = plan_exchange(np.asarray(keep), r, world, L)
        assert send_c == sc and recv_c == rc_, (r, send_c, sc, recv_c, rc_)
        assert np.array_equal(send_idx, src_l), r
    for c in comms:
        c.close()
    for sh in shards:
        sh.close()


# ------------------------------------------------------------------------------------------------ 7. records
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf", [40, 41])
def test_records_around_256_scalars_and_a_growing_index_list(gpu_required, nf, dtype):
    """pf_pack_kernel / pf_unpack_kernel with a record of 13 + 6 nf = 253 and 259 scalars (the 256-thread stride over the
    record takes a second trip for 3 of them), and cslam_pf.hip stage_idx with count = 1, then 70 (more than the 64-entry
    index buffer of a 20-particle shard: ensure_m reallocates dIdx), then 200 (a second growth), with repeated sources.
    Every record must be the source particle bit for bit, and land bit for bit in the slot it is unpacked to."""
    npart = 20
    parts = random_particles(npart, nf, dtype, seed=120 + nf)
    a = shard_from(parts, nf, dtype)
    b = shard_from(random_particles(npart, nf, dtype, seed=7), nf, dtype)
    assert a.record_len == 13 + 6 * nf
    src_parts = [a.get_particle(i) for i in range(npart)]
    rng = np.random.default_rng(121)
    for count in (1, 70, 200):
        src = rng.integers(0, npart, count).astype(np.int32)
        if count > 1:
            src[1] = src[0]
            assert len(set(src.tolist())) < count
        buf = a.pack(src)
        assert tuple(buf.shape) == (count, 13 + 6 * nf)
        host = buf.cpu().numpy()
        for j, s in enumerate(src):
            w, Xv, Pv, XF, PF = src_parts[s]
            want = np.concatenate([[w], Xv, Pv.reshape(-1, order="F"), XF.reshape(-1, order="F"), PF.reshape(-1, order="F")])
            assert _same_bits(host[j], want.astype(dtype)), (count, j, int(s))
        perm = rng.permutation(npart)
        dst = perm[src].astype(np.int32)  # a source always goes to the same slot: repeated records carry the same values
        before = [b.get_particle(i) for i in range(npart)]
        b.unpack(dst, buf)
        hit = set(dst.tolist())
        inv = {int(perm[s]): int(s) for s in src}
        for d in range(npart):
            want = src_parts[inv[d]] if d in hit else before[d]
            for x, y in zip(b.get_particle(d), want):
                assert _same_bits(np.asarray(x), np.asarray(y)), (count, d)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 8. staging ring
@pytest.mark.parametrize("dtype", DTYPES)
def test_staging_ring_round_a_lap_and_grown_inside_one(gpu_required, dtype):
    """The pinned staging ring of cslam_pf.hip (16 slots of 4096 bytes at first) taken round a lap and reallocated in the
    middle of one, on two shards A and B from one case (np = 300, nf = 4).  20 feature updates at m = 3 whose Z
    alternates between two sets, so that every call stages a copy: slots 0..15, then 0..3 again (a slot is reused behind
    its event, not behind a drained stream).  Then 20 observation steps (host arrays) at m = 3: Z | idf | normals |
    select of 300 particles is more than 4096 bytes, so the first of them reallocates the ring at position 4 of its second
    lap, and the rest take the new ring round once more.  A queues everything back to back, B synchronises after every
    call: every array must agree bit for bit, and each of the 40 calls must have enqueued exactly one copy."""
    from conan_slam_amd.pf import stratified_random

    npart, nf, m = 300, 4, 3
    case = proposal_case((m, npart, nf, True), dtype)
    assert (2 * 64 + 4 * npart) * np.dtype(dtype).itemsize + 64 * 4 > 4096  # the whole step does not fit the first slots
    shards = [shard_from(case.parts, nf, dtype) for _ in range(2)]
    rng = np.random.default_rng(310)
    Zs = [case.Z, tight_obs(case.base, case.idf, dtype, seed=311)]
    assert not _same_bits(Zs[0], Zs[1])
    pose, steps = TRUE_POSE, []
    for t in range(20):
        pose = advance_pose(pose, *PREDICT)
        idf = (rng.permutation(nf)[:m] + 1).astype(np.int32)
        steps.append((tight_obs(case.base, idf, dtype, seed=320 + t, pose=pose), idf,
                      rng.normal(size=(3, npart)).astype(dtype), stratified_random(npart, rng.uniform(size=npart), dtype)))
    for sh, sync in zip(shards, (False, True)):
        copies = sh.stage_copies()
        for t in range(20):
            sh.feature_update(Zs[t % 2], case.idf, case.R)
            if sync:
                sh.synchronize()
        assert sh.stage_copies() - copies == 20
        for Z, idf, nrm, sel in steps:
            _fused_step(sh, case, Z, idf, nrm, sel, npart + 1)
            if sync:
                sh.synchronize()
        assert sh.stage_copies() - copies == 40
    a, b = shards
    calls, resamples, neff = a.resample_stats()
    assert (calls, resamples) == (20, 20) and np.isfinite(neff)
    assert np.all(np.isfinite(a.get_weights()))
    _assert_shards_bit_equal(a, b, "staging ring, back to back against synchronised")
    a.close()
    b.close()
