"""The particle filter's random inputs drawn on the device (conan_slam_amd/csrc/pf_draw_kernels.hpp, the *_drawn calls of
include/cslam.h) through conan_slam_amd.pf.ParticleShard.

Two kinds of statement.  The DRAWS are those conan_slam_amd/synth.py restates (pf_draw_normals, pf_draw_select): select
bit for bit, the normals to the device's log / cos.  The CONSUMPTION is the host-array path bit for bit: a *_drawn call
on one shard against its twin call on a second shard that is handed the first one's read-back draws -- same consumer
kernels, same inputs, so every weight, pose, covariance and feature must come out identical."""
import numpy as np
import pytest

from conan_slam_amd import synth
from pf_builders import (DTYPES, PREDICT, TRUE_POSE, ProposalCase, advance_pose, random_particles, shard_from, tight_obs)
from pyoracle import REF_EXACT, TEXTBOOK
from test_pf_edges_gpu import _assert_shards_bit_equal, _bulk_read, _bulk_shard, _same_bits

pytestmark = pytest.mark.gpu

SEED = 20240607
BIG_STEP = 2**31 + 5  # (step * 4 + e) << 32 has left uint64: the key wraps on the device as it does in numpy

# Largest deviation of the device's f64 normals from synth.normal over the draws of test_draws_against_the_restatement,
# in f64 ulps, as first measured on an MI355X (2 ulp, 294 of the 6948 f64 entries not bitwise equal; every f32
# entry bitwise equal); the test allows four times that: the device's log and cos against glibc's, each good to about an ulp.
F64_NORMAL_ULPS_MEASURED = 2.0


def _shard(npart, dtype, nf=1):
    from conan_slam_amd.pf import ParticleShard

    return ParticleShard(npart, nf, dtype=dtype)


def _bad_arg(fn):
    from conan_slam_amd import CslamError, _capi

    with pytest.raises(CslamError) as ei:
        fn()
    assert ei.value.code == _capi.ERR_BAD_ARG and str(ei.value).strip()


# ------------------------------------------------------------------------------------------------ 1. the draws
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npart", [1, 63, 65, 257])
def test_draws_against_the_restatement(gpu_required, npart, dtype):
    """pf_stage_draw_kernel alone (cslam_pf_get_draws): one lane, a partial block, two blocks (257); slots that start at
    0 and at 1000; a step whose key wraps.  n_global is first + np + 7: more strata than particles, so the select lanes
    run past the normal lanes.  The handle is re-seeded for every case."""
    sh = _shard(npart, dtype)
    worst_ulp, differ, total = 0.0, 0, 0
    for first in (0, 1000):
        n_global = first + npart + 7
        sh.seed_draws(SEED, first, n_global)
        for step in (0, 1, BIG_STEP):
            nrm, sel = sh.draws(step)
            assert _same_bits(sel, synth.pf_draw_select(SEED, step, n_global, dtype)), (first, step)
            ref = synth.pf_draw_normals(SEED, step, first, npart, dtype)
            assert nrm.shape == ref.shape and np.all(np.isfinite(nrm))
            ulp = np.abs(nrm.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
            worst_ulp = max(worst_ulp, float(ulp.max()))
            differ += int((nrm.view(np.uint8).reshape(nrm.size, -1) != ref.view(np.uint8).reshape(ref.size, -1)).any(axis=1).sum())
            total += nrm.size
            # only one of the two asked for: the other is left alone, the bits are the same
            only_n, none = sh.draws(step, select=False)
            none2, only_s = sh.draws(step, normals=False)
            assert none is None and none2 is None and _same_bits(only_n, nrm) and _same_bits(only_s, sel)
    print(f"[draws] np={npart} {np.dtype(dtype).name}: normals off the restatement by at most {worst_ulp:.2f} ulp, "
          f"{differ} of {total} not bitwise equal")
    if np.dtype(dtype) == np.float32:
        assert worst_ulp <= 1.0
        assert differ <= 0.01 * total
    else:
        assert F64_NORMAL_ULPS_MEASURED is not None, "record the first measured figure (see the constant's comment)"
        assert worst_ulp <= 4.0 * F64_NORMAL_ULPS_MEASURED
    sh.close()


def test_seed_arguments(gpu_required):
    sh = _shard(8, np.float32)
    for first, n_global in ((-1, 8), (1, 8), (0, 7), (0, 2**32), (2**32 - 4, 2**32 + 4), (2**63 - 1, 100)):
        _bad_arg(lambda: sh.seed_draws(1, first, n_global))
    _bad_arg(lambda: sh.draws(0))  # none of the refused calls seeded it
    # a set beyond what one resample holds (2^31 - 1) draws its normals -- the keys reach every slot below 2^32 -- and
    # has no strata
    sh.seed_draws(1, 2**32 - 9, 2**32 - 1)
    nrm, _ = sh.draws(4, select=False)
    assert _same_bits(nrm, synth.pf_draw_normals(1, 4, 2**32 - 9, 8, np.float32))
    _bad_arg(lambda: sh.draws(4))
    sh.seed_draws(1, 3, 11)
    sh.seed_draws(2)               # again, with the defaults: slots 0.. of the shard's own n_global
    nrm, sel = sh.draws(4)
    assert sel.shape == (8,) and _same_bits(nrm, synth.pf_draw_normals(2, 4, 0, 8, np.float32))
    sh.close()


# ------------------------------------------------------------------------------------------------ 2. the proposal
PROPOSAL_M = [1, 8, 9, 32, 33]  # 8 / 9: the proposal's observation chunk; 32 / 33: kernel arguments / the staged copy
PROPOSAL_NP = [1, 65]
PROPOSAL_NF = 40


def _proposal_case(m, npart, dtype, predict=False):
    if m >= 2:
        return ProposalCase(m, npart, dtype, nf=PROPOSAL_NF, predict=predict)
    case = ProposalCase(2, npart, dtype, nf=PROPOSAL_NF, predict=predict)  # (the builder wants two observations)
    case.m, case.idf, case.Z = m, case.idf[:m].copy(), np.asfortranarray(case.Z[:, :m])
    return case


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npart", PROPOSAL_NP)
@pytest.mark.parametrize("m", PROPOSAL_M)
def test_proposal_consumes_the_draws_as_the_host_array_path(gpu_required, m, npart, dtype):
    """cslam_pf_sample_proposal_drawn on A against cslam_pf_sample_proposal(normals = A.draws(step)) on its twin B, then
    cslam_pf_feature_update on both (on A its Z | idf are those the producer kernel wrote -- or, at m = 33, the staged
    copy -- and the call sends nothing).  REF_EXACT on one half of the (m, np) grid, TEXTBOOK on the other."""
    quirks = REF_EXACT if (PROPOSAL_M.index(m) + PROPOSAL_NP.index(npart)) % 2 == 0 else TEXTBOOK
    case = _proposal_case(m, npart, dtype)
    a = shard_from(case.parts, case.nf, dtype, quirks)
    b = shard_from(case.parts, case.nf, dtype, quirks)
    a.seed_draws(SEED + m)
    step = 3
    normals, _ = a.draws(step)
    assert _same_bits(normals, a.draws(step)[0])
    w0 = a.get_weights()
    copies = a.stage_copies()
    a.sample_proposal_drawn(case.Z, case.idf, case.R, step)
    b.sample_proposal(case.Z, case.idf, case.R, normals)
    tag = f"drawn proposal m={m} np={npart} quirks={quirks}"
    _assert_shards_bit_equal(a, b, tag)
    assert np.all(np.isfinite(a.get_weights())) and not _same_bits(a.get_weights(), w0)
    a.feature_update(case.Z, case.idf, case.R)
    b.feature_update(case.Z, case.idf, case.R)
    _assert_shards_bit_equal(a, b, tag + " + feature update")
    assert a.stage_copies() - copies == (1 if m > 32 else 0)
    # other observations behind the same staging area: nothing of the previous call is taken for them
    idf2 = np.roll(case.idf, 1) if m > 1 else np.array([case.idf[0] % case.nf + 1], np.int32)
    Z2 = tight_obs(case.base, idf2, dtype, seed=5)
    a.feature_update(Z2, idf2, case.R)
    b.feature_update(Z2, idf2, case.R)
    _assert_shards_bit_equal(a, b, tag + " + another feature update")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3. the fused step
def _step_inputs(case, m, t, dup, rng, dtype, avoid=()):
    pose = TRUE_POSE
    for _ in range(t + 1):
        pose = advance_pose(pose, *PREDICT)
    if m == 0:
        return np.zeros((2, 0), dtype, order="F"), np.zeros(0, np.int32)
    free = np.setdiff1d(np.arange(case.nf), np.asarray(avoid, dtype=int))
    idf = (rng.permutation(free)[:m] + 1).astype(np.int32)
    Z = tight_obs(case.base, idf, dtype, seed=50 + t, pose=pose)
    if dup:
        idf[m - 1] = idf[2]
        Z[:, m - 1] = Z[:, 2] + np.array([0.05, -0.002], dtype=dtype)
    return Z, idf


def _restore_covariances(shards, parts):
    """Between two steps of a multi-step comparison: every particle keeps its weight, pose and feature means and gets
    the Pv and PF it started with, on every handle alike (cslam_pf_set_particle: the handles and their staging state
    stay).  The reference's sampleProposal leaves Pv = 0 (PF.cpp:502-544), so without this the next step's prior is
    evaluated on the rank-2 covariance that predict adds and the weights stop being finite: a forced resample would
    then resample nothing.  Every value read on the way must be finite."""
    for sh in shards:
        for i, p in enumerate(parts):
            w, Xv, _, XF, _ = sh.get_particle(i)
            assert np.isfinite(w) and np.all(np.isfinite(Xv)) and np.all(np.isfinite(XF)), i
            sh.set_particle(i, w, Xv, p[2], XF, p[4])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("force", [True, False], ids=["resample", "never"])
@pytest.mark.parametrize("m,dup", [(0, False), (8, False), (33, False), (9, True)], ids=["m0", "m8", "m33", "m9-dup"])
def test_fused_step_drawn(gpu_required, m, dup, force, dtype):
    """cslam_pf_observation_step_drawn on A against cslam_pf_observation_step fed with A's read-back draws on B, three
    consecutive steps: m = 0 (predict + resample, select alone is drawn), m = 8 (kernel arguments), m = 33 (the staged
    copy of Z | idf, the draws behind it), and a list that names a feature twice (the separate feature update).  On a
    third shard C, predict + sample_proposal_drawn + feature_update + resample_local_drawn of the same step.
    Every step runs on a healthy set (_restore_covariances): every weight, pose and feature is finite after every step,
    and a forced resample happens at every one of the three steps, each with its own step's strata.  A feature named
    twice is left to the last writer: it is not compared, and no later step observes it."""
    npart = 65
    case = ProposalCase(max(m, 2), npart, dtype, nf=PROPOSAL_NF, predict=True)
    quirks = REF_EXACT if force else TEXTBOOK
    a, b, c = (shard_from(case.parts, case.nf, dtype, quirks) for _ in range(3))
    a.seed_draws(SEED)
    c.seed_draws(SEED)
    nmin = npart + 1 if force else 0
    rng = np.random.default_rng(300 + m)
    skip, selects = [], []
    for t in range(3):
        step = 10 + t
        Z, idf = _step_inputs(case, m, t, dup, rng, dtype, avoid=skip)
        normals, select = a.draws(step)
        selects.append(select)
        a.observation_step_drawn(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3], Z, idf, case.R, step, nmin, True)
        b.observation_step(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3], Z, idf, case.R, normals, select, nmin, True)
        c.predict(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3])
        if m > 0:  # (without observations the fused step does not sample the proposal at all)
            c.sample_proposal_drawn(Z, idf, case.R, step)
            c.feature_update(Z, idf, case.R)
        neff, did = c.resample_local_drawn(step, nmin, True)
        assert np.isfinite(neff) and 1.0 <= neff <= npart * (1 + 1e-6) and did == force, (t, neff, did)
        wa = a.get_weights()
        assert np.all(np.isfinite(wa)) and np.all(wa >= 0) and abs(float(wa.astype(np.float64).sum()) - 1.0) < 1e-3, t
        assert a.resample_stats()[:2] == (t + 1, t + 1 if force else 0), t
        tag = f"drawn step {t} m={m} dup={dup} force={force}"
        if dup:
            skip.append(int(idf[2]) - 1)
        _assert_shards_bit_equal(a, b, tag, skip_features=skip)
        _assert_shards_bit_equal(a, c, tag + " (separate calls)", skip_features=skip)
        _restore_covariances((a, b, c), case.parts)
    assert not _same_bits(selects[0], selects[1]) and not _same_bits(selects[1], selects[2])
    sa, sb, sc = a.resample_stats(), b.resample_stats(), c.resample_stats()
    assert sa[:2] == sb[:2] == sc[:2] == (3, 3 if force else 0)
    for sh in (a, b, c):
        sh.close()


def _cloud_records(n, dtype, seed):
    """n packed records [w, xv, pv, xf, pf] of a tight cloud with ONE feature at (50, 30), weights that differ."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 19), np.float64)
    rec[:, 0] = rng.uniform(0.5, 1.5, n) / n
    rec[:, 1:4] = rng.normal(0.0, 1.0, (n, 3)) * np.array([0.3, 0.3, 0.006]) + np.array(TRUE_POSE)
    rec[:, 4], rec[:, 8], rec[:, 12] = 0.05, 0.05, 1e-4
    rec[:, 13:15] = np.array([50.0, 30.0]) + rng.normal(0.0, 0.3, (n, 2))
    rec[:, 15], rec[:, 18] = 0.3, 0.3
    return rec.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_step_drawn_beyond_one_lds_stage(gpu_required, dtype):
    """8193 particles -- one past the 8192 weights pf_resample_plan_kernel stages in LDS, 33 blocks of the producer
    kernel -- with one feature: three forced resamples, every one of which happens, on a set that is finite after every
    step (between steps the records go back with the Pv and PF they started with, one unpack per handle)."""
    import torch

    n = 8193
    rec = _cloud_records(n, dtype, 17)
    a, b = _bulk_shard(rec, dtype), _bulk_shard(rec, dtype)
    a.seed_draws(SEED)
    Q = np.diag([0.18, 6e-4]).astype(dtype)
    R = np.diag([0.08, 0.0024]).astype(dtype)
    idf = np.array([1], np.int32)
    pose = TRUE_POSE
    slots = np.arange(n, dtype=np.int32)
    for t in range(3):
        pose = advance_pose(pose, *PREDICT)
        Z = tight_obs(np.array([[50.0], [30.0]]), idf, dtype, seed=70 + t, pose=pose)
        normals, select = a.draws(t)
        assert _same_bits(select, synth.pf_draw_select(SEED, t, n, dtype))
        a.observation_step_drawn(PREDICT[0], PREDICT[1], Q, PREDICT[2], PREDICT[3], Z, idf, R, t, n + 1, True)
        b.observation_step(PREDICT[0], PREDICT[1], Q, PREDICT[2], PREDICT[3], Z, idf, R, normals, select, n + 1, True)
        ra, rb = _bulk_read(a), _bulk_read(b)
        assert np.all(np.isfinite(ra)) and _same_bits(ra, rb), t
        assert np.all(ra[:, 0] == dtype(1.0 / n)), t  # it resampled
        calls, resamples, neff = a.resample_stats()
        assert (calls, resamples) == (t + 1, t + 1) and np.isfinite(neff) and 1.0 <= neff < n, (t, calls, resamples, neff)
        assert b.resample_stats()[:2] == (t + 1, t + 1)
        ra[:, 4:13], ra[:, 15:19] = rec[:, 4:13], rec[:, 15:19]
        for sh in (a, b):
            sh.unpack(slots, torch.from_numpy(np.ascontiguousarray(ra)).cuda())
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. the association
@pytest.mark.parametrize("key", [0, 1], ids=["float32", "float64"])
def test_association_consumer_drawn(gpu_required, key):
    """cslam_pf_sample_proposal_assoc_drawn against cslam_pf_sample_proposal_assoc with the read-back normals, on a
    per-particle table that is neither empty nor complete and a mask with holes; refused after a resample, as the twin."""
    import pf_assoc_ref as ref
    from test_pf_assoc_gpu import MISS, upload

    case = ref.get_case(ref.MIXED_KEYS[key])
    dt = case.dtype.type
    a, b = upload(case), upload(case)
    use = np.ones(case.m, np.int32)
    use[1::4] = 0
    for sh in (a, b):
        sh.predict(PREDICT[0], PREDICT[1], np.diag([0.18, 6e-4]), PREDICT[2], PREDICT[3])
        sh.associate(case.Z, case.R, *case.gates[0])
    idf, _, _ = a.association()
    assert (idf == 0).any() and (idf != 0).any(), case
    a.seed_draws(SEED)
    normals, _ = a.draws(7)
    a.sample_proposal_assoc_drawn(case.Z, case.R, 7, use, MISS)
    b.sample_proposal_assoc(case.Z, case.R, normals, use, MISS)
    _assert_shards_bit_equal(a, b, f"drawn association consumer {case}")
    assert not _same_bits(a.get_weights(), np.asarray(case.w, dt))
    # the table is per slot: after a resample the drawn consumer refuses it, and a refused call changes nothing
    a.resample_local_drawn(7, case.np_ + 1, True)
    b.resample_local(a.draws(7)[1], case.np_ + 1, True)
    _bad_arg(lambda: a.sample_proposal_assoc_drawn(case.Z, case.R, 8, use, MISS))
    _bad_arg(lambda: b.sample_proposal_assoc(case.Z, case.R, normals, use, MISS))
    _assert_shards_bit_equal(a, b, f"after the refused consumer {case}")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. sharded
@pytest.mark.parametrize("dtype", DTYPES)
def test_sharded_resample_drawn(gpu_required, dtype):
    """Loopback world 2 x 33: every rank draws the 66 strata itself (cslam_pf_resample_sharded_drawn) against ranks that
    are handed them (cslam_pf_resample_sharded).  Rank 1 holds nearly all the weight, so records cross ranks.  The two
    ranks' normals are those of one handle of 66 particles: a draw depends on the GLOBAL slot."""
    from conan_slam_amd.pf import LoopbackComm
    from test_pf_gpu import _run_ranks

    world, L, nf, step = 2, 33, 3, 12
    N = world * L
    parts = random_particles(N, nf, dtype, seed=44)
    for i, p in enumerate(parts):
        p[0] = dtype(p[0] * (1e-3 if i < L else 1.0))
    drawn = [shard_from(parts[r * L:(r + 1) * L], nf, dtype) for r in range(world)]
    given = [shard_from(parts[r * L:(r + 1) * L], nf, dtype) for r in range(world)]
    whole = shard_from(parts, nf, dtype)
    whole.seed_draws(SEED)
    n_whole, select = whole.draws(step)
    assert _same_bits(select, synth.pf_draw_select(SEED, step, N, dtype))
    for r in range(world):
        drawn[r].seed_draws(SEED, r * L, N)
        n_r, s_r = drawn[r].draws(step)
        assert _same_bits(s_r, select) and _same_bits(n_r, np.ascontiguousarray(n_whole[:, r * L:(r + 1) * L])), r
    comms_a, comms_b = LoopbackComm.create(world), LoopbackComm.create(world)
    res_a = _run_ranks([(lambda r=r: drawn[r].resample_sharded_drawn(comms_a[r], step, N + 1, True)) for r in range(world)],
                       timeout=60.0)
    res_b = _run_ranks([(lambda r=r: given[r].resample_sharded(comms_b[r], select, N + 1, True)) for r in range(world)],
                       timeout=60.0)
    assert res_a == res_b and all(did for _, did in res_a)
    for r in range(world):
        _assert_shards_bit_equal(drawn[r], given[r], f"sharded drawn rank {r}")
        ea, eb = drawn[r].debug_last_exchange(world), given[r].debug_last_exchange(world)
        assert ea[0] == eb[0] and ea[1] == eb[1] and np.array_equal(ea[2], eb[2]), r
    assert drawn[1].debug_last_exchange(world)[0][0] > 0, "no record crossed from rank 1 to rank 0"
    # ... and the sharded set is the unsharded resample of the whole set with the same seed
    whole.resample_local_drawn(step, N + 1, True)
    wa = np.concatenate([sh.get_weights() for sh in drawn])
    assert _same_bits(wa, whole.get_weights())
    for g in (0, L - 1, L, N - 1):
        pa, pw = drawn[g // L].get_particle(g % L), whole.get_particle(g)
        assert all(_same_bits(x, y) for x, y in zip(pa[1:], pw[1:])), g
    # a shard seeded for other slots is refused before anything happens
    drawn[0].seed_draws(SEED, 0, L)
    _bad_arg(lambda: drawn[0].resample_sharded_drawn(comms_a[0], step, N + 1, True))
    _bad_arg(lambda: given[0].resample_sharded_drawn(comms_b[0], step, N + 1, True))  # never seeded
    for cm in comms_a + comms_b:
        cm.close()
    for sh in drawn + given + [whole]:
        sh.close()


# ------------------------------------------------------------------------------------------------ 6. no copy
def test_the_drawn_step_enqueues_no_copy_up_to_32_observations(gpu_required):
    dtype, npart = np.float32, 65
    case = ProposalCase(33, npart, dtype, nf=PROPOSAL_NF)
    sh = shard_from(case.parts, case.nf, dtype)
    sh.seed_draws(SEED)
    args = (0.0, 0.0, case.Q, PREDICT[2], PREDICT[3])  # a vehicle at rest: the same observations stay plausible
    step = 0
    for m, per_step in ((8, 0), (32, 0), (33, 1)):
        before = sh.stage_copies()
        for _ in range(3):  # (the same observations every time: a step of 33 still sends them every time)
            sh.observation_step_drawn(*args, case.Z[:, :m], case.idf[:m], case.R, step, 0, True)
            step += 1
        assert sh.stage_copies() - before == 3 * per_step, m
    normals, select = sh.draws(step)
    before = sh.stage_copies()
    for k in range(3):
        sh.observation_step(*args, case.Z[:, :8], case.idf[:8], case.R, normals, select, 0, True)
        assert sh.stage_copies() - before == k + 1
    sh.synchronize()
    sh.close()


# ------------------------------------------------------------------------------------------------ 7. isolation
@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_isolated(gpu_required, dtype):
    npart, m = 65, 8
    case = ProposalCase(m, npart, dtype, nf=PROPOSAL_NF, predict=True)
    a, b, plain = (shard_from(case.parts, case.nf, dtype) for _ in range(3))
    a.seed_draws(SEED)
    b.seed_draws(SEED)
    n0, s0 = a.draws(5)
    assert all(_same_bits(x, y) for x, y in zip(b.draws(5), (n0, s0)))
    n1, s1 = a.draws(6)
    assert not np.any(n1 == n0) and not _same_bits(s1, s0)
    b.seed_draws(SEED + 1)
    n2, s2 = b.draws(5)
    assert not np.any(n2 == n0) and not _same_bits(s2, s0)
    # an unseeded handle refuses every drawn call and its store is untouched
    args = (PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3])
    twin = shard_from(case.parts, case.nf, dtype)
    copies = plain.stage_copies()
    for call in (lambda: plain.draws(0), lambda: plain.sample_proposal_drawn(case.Z, case.idf, case.R, 0),
                 lambda: plain.sample_proposal_assoc_drawn(case.Z, case.R, 0),
                 lambda: plain.resample_local_drawn(0, npart + 1, True),
                 lambda: plain.observation_step_drawn(*args, case.Z, case.idf, case.R, 0, npart + 1, True)):
        _bad_arg(call)
    _assert_shards_bit_equal(plain, twin, "unseeded, refused")
    assert plain.stage_copies() == copies and plain.resample_stats()[0] == 0
    # a handle seeded for a slice of a larger set draws, but does not resample by itself
    twin.seed_draws(SEED, 10, 200)
    twin.draws(0)
    _bad_arg(lambda: twin.resample_local_drawn(0, npart + 1, True))
    _bad_arg(lambda: twin.observation_step_drawn(*args, case.Z, case.idf, case.R, 0, npart + 1, True))
    _assert_shards_bit_equal(plain, twin, "seeded for a slice, refused")
    # seeding changes nothing about the calls that take host arrays
    for t in range(2):
        a.observation_step(*args, case.Z, case.idf, case.R, n0, s0, npart + 1, True)
        plain.observation_step(*args, case.Z, case.idf, case.R, n0, s0, npart + 1, True)
        a.draws(t)  # (reading draws in between disturbs neither the store nor the staging area)
    _assert_shards_bit_equal(a, plain, "seeded against unseeded, host arrays")
    for sh in (a, b, plain, twin):
        sh.close()


def test_resample_particles_routes_a_step_to_the_drawn_forms(gpu_required):
    from conan_slam_amd.pf import SingleComm, resample_particles

    dtype, npart = np.float32, 70
    parts = random_particles(npart, 2, dtype, seed=9)
    a, b = shard_from(parts, 2, dtype), shard_from(parts, 2, dtype)
    a.seed_draws(SEED)
    ra = resample_particles(a, SingleComm(), npart + 1, True, step=4)
    rb = resample_particles(b, SingleComm(), npart + 1, True, select=synth.pf_draw_select(SEED, 4, npart, dtype))
    assert ra == rb and ra[1]
    _assert_shards_bit_equal(a, b, "resample_particles(step=)")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 8. statistics
def test_statistics_off_the_device(gpu_required):
    """3 x 4096 normals and 4096 strata uniforms at four steps, read from the device in f64 (the uniforms back out of the
    strata positions: u[i] = n select[i] - i, good to parts in 10^12)."""
    n = 4096
    sh = _shard(n, np.float64)
    sh.seed_draws(12345)
    xs, us = [], []
    for step in range(4):
        nrm, sel = sh.draws(step)
        xs.append(nrm.reshape(-1))
        us.append(sel * n - np.arange(n))
    x, u = np.concatenate(xs), np.concatenate(us)
    K = x.size
    z_mean, z_var = x.mean() * np.sqrt(K), (x.var() - 1.0) * np.sqrt(K / 2.0)
    z_u = (u.mean() - 0.5) * np.sqrt(12.0 * u.size)
    print(f"[draws] device: {K} normals mean z {z_mean:+.2f} variance z {z_var:+.2f}; {u.size} uniforms mean z {z_u:+.2f}")
    assert abs(z_mean) < 5 and abs(z_var) < 5 and abs(z_u) < 5
    assert u.min() > -1e-9 and u.max() < 1 + 1e-9
    sh.close()
