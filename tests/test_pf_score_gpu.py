"""The particle filter's score and trajectory log on the device (cslam_pf_score*, include/cslam.h) against the
restatement tests/score_ref.py with one instance, applied through tests/pf_score_ref.py to what ParticleShard.estimate()
/ best_particle("max") return at that moment: counts exact, sums and series within score_ref's bounds, the track bit for
bit.  The estimate reads in these tests serve the reference only; the score calls themselves return nothing."""
import ctypes as C

import numpy as np
import pytest

from pf_builders import DTYPES, PREDICT, ProposalCase, random_particles, shard_from
from pf_estimate_cases import wrap_cloud
from pf_estimate_ref import download
from pf_score_ref import PfScoreRef, VALUES_NF, VALUES_NP, call, truth_count, values_case
from score_ref import (FIELDS, GATE_LM, GATE_POSE, LM_BAD, LM_ERR2, LM_IN, LM_N, LM_NEES, POSE_BAD, POSE_EPHI2, POSE_ERR2,
                       POSE_IN, POSE_N, POSE_NEES, wrap)
from test_pf_gpu import _run_ranks

from conan_slam_amd import CslamError, _capi

pytestmark = pytest.mark.gpu

LM_FIELDS = [LM_N, LM_BAD, LM_IN, LM_ERR2, LM_NEES]
POSE_SUMS = [POSE_ERR2, POSE_EPHI2, POSE_NEES]


def _read(sh, estimator, comm=None):
    """The estimate a caller would read now (for the reference only)."""
    if estimator == "mean":
        return sh.estimate() if comm is None else sh.estimate_sharded(comm)
    return sh.best_particle("max") if comm is None else sh.best_particle_sharded(comm, "max")


def _same_scores(a, b):
    return (a.totals.tobytes() == b.totals.tobytes() and a.series.tobytes() == b.series.tobytes()
            and a.track.tobytes() == b.track.tobytes() and a.calls == b.calls)


def _bad_arg(fn):
    with pytest.raises(CslamError) as ei:
        fn()
    assert ei.value.code == _capi.ERR_BAD_ARG, ei.value


# ------------------------------------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nf", VALUES_NF)
@pytest.mark.parametrize("npart", VALUES_NP)
def test_values(gpu_required, npart, nf, dtype):
    """Every shape, both estimators on one shard: truth, three score calls with different true poses; nf = 257 with
    200 truth rows scores 200 features."""
    sh = None
    for estimator in ("mean", "best"):
        case = values_case(npart, nf, dtype, estimator)
        if sh is None:
            sh = shard_from(case.parts, max(nf, 1), dtype)
        tag = f"np={npart} nf={nf} {np.dtype(dtype).name} {estimator}"
        sh.score_reset(estimator, series_capacity=3)
        sh.score_set_truth(case.truth)
        ref = PfScoreRef(dtype, estimator, series_capacity=3)
        for xv_true in case.xv_trues:
            ref.add(_read(sh, estimator), case.truth, xv_true)
            sh.score(xv_true)
        got = sh.scores()
        print(f"[pf score] {tag}: totals {got.totals} ref {ref.totals} bounds {ref.acc.B[0]}")
        ref.check(got, tag)
        c = truth_count(nf)
        assert got.totals[LM_N] == 3 * c and got.totals[POSE_N] == 3 and got.totals[POSE_IN] == 2, (tag, got.totals)
        if estimator == "best":
            assert np.all(got.track[:, 4] == _read(sh, "best").index), (tag, got.track)
    sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("estimator", ["mean", "best"])
def test_without_the_map(gpu_required, estimator, dtype):
    """with_map=False: the landmark totals stay zero and series fields 2 and 3 are NaN; a call with the map on the same
    handle then scores the features."""
    npart, nf = 65, 257
    case = values_case(npart, nf, dtype, estimator)
    sh = shard_from(case.parts, nf, dtype)
    sh.score_reset(estimator, series_capacity=2)
    sh.score_set_truth(case.truth)
    ref = PfScoreRef(dtype, estimator, series_capacity=2)
    ref.add(_read(sh, estimator), case.truth, case.xv_trues[0], with_map=False)
    sh.score(case.xv_trues[0], with_map=False)
    got = sh.scores()
    ref.check(got, "no map")
    assert np.all(got.totals[LM_FIELDS] == 0) and np.isnan(got.series[0, 2:]).all() and np.isfinite(got.series[0, :2]).all()
    ref.add(_read(sh, estimator), case.truth, case.xv_trues[1])
    sh.score(case.xv_trues[1])
    got = sh.scores()
    ref.check(got, "then with the map")
    assert got.totals[LM_N] == truth_count(nf) and np.isfinite(got.series[1]).all()
    sh.close()


# ------------------------------------------------------------------------------------------------ 2. heading wrap
@pytest.mark.parametrize("dtype", DTYPES)
def test_heading_error_is_wrapped(gpu_required, dtype):
    parts = wrap_cloud(64, 2, dtype)
    sh = shard_from(parts, 2, dtype)
    est = sh.estimate()
    assert float(est.Xv[2]) > 3.0
    xv_true = np.array([float(est.Xv[0]) + 0.1, float(est.Xv[1]) - 0.1, -3.1])
    sh.score_reset("mean", 1)
    sh.score(xv_true, with_map=False)
    got = sh.scores()
    T, B, _, _ = call(est, dtype, np.zeros((0, 2)), xv_true, with_map=False)
    e2 = wrap(float(est.Xv[2]) + 3.1)
    assert abs(e2) < 0.2 and abs(T[POSE_EPHI2] - e2 * e2) <= B[POSE_EPHI2]
    print(f"[pf score] wrap {np.dtype(dtype).name}: EPHI2 {got.totals[POSE_EPHI2]:.17g} ref {T[POSE_EPHI2]:.17g} "
          f"bound {B[POSE_EPHI2]:.3e}")
    assert got.totals[POSE_N] == 1
    assert abs(got.totals[POSE_EPHI2] - T[POSE_EPHI2]) <= B[POSE_EPHI2]
    assert got.totals[POSE_EPHI2] < 0.05, "the error must not be near (2 pi)^2"
    sh.close()


# ------------------------------------------------------------------------------------------------ 3. bad blocks
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_blocks(gpu_required, dtype):
    npart, nf, c = 65, 5, 4
    parts = random_particles(npart, nf, dtype, seed=31)
    sh = shard_from(parts, nf, dtype)
    est = sh.estimate()
    truth = np.asarray(est.XF, np.float64).T[:c] + 0.01
    xv_true = np.asarray(est.Xv, np.float64) + 0.01
    sh.score_reset("mean", 4)
    sh.score_set_truth(truth)
    ref = PfScoreRef(dtype, "mean", 4)
    ref.add(est, truth, xv_true)
    sh.score(xv_true)
    before = sh.scores()
    ref.check(before, "healthy")
    assert before.totals[POSE_N] == 1 and before.totals[LM_N] == c
    # all weights zero: the estimate is NaN
    w = sh.get_weights()
    sh.set_weights(np.zeros(npart, dtype))
    ref.add(sh.estimate(), truth, xv_true)
    sh.score(xv_true)
    got = sh.scores()
    ref.check(got, "zero weights", track_bits=False)
    assert got.totals[POSE_BAD] == 1 and got.totals[LM_BAD] == c
    sums = POSE_SUMS + [LM_ERR2, LM_NEES, POSE_N, POSE_IN, LM_N, LM_IN]
    assert got.totals[sums].tobytes() == before.totals[sums].tobytes(), "a bad block must leave the sums alone"
    assert np.isnan(got.series[1]).all() and got.track[1, 3] == 0.0 and np.isnan(got.track[1, [0, 1, 2, 4]]).all()
    sh.set_weights(w)
    # one truth row NaN: exactly one bad landmark
    bad_truth = truth.copy()
    bad_truth[2, 1] = np.nan
    sh.score_set_truth(bad_truth)
    ref.add(sh.estimate(), bad_truth, xv_true)
    sh.score(xv_true)
    got = sh.scores()
    ref.check(got, "NaN truth row", track_bits=False)
    assert got.totals[LM_BAD] == c + 1 and got.totals[LM_N] == 2 * c - 1 and got.totals[POSE_N] == 2
    sh.close()
    # BEST right after a proposal: the sampled pose has Pv = 0, which is no covariance to score against
    pc = ProposalCase(4, 73, dtype, nf=6)
    sh = shard_from(pc.parts, 6, dtype)
    sh.sample_proposal(pc.Z, pc.idf, pc.R, pc.normals)
    best = sh.best_particle("max")
    assert not np.any(np.asarray(best.Pv)), "PF.cpp:537 leaves Pv = 0 behind the proposal"
    sh.score_reset("best", 1)
    sh.score_set_truth(pc.base.T)
    ref = PfScoreRef(dtype, "best", 1)
    ref.add(best, pc.base.T, np.asarray(best.Xv, np.float64) + 0.01)
    sh.score(np.asarray(best.Xv, np.float64) + 0.01)
    got = sh.scores()
    ref.check(got, "best after a proposal")
    assert got.totals[POSE_BAD] == 1 and got.totals[POSE_N] == 0 and not np.any(got.totals[POSE_SUMS])
    assert got.totals[LM_N] == 6 and np.isnan(got.series[0, :2]).all()
    sh.close()


# ------------------------------------------------------------------------------------------------ 4. no perturbation
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_perturbation_determinism_and_no_copy(gpu_required, dtype):
    case = ProposalCase(4, 73, dtype, nf=6, predict=True)
    truth = case.base.T
    xv_true = np.array([0.05, -0.02, 0.21])

    def run(score):
        sh = shard_from(case.parts, 6, dtype)
        sh.seed_draws(11)
        if score:
            sh.score_reset("mean", 8)
            sh.score_set_truth(truth)
        for step in range(4):
            sh.observation_step_drawn(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3], case.Z, case.idf, case.R,
                                      step, 73 * 0.75, True)
            if score:
                sh.score(xv_true)
        return sh

    a, b = run(True), run(False)
    assert a.stage_copies() == b.stage_copies(), "a score call must not stage a copy"
    assert a.resample_stats() == b.resample_stats()
    for name, x, y in zip("w X P XF PF".split(), download(a), download(b)):
        assert x.tobytes() == y.tobytes(), ("the score perturbed the store", name)
    first = a.scores()
    assert first.calls == 4 and first.series.shape == (4, 4) and first.totals[POSE_N] + first.totals[POSE_BAD] == 4
    # the same state scored twice: identical bits
    for sh in (a, b):
        sh.score_reset("mean", 2)
        sh.score_set_truth(truth)
        sh.score(xv_true)
        sh.score(xv_true)
    sa, sb = a.scores(), b.scores()
    assert _same_scores(sa, sb)
    assert sa.series[0].tobytes() == sa.series[1].tobytes() and sa.track[0].tobytes() == sa.track[1].tobytes()
    # a score queued right behind an asynchronous step scores the advanced store
    before = a.estimate()
    a.score_reset("mean", 1)
    a.observation_step_drawn(PREDICT[0], PREDICT[1], case.Q, PREDICT[2], PREDICT[3], case.Z, case.idf, case.R, 4, 0.0, False)
    a.score(xv_true)
    after = a.estimate()
    assert np.asarray(after.Xv).tobytes() != np.asarray(before.Xv).tobytes()
    ref = PfScoreRef(dtype, "mean", 1)
    ref.add(after, truth, xv_true)
    ref.check(a.scores(), "behind a queued step")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. capacity and reset
@pytest.mark.parametrize("dtype", DTYPES)
def test_capacity_and_reset(gpu_required, dtype):
    npart, nf = 65, 1
    case = values_case(npart, nf, dtype, "mean")
    sh = shard_from(case.parts, nf, dtype)
    xs = [case.xv_trues[i % 3] + 0.001 * i for i in range(5)]
    # without a reset: as after reset(MEAN, 0, 0, 0), and no truth yet -> no feature scored
    est = sh.estimate()
    ref = PfScoreRef(dtype, "mean", 0)
    ref.add(est, np.zeros((0, 2)), xs[0])
    sh.score(xs[0])
    got = sh.scores()
    ref.check(got, "no reset")
    assert got.calls == 1 and got.series.shape == (0, 4) and got.track.shape == (0, 5) and got.totals[LM_N] == 0
    # capacity 2, five calls
    sh.score_set_truth(case.truth)
    sh.score_reset("mean", 2)
    ref = PfScoreRef(dtype, "mean", 2)
    for x in xs:
        ref.add(est, case.truth, x)
        sh.score(x)
    got = sh.scores()
    ref.check(got, "capacity 2")
    assert got.calls == 5 and got.series.shape == (2, 4) and got.totals[POSE_N] == 5 and got.totals[LM_N] == 5 * nf
    one = sh.scores(capacity_records=1)
    assert one.series.shape == (1, 4) and one.series.tobytes() == got.series[:1].tobytes()
    assert one.track.tobytes() == got.track[:1].tobytes() and one.totals.tobytes() == got.totals.tobytes()
    rec, calls = C.c_int(-1), C.c_longlong(-1)
    assert _capi.lib().cslam_pf_get_scores(sh._h, None, None, None, 0, C.byref(rec), C.byref(calls)) == _capi.OK
    assert rec.value == 2 and calls.value == 5
    # reset: zeroes, and keeps the truth (the next call scores the feature again)
    sh.score_reset("mean", 3)
    got = sh.scores()
    assert got.calls == 0 and not np.any(got.totals) and got.series.shape == (0, 4)
    ref = PfScoreRef(dtype, "mean", 3)
    ref.add(est, case.truth, xs[1])
    sh.score(xs[1])
    got = sh.scores()
    ref.check(got, "after the reset")
    assert got.totals[LM_N] == nf
    # gates: <= 0 takes the defaults; a tiny pose gate and a huge landmark gate change only the IN counts
    q_pose, q_lm = got.totals[POSE_NEES], got.totals[LM_NEES]
    assert got.totals[POSE_IN] == float(q_pose <= GATE_POSE) and got.totals[LM_IN] == float(q_lm <= GATE_LM)
    sh.score_reset("mean", 0, -1.0, 0.0)
    sh.score(xs[1])
    dflt = sh.scores()
    assert dflt.totals.tobytes() == got.totals.tobytes()
    sh.score_reset("mean", 0, q_pose * 0.5, q_lm * 2.0)
    ref = PfScoreRef(dtype, "mean", 0, q_pose * 0.5, q_lm * 2.0)
    ref.add(est, case.truth, xs[1])
    sh.score(xs[1])
    got = sh.scores()
    ref.check(got, "own gates")
    assert got.totals[POSE_IN] == 0 and got.totals[LM_IN] == 1
    sh.close()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors_change_nothing(gpu_required):
    dtype, npart, nf = np.float32, 65, 1
    case = values_case(npart, nf, dtype, "mean")
    sh = shard_from(case.parts, nf, dtype)
    L = _capi.lib()
    sh.score_reset("mean", 4)
    sh.score_set_truth(case.truth)
    sh.score(case.xv_trues[0])
    sh.score(case.xv_trues[1])
    before = sh.scores()
    assert before.calls == 2
    x = np.ascontiguousarray(case.xv_trues[2], dtype=np.float64)
    nan_x = x.copy()
    nan_x[1] = np.nan
    inf_x = x.copy()
    inf_x[2] = np.inf
    refused = [
        lambda: sh.score_reset(2, 4),                       # a bad estimator
        lambda: sh.score_reset(-1, 4),
        lambda: sh.score_reset("best", -1),                 # a negative capacity
        lambda: sh.score_set_truth(np.zeros((nf + 1, 2))),  # count > max_features
        lambda: sh.score(nan_x),
        lambda: sh.score(inf_x),
    ]
    for i, fn in enumerate(refused):
        _bad_arg(fn)
        assert _same_scores(sh.scores(), before), ("a refused call changed the score", i)
    assert L.cslam_pf_score(sh._h, None, C.c_int(1)) == _capi.ERR_BAD_ARG  # a NULL true pose
    assert L.cslam_pf_score_set_truth(sh._h, None, C.c_int(-1)) == _capi.ERR_BAD_ARG
    assert L.cslam_pf_score_sharded(sh._h, None, x.ctypes.data_as(C.c_void_p), C.c_int(1)) == _capi.ERR_BAD_ARG
    assert _same_scores(sh.scores(), before)
    # the refused reset("best") left the estimator, and the refused set_truth the rows: the next call continues the run
    ref = PfScoreRef(dtype, "mean", 4)
    for xv in case.xv_trues:
        ref.add(sh.estimate(), case.truth, xv)
    sh.score(x)
    ref.check(sh.scores(), "after the refusals")
    sh.close()


# ------------------------------------------------------------------------------------------------ 7. sharded
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("estimator", ["mean", "best"])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_sharded_loopback(gpu_required, world, estimator, dtype):
    """65 particles per rank, 3 features: every rank ends with the same bits, they pass the restatement on the sharded
    estimate, a world of one equals the unsharded call bit for bit, and BEST logs the GLOBAL index."""
    from conan_slam_amd.pf import LoopbackComm

    L, nf = 65, 3
    parts = random_particles(world * L, nf, dtype, seed=40 + world)
    if estimator == "best" and world > 1:
        parts[(world - 1) * L + 7][0] = dtype(0.9)  # the maximum lives on the last rank
    whole = shard_from(parts, nf, dtype)
    shards = [shard_from(parts[r * L:(r + 1) * L], nf, dtype) for r in range(world)]
    comms = LoopbackComm.create(world)
    est0 = _read(whole, estimator)
    truth = np.asarray(est0.XF, np.float64).T + np.array([0.3, -0.2])
    xs = [np.asarray(est0.Xv, np.float64) + d for d in ([0.1, 0.1, 0.01], [-0.4, 0.2, -0.02], [2.0, -2.0, 0.1])]

    def rank(r):
        sh = shards[r]
        sh.score_reset(estimator, 3)
        sh.score_set_truth(truth)
        reads = []
        for i, xv in enumerate(xs):
            reads.append(_read(sh, estimator, comms[r]))
            sh.score_sharded(comms[r], xv, with_map=(i != 1))
        return reads, sh.scores()

    res = _run_ranks([(lambda r=r: rank(r)) for r in range(world)])
    tag = f"world={world} {estimator} {np.dtype(dtype).name}"
    for r in range(1, world):
        assert _same_scores(res[r][1], res[0][1]), (tag, "ranks differ", r)
    ref = PfScoreRef(dtype, estimator, 3)
    for i, xv in enumerate(xs):
        ref.add(res[0][0][i], truth, xv, with_map=(i != 1))
    got = res[0][1]
    ref.check(got, tag)
    assert got.totals[POSE_N] == 3 and got.totals[LM_N] == 2 * nf
    if estimator == "best":
        assert np.all(got.track[:, 4] == whole.best_particle("max").index), (tag, got.track)
        if world > 1:
            assert got.track[0, 4] == (world - 1) * L + 7
    if world == 1:
        whole.score_reset(estimator, 3)
        whole.score_set_truth(truth)
        for i, xv in enumerate(xs):
            whole.score(xv, with_map=(i != 1))
        assert _same_scores(whole.scores(), got), (tag, "a world of one must equal the unsharded call")
    for c in comms:
        c.close()
    for sh in shards + [whole]:
        sh.close()
    assert len(FIELDS) == _capi.SCORE_FIELDS
