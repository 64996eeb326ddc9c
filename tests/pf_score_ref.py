"""Expected values of the particle filter's device-side score (cslam_pf_score*, include/cslam.h).  The specification is the
batched engine's restatement tests/score_ref.py with ONE instance, applied to the estimate a caller would have read at
that point -- an Estimate (ParticleShard.estimate()), a BestParticle (best_particle("max")) or the numpy Moments of
pf_estimate_ref.estimate_ref -- after rounding to the handle's dtype.  No arithmetic is restated here: this file only
reshapes the estimate into score_ref's arguments, keeps the expected track, and builds the inputs of the tests.

  reads(est, dtype)        the estimate -> x [1,3], pvv [1,3,3], xl [1,nf,2], pll [1,nf,2,2] (T-rounded, widened to f64)
  call(...)                score_ref.score_call with I = 1 -> (totals [11], bounds [11], record [4], record bounds [4])
  track_record(...)        the five doubles a score call logs
  PfScoreRef               score_ref.Accumulator with I = 1, plus the track
  values_case(...)         particles, truth rows and three true poses of the "values" cases (CPU and GPU files)
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import score_ref
from pf_builders import random_particles
from pf_estimate_ref import best_ref, estimate_ref, stack

BestRef = namedtuple("BestRef", "index w Xv Pv XF PF")  # the numpy twin of pf.BestParticle


def _rounded(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def reads(est, dtype, with_map=True):
    """est.Xv [3], est.Pv [3,3], est.XF [2,nf], est.PF [4,nf] (2 x 2 blocks column-major; XF / PF may be None)."""
    x = _rounded(est.Xv, dtype).reshape(1, 3)
    pvv = _rounded(est.Pv, dtype).reshape(1, 3, 3)
    if not with_map or est.XF is None or np.asarray(est.XF).size == 0:
        return x, pvv, np.zeros((1, 0, 2)), np.zeros((1, 0, 2, 2))
    XF, PF = _rounded(est.XF, dtype), _rounded(est.PF, dtype)
    nf = XF.shape[1]
    xl = XF.T.reshape(1, nf, 2)
    pll = PF.T.reshape(nf, 2, 2).transpose(0, 2, 1).reshape(1, nf, 2, 2)  # pll[f, r, c] = PF[r + 2 c, f]
    return x, pvv, xl, pll


def call(est, dtype, truth, xv_true, with_map=True, gate_pose=0.0, gate_lm=0.0):
    T, B, rec, rb = score_ref.score_call(*reads(est, dtype, with_map), truth, xv_true, gate_pose, gate_lm)
    return T[0], B[0], rec[0], rb[0]


def track_record(est, dtype, estimator):
    """(Xv, W, Neff) of the mixture or (Xv, w, index) of the best particle, as the handle's dtype holds them."""
    x = _rounded(est.Xv, dtype).reshape(3)
    if estimator == "mean":
        return np.array([x[0], x[1], x[2], float(est.w_sum), float(est.neff)])
    return np.array([x[0], x[1], x[2], float(_rounded(est.w, dtype)), float(est.index)])


class PfScoreRef:
    """A sequence of score calls: totals and series (score_ref.Accumulator, one instance) and the track."""

    def __init__(self, dtype, estimator="mean", series_capacity=0, gate_pose=0.0, gate_lm=0.0):
        self.dtype, self.estimator, self.cap = dtype, estimator, series_capacity
        self.acc = score_ref.Accumulator(1, series_capacity, gate_pose, gate_lm)
        self.track = []

    def add(self, est, truth, xv_true, with_map=True):
        if self.acc.calls < self.cap:
            self.track.append(track_record(est, self.dtype, self.estimator))
        self.acc.add(*reads(est, self.dtype, with_map), truth, xv_true)

    @property
    def totals(self):
        return self.acc.T[0]

    def expected_track(self):
        return np.array(self.track, dtype=np.float64).reshape(len(self.track), 5)

    def check(self, scores, tag="", track_bits=True):
        """scores: pf.PfScores.  Counts exact, sums and series within score_ref's bounds, the track bit for bit (NaNs
        alike when track_bits is False: a degenerate estimate)."""
        self.acc.check(scores.totals.reshape(1, -1), scores.series.reshape(-1, 1, 4), scores.calls, tag)
        want = self.expected_track()
        assert scores.track.shape == want.shape, (tag, scores.track.shape, want.shape)
        if track_bits:
            assert scores.track.tobytes() == want.tobytes(), f"{tag}: track\n{scores.track}\n{want}"
        else:
            assert np.array_equal(scores.track, want, equal_nan=True), f"{tag}: track\n{scores.track}\n{want}"


# ------------------------------------------------------------------------------------------------ the "values" cases
VALUES_NP = [1, 64, 65, 1025]  # one lane, one wave, a wave plus one, one estimate chunk plus one
VALUES_NF = [0, 1, 256, 257]   # no feature, one, exactly one landmark block, a block plus one
TRUTH_SHORT = 200              # truth rows given with nf = 257: fewer than the map holds
POSE_R2 = (1.5, 4.0, 20.0)     # squared Mahalanobis distance of the three true poses: two inside the gate 7.8147
LM_R2 = (0.5, 2.0, 12.0, 3.0, 30.0)  # of the true positions, cycled over the features: gate 5.9915

ValuesCase = namedtuple("ValuesCase", "parts ref truth xv_trues")


@lru_cache(maxsize=None)
def _particles(npart, nf, dtype_name):
    return random_particles(npart, nf, np.dtype(dtype_name).type, seed=100 * npart + nf)


def reference_estimate(parts, dtype, estimator):
    """What the handle would return, from float64 numpy on the stored values, rounded to dtype (widened again)."""
    w, X, P, XF, PF = stack(parts)
    if estimator == "mean":
        m = estimate_ref(w, X, P, XF, PF)
        return m._replace(Xv=_rounded(m.Xv, dtype), Pv=_rounded(m.Pv, dtype), XF=_rounded(m.XF, dtype),
                          PF=_rounded(m.PF, dtype))
    i = best_ref(w, "max")
    return BestRef(i, w[i], X[i], P[i], XF[i], PF[i])


def truth_count(nf):
    return TRUTH_SHORT if nf == 257 else nf


def _away(mean, cov_lower, r2, angles):
    """A point at squared Mahalanobis distance r2 from `mean` under the covariance whose lower triangle is given: the
    score's NEES of it is r2 up to rounding, far from either gate."""
    S = np.tril(cov_lower) + np.tril(cov_lower, -1).T
    L = np.linalg.cholesky(S)
    d = np.array([np.cos(angles[0]), np.sin(angles[0])]) if len(mean) == 2 else np.array(
        [np.cos(angles[0]) * np.cos(angles[1]), np.sin(angles[0]) * np.cos(angles[1]), np.sin(angles[1])])
    return mean - L @ (np.sqrt(r2) * d)


def values_case(npart, nf, dtype, estimator):
    """random_particles(npart, nf), the reference estimate, truth rows placed around its features and three true poses
    placed around its pose at known Mahalanobis distances (so that no NEES sits near a gate)."""
    dtype = np.dtype(dtype).type
    parts = _particles(npart, nf, np.dtype(dtype).name)
    ref = reference_estimate(parts, dtype, estimator)
    rng = np.random.default_rng(7 * npart + nf)
    k = truth_count(nf)
    truth = np.zeros((k, 2))
    for f in range(k):
        block = ref.PF[:, f].reshape(2, 2, order="F")
        truth[f] = _away(ref.XF[:, f], block, LM_R2[f % len(LM_R2)], rng.uniform(0, 2 * np.pi, 1))
    xv_trues = [_away(np.asarray(ref.Xv, np.float64), np.asarray(ref.Pv, np.float64), r2,
                      (rng.uniform(0, 2 * np.pi), rng.uniform(-1.0, 1.0))) for r2 in POSE_R2]
    return ValuesCase(parts, ref, truth, xv_trues)
