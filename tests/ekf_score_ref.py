"""The restatement of the single handle's score (cslam_ekf_score, EKF.score / scores): score_ref.Accumulator with one
instance, fed from the reads a host scorer makes at the same point -- EKF.pose() and EKF.landmarks(), which leave the run
alone -- plus what score_ref does not hold: the track record (X[0:3], trace(P), n) and its rounding bound.

Device and restatement start from the same bits (the handle's dtype) and work in f64, for f32 and f64 handles alike.
  track pose   X[0:3] widened to f64: bitwise.
  track n      exact.
  track trace  the n diagonal entries d -- three from pose()'s block, two per landmark from landmarks()'s blocks -- widened
               and added in f64.  The device adds them in another order (per landmark, a shuffle tree, the waves, the
               blocks, the pose), the restatement exactly (math.fsum): a sum of n terms in any order is within
               (n - 1) u sum |d| of the exact one, u = 2^-53; the bound used is twice that.
"""
import math

import numpy as np

import score_ref as sr

U = sr.U


def trace_terms(pvv, pll):
    """the diagonal of P from the reads, widened: pose block [3, 3], landmark blocks [c, 2, 2] -> f64 [3 + 2 c]"""
    pvv, pll = np.asarray(pvv, np.float64), np.asarray(pll, np.float64)
    return np.concatenate([np.diagonal(pvv), pll[:, 0, 0], pll[:, 1, 1]]) if pll.size else np.diagonal(pvv).copy()


def trace_ref(d):
    """(the exact f64 sum of the terms, the bound 2 (n - 1) u sum |d|)"""
    d = np.asarray(d, np.float64)
    return math.fsum(d.tolist()), 2 * (d.size - 1) * U * float(np.abs(d).sum())


class SingleRef:
    """What a sequence of EKF.score calls must leave in scores(): add() right after every score call of the handle."""

    def __init__(self, series_capacity=0, gate_pose=0.0, gate_lm=0.0):
        self.acc = sr.Accumulator(1, series_capacity, gate_pose, gate_lm)
        self.cap = series_capacity
        self.track = []  # per record: (x f64 [3], trace or NaN, bound, n)

    def add(self, e, truth, xv_true, with_map=True):
        """e: the EKF handle, just scored against xv_true with this truth ([k, 2]) and with_map"""
        x, pvv = e.pose()
        nl = (e.n - 3) // 2
        if nl:
            xl, pll, _ = e.landmarks()
        else:
            xl, pll = np.zeros((0, 2), e.dtype), np.zeros((0, 2, 2), e.dtype)
        rows = np.asarray(truth, np.float64).reshape(-1, 2) if with_map else np.zeros((0, 2))
        record = self.acc.calls < self.cap
        self.acc.add(x[None], pvv[None], xl[None], pll[None], rows, np.asarray(xv_true, np.float64))
        if record:
            tr, b = trace_ref(trace_terms(pvv, pll)) if with_map else (np.nan, 0.0)
            self.track.append((x.astype(np.float64), tr, b, e.n))
        return x, pvv, xl, pll

    def check(self, scores, tag="", control=True):
        """scores: EKF.scores().  Counts exact, sums and series within score_ref's bounds, the track as in the docstring;
        control: the bounds reject a relative error of 1e-6 in every sum and series value and of 1e-9 in the trace."""
        totals, series, track, calls = scores
        T, S = totals[None], series[:, None, :]
        self.acc.check(T, S, calls, tag)
        assert track.shape == (len(self.track), 5) and track.dtype == np.float64, (tag, track.shape)
        for r, (x, tr, b, n) in enumerate(self.track):
            assert track[r, :3].tobytes() == x.tobytes(), f"{tag}: track pose of record {r} is not pose()'s x"
            assert track[r, 4] == n, (tag, r, track[r, 4], n)
            if np.isnan(tr):
                assert np.isnan(track[r, 3]), (tag, r, track[r, 3])
                continue
            assert abs(track[r, 3] - tr) <= b, f"{tag}: trace of record {r} off by {abs(track[r, 3] - tr):.3e} > {b:.3e}"
            if control and tr != 0:
                assert abs(track[r, 3] * (1 + 1e-9) - tr) > b, f"{tag}: the trace bound is too loose to reject 1e-9"
        if not control:
            return
        for f in (sr.POSE_ERR2, sr.POSE_EPHI2, sr.POSE_NEES, sr.LM_ERR2, sr.LM_NEES):
            if T[0, f] == 0:
                continue
            bad = T.copy()
            bad[0, f] *= 1 + 1e-6
            try:
                self.acc.check(bad, S, calls, tag)
            except AssertionError:
                continue
            raise AssertionError(f"{tag}: the bound of {sr.FIELDS[f]} is too loose to reject 1e-6")
        if S.size and np.any(np.isfinite(S) & (S != 0)):
            try:
                self.acc.check(T, (S.astype(np.float64) * (1 + 1e-6)).astype(np.float32), calls, tag)
            except AssertionError:
                return
            raise AssertionError(f"{tag}: the series bounds are too loose to reject 1e-6")
