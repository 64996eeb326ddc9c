"""A numpy f64 restatement of the batched engine's score step (cslam_ekf_batch_score, include/cslam.h): what one call adds
to the totals of every instance and the series record it writes, from the reads a host scorer would make at that point
(EKFBatch.poses() and EKFBatch.landmarks()), with a rounding bound for every number.

The bounds (u = 2^-53; both sides work in f64 from the same f32 state, so they differ by rounding only, the device side
with fused multiply-adds):
  landmark  q = N / det, N = p11 e0^2 - 2 p10 e0 e1 + p00 e1^2, det = p00 p11 - p10^2.  N carries at most 8 roundings
            of terms bounded by Nabs = |p11| e0^2 + 2 |p10 e0 e1| + |p00| e1^2, det at most 3 of terms bounded by
            Dabs = |p00 p11| + p10^2, the quotient one more, on each side:
                |dq| <= 2 * 8 u (Nabs / det + |q| Dabs / det + |q|).
            Dabs / det is the block's condition in the sense that matters here (cancellation in the determinant).
  pose      q = e^T A^-1 e by a 3 x 3 Cholesky and a forward substitution: |dq| <= 2 * 32 u cond_2(A) q (Higham,
            Accuracy and Stability of Numerical Algorithms, Theorem 10.4 with n = 3 and a generous constant), plus the
            heading wrap: d - 2 pi k is one fused or two separate roundings, |de2| <= 4 u (|d| + 2 pi), which moves
            e2^2 by 2 |e2| |de2| and q by 2 sqrt(q / lambda_min(A)) |de2|.
  err^2     e0^2 + e1^2: three roundings a side, 8 u err^2.
  a sum     of n terms in any order: (n - 1) u sum |t| a side, on top of the terms' own bounds.
  series    an f64 value with bound b stored as f32: b + half an f32 ulp of the value; a mean S / n: b_S / n + 2 u |mean|.
"""
import numpy as np

FIELDS = ("POSE_N", "POSE_BAD", "POSE_IN", "POSE_ERR2", "POSE_EPHI2", "POSE_NEES",
          "LM_N", "LM_BAD", "LM_IN", "LM_ERR2", "LM_NEES")
(POSE_N, POSE_BAD, POSE_IN, POSE_ERR2, POSE_EPHI2, POSE_NEES, LM_N, LM_BAD, LM_IN, LM_ERR2, LM_NEES) = range(len(FIELDS))
COUNTS = (POSE_N, POSE_BAD, POSE_IN, LM_N, LM_BAD, LM_IN)
GATE_POSE, GATE_LM = 7.8147, 5.9915  # the 95 % chi-square points of 3 and 2 degrees of freedom
U = 2.0 ** -53


def wrap(d):
    """(-pi, pi]"""
    return d - 2 * np.pi * np.ceil((d - np.pi) / (2 * np.pi))


def pose_score(x, A, xt):
    """One instance's pose: (ok, e [3], nees, bounds (err2, ephi2, nees)).  A: the 3 x 3 pose block (its lower triangle
    is used)."""
    x, A, xt = np.asarray(x, np.float64), np.asarray(A, np.float64), np.asarray(xt, np.float64)
    d = x[2] - xt[2]
    e = np.array([x[0] - xt[0], x[1] - xt[1], wrap(d)])
    low = A[np.tril_indices(3)]
    if not (np.all(np.isfinite(e)) and np.all(np.isfinite(low))):
        return False, e, np.nan, None
    L = np.zeros((3, 3))
    for c in range(3):
        piv = A[c, c] - L[c, :c] @ L[c, :c]
        if not (np.isfinite(piv) and piv > 0):
            return False, e, np.nan, None
        L[c, c] = np.sqrt(piv)
        for r in range(c + 1, 3):
            L[r, c] = (A[r, c] - L[r, :c] @ L[c, :c]) / L[c, c]
    y = np.zeros(3)
    for r in range(3):
        y[r] = (e[r] - L[r, :r] @ y[:r]) / L[r, r]
    q = float(y @ y)
    if not np.isfinite(q):
        return False, e, np.nan, None
    S = np.tril(A) + np.tril(A, -1).T
    lam = np.linalg.eigvalsh(S)
    cond = lam[-1] / lam[0] if lam[0] > 0 else np.inf
    de2 = 4 * U * (abs(d) + 2 * np.pi)
    err2 = e[0] ** 2 + e[1] ** 2
    b = (8 * U * err2, 2 * abs(e[2]) * de2 + 8 * U * e[2] ** 2,
         2 * 32 * U * cond * q + 2 * np.sqrt(q / lam[0]) * de2 if lam[0] > 0 else np.inf)
    return True, e, q, b


def landmark_scores(xl, pll, truth):
    """One instance's landmarks xl [c, 2], pll [c, 2, 2] against truth [c, 2]: (ok [c], err2 [c], nees [c],
    bound_err2 [c], bound_nees [c]); entries of bad blocks are zero."""
    xl, pll, truth = np.asarray(xl, np.float64), np.asarray(pll, np.float64), np.asarray(truth, np.float64)
    c = xl.shape[0]
    e = xl - truth[:c]
    p00, p10, p11 = pll[:, 0, 0], pll[:, 1, 0], pll[:, 1, 1]
    with np.errstate(all="ignore"):
        det = p00 * p11 - p10 * p10
        N = p11 * e[:, 0] ** 2 - 2 * p10 * e[:, 0] * e[:, 1] + p00 * e[:, 1] ** 2
        q = N / det
        fin = np.isfinite(e).all(axis=1) & np.isfinite(p00) & np.isfinite(p10) & np.isfinite(p11) & np.isfinite(q)
        ok = fin & (p00 > 0) & (det > 0)
        err2 = e[:, 0] ** 2 + e[:, 1] ** 2
        Nabs = np.abs(p11) * e[:, 0] ** 2 + 2 * np.abs(p10 * e[:, 0] * e[:, 1]) + np.abs(p00) * e[:, 1] ** 2
        Dabs = np.abs(p00 * p11) + p10 * p10
        bq = 2 * 8 * U * (Nabs / det + np.abs(q) * Dabs / det + np.abs(q))
    z = np.zeros(c)
    return ok, np.where(ok, err2, z), np.where(ok, q, z), np.where(ok, 8 * U * err2, z), np.where(ok, bq, z)


def score_call(x, pvv, xl, pll, truth, xv_true, gate_pose=0.0, gate_lm=0.0):
    """What one score call adds: (totals [I, 11], totals_bound [I, 11], record [I, 4] f64, record_bound [I, 4]).
    x [I, 3], pvv [I, 3, 3], xl [I, c, 2], pll [I, c, 2, 2] as EKFBatch.poses() / landmarks() return them; truth [k, 2]:
    min(c, k) features are scored.  The record bound includes the half f32 ulp of the stored value."""
    gp = gate_pose if gate_pose > 0 else GATE_POSE
    gl = gate_lm if gate_lm > 0 else GATE_LM
    I = len(x)
    truth = np.asarray(truth, np.float64).reshape(-1, 2)
    c = min(xl.shape[1], truth.shape[0]) if I else 0
    T, B = np.zeros((I, len(FIELDS))), np.zeros((I, len(FIELDS)))
    rec, rb = np.full((I, 4), np.nan), np.zeros((I, 4))
    for i in range(I):
        ok, e, q, b = pose_score(x[i], pvv[i], xv_true)
        if ok:
            err2 = e[0] ** 2 + e[1] ** 2
            T[i, POSE_N], T[i, POSE_IN] = 1, float(q <= gp)
            T[i, POSE_ERR2], T[i, POSE_EPHI2], T[i, POSE_NEES] = err2, e[2] ** 2, q
            B[i, POSE_ERR2], B[i, POSE_EPHI2], B[i, POSE_NEES] = b
            rec[i, 0], rec[i, 1] = err2, q
            rb[i, 0], rb[i, 1] = b[0], b[2]
        else:
            T[i, POSE_BAD] = 1
        lok, lerr2, lq, berr2, bq = landmark_scores(xl[i, :c], pll[i, :c], truth[:c])
        nv = int(lok.sum())
        T[i, LM_N], T[i, LM_BAD], T[i, LM_IN] = nv, c - nv, int((lok & (lq <= gl)).sum())
        T[i, LM_ERR2], T[i, LM_NEES] = lerr2.sum(), lq.sum()
        B[i, LM_ERR2] = berr2.sum() + 2 * max(c - 1, 0) * U * np.abs(lerr2).sum()
        B[i, LM_NEES] = bq.sum() + 2 * max(c - 1, 0) * U * np.abs(lq).sum()
        if nv:
            rec[i, 2], rec[i, 3] = T[i, LM_ERR2] / nv, T[i, LM_NEES] / nv
            rb[i, 2] = B[i, LM_ERR2] / nv + 2 * U * abs(rec[i, 2])
            rb[i, 3] = B[i, LM_NEES] / nv + 2 * U * abs(rec[i, 3])
    with np.errstate(invalid="ignore"):
        half_ulp = np.where(np.isfinite(rec), 0.5 * np.spacing(np.abs(rec).astype(np.float32)).astype(np.float64), 0.0)
    return T, B, rec, rb + half_ulp


class Accumulator:
    """The totals and series of a sequence of score calls, with their bounds (one more rounding per call and sum)."""

    def __init__(self, instances, series_capacity=0, gate_pose=0.0, gate_lm=0.0):
        self.I, self.cap, self.gp, self.gl = instances, series_capacity, gate_pose, gate_lm
        self.T = np.zeros((instances, len(FIELDS)))
        self.B = np.zeros((instances, len(FIELDS)))
        self.series, self.series_bound, self.calls = [], [], 0

    def add(self, x, pvv, xl, pll, truth, xv_true):
        T, B, rec, rb = score_call(x, pvv, xl, pll, truth, xv_true, self.gp, self.gl)
        self.T += T
        self.B += B + 2 * U * np.abs(self.T)
        if self.calls < self.cap:
            self.series.append(rec)
            self.series_bound.append(rb)
        self.calls += 1

    def check(self, totals, series, calls, tag=""):
        """Counts exact, sums and series within the bounds; raises AssertionError."""
        assert calls == self.calls, (tag, calls, self.calls)
        assert np.array_equal(totals[:, COUNTS], self.T[:, COUNTS]), f"{tag}: counts differ\n{totals[:, COUNTS]}\n{self.T[:, COUNTS]}"
        assert np.all(np.isfinite(totals)), f"{tag}: non-finite totals"
        d = np.abs(totals - self.T)
        assert np.all(d <= self.B), f"{tag}: totals off the restatement: {d.max(axis=0)} > {self.B.max(axis=0)}"
        assert series.shape == (len(self.series), self.I, 4), (tag, series.shape)
        if self.series:
            ref, rb = np.stack(self.series), np.stack(self.series_bound)
            assert np.array_equal(np.isnan(series), np.isnan(ref)), f"{tag}: NaN pattern of the series differs"
            m = ~np.isnan(ref)
            d = np.abs(series.astype(np.float64)[m] - ref[m])
            assert np.all(d <= rb[m]), f"{tag}: series off the restatement by {(d - rb[m]).max():.3e}"
