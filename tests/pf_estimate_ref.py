"""Expected values of the particle filter's read path (cslam_pf_best_particle / _estimate / _get_all_features), in plain
float64 numpy, from the particle values as the handle stores them.  Nothing here touches the engine.

  stack(parts)            the builders' particle lists -> arrays (w [n], X [n,3], P [n,3,3], XF [n,2,nf], PF [n,4,nf])
  estimate_ref            the mixture moments, TWO passes: means first, then second moments about them
  estimate_blocks_ref     the same moments from per-block summaries merged in block order (the sharded form's algebra)
  estimate_raw_ref        the same moments the way they must NOT be computed: sum w x x^T / W - xbar xbar^T
  best_ref, all_features_ref
and the tolerances of the tests (derivation in mean_errors / cov_errors).
"""
from collections import namedtuple

import numpy as np

Moments = namedtuple("Moments", "w_sum neff Xv Pv XF PF")  # Xv [3], Pv [3,3], XF [2,nf], PF [4,nf] (column-major 2x2)
TWO_PI = 2.0 * np.pi


def pi2pi(a):
    """slam.h:816-829 on float64 arrays."""
    a = np.fmod(np.asarray(a, dtype=np.float64), TWO_PI)
    a = np.where(a > np.pi, a - TWO_PI, a)
    return np.where(a < -np.pi, a + TWO_PI, a)


def stack(parts):
    """Particle lists of tests/pf_builders.py ([w, Xv, Pv, XF, PF] each) -> float64 arrays of the stored values."""
    n = len(parts)
    nf = np.asarray(parts[0][3]).size // 2
    w = np.array([float(p[0]) for p in parts], dtype=np.float64)
    X = np.array([np.asarray(p[1], dtype=np.float64) for p in parts]).reshape(n, 3)
    P = np.array([np.asarray(p[2], dtype=np.float64).reshape(3, 3) for p in parts]).reshape(n, 3, 3)
    XF = np.array([np.asarray(p[3], dtype=np.float64).reshape(2, nf, order="F") for p in parts]).reshape(n, 2, nf)
    PF = np.array([np.asarray(p[4], dtype=np.float64).reshape(4, nf, order="F") for p in parts]).reshape(n, 4, nf)
    return w, X, P, XF, PF


def download(shard):
    """The set as the handle holds it, one get_particle per particle."""
    return stack([list(shard.get_particle(i)) for i in range(shard.n_local)])


def _outer2(d):
    """[n,2,nf] -> [n,4,nf]: d d^T column-major (e = r + 2c)."""
    return np.stack([d[:, 0] * d[:, 0], d[:, 1] * d[:, 0], d[:, 0] * d[:, 1], d[:, 1] * d[:, 1]], axis=1)


def _pose_residual(X, m):
    return np.stack([X[:, 0] - m[0], X[:, 1] - m[1], pi2pi(X[:, 2] - m[2])], axis=1)


def estimate_ref(w, X, P, XF, PF):
    W = float(np.sum(w))
    neff = W * W / float(np.sum(w * w))
    with np.errstate(all="ignore"):
        m = np.array([np.sum(w * X[:, 0]) / W, np.sum(w * X[:, 1]) / W,
                      np.arctan2(np.sum(w * np.sin(X[:, 2])), np.sum(w * np.cos(X[:, 2])))])
        d = _pose_residual(X, m)
        Pv = np.einsum("n,nij->ij", w, P + d[:, :, None] * d[:, None, :]) / W
        mf = np.einsum("n,ncf->cf", w, XF) / W
        df = XF - mf[None]
        Pf = np.einsum("n,nef->ef", w, PF + _outer2(df)) / W
    if not (W > 0 and np.isfinite(W)):
        neff, m, Pv, mf, Pf = np.nan, m * np.nan, Pv * np.nan, mf * np.nan, Pf * np.nan
    return Moments(W, neff, m, Pv, mf, Pf)


def estimate_blocks_ref(w, X, P, XF, PF, blocks):
    """Split the set into `blocks` equal blocks; each gives (W, mean r, S1 = sum w (x - r), S2 = sum w (P + (x - r)(x - r)^T))
    about its own mean; merge in block order.  Moving a block to the merged mean r' by s = r' - r:
    S1' = S1 - W s, S2' = S2 - s S1^T - S1 s^T + W s s^T (Chan's update when S1 = 0); the merged heading is the circular
    mean of the merged sin / cos sums, residuals wrapped."""
    n = w.shape[0]
    assert n % blocks == 0
    L = n // blocks
    state = None
    for b in range(blocks):
        sl = slice(b * L, (b + 1) * L)
        wb, Xb = w[sl], X[sl]
        Wb = float(np.sum(wb))
        ss, sc = float(np.sum(wb * np.sin(Xb[:, 2]))), float(np.sum(wb * np.cos(Xb[:, 2])))
        rb = np.array([np.sum(wb * Xb[:, 0]) / Wb, np.sum(wb * Xb[:, 1]) / Wb, np.arctan2(ss, sc)])
        d = _pose_residual(Xb, rb)
        S1b = np.einsum("n,ni->i", wb, d)
        S2b = np.einsum("n,nij->ij", wb, P[sl] + d[:, :, None] * d[:, None, :])
        mfb = np.einsum("n,ncf->cf", wb, XF[sl]) / Wb
        M2b = np.einsum("n,nef->ef", wb, PF[sl] + _outer2(XF[sl] - mfb[None]))
        cur = dict(W=Wb, W2=float(np.sum(wb * wb)), ss=ss, sc=sc, r=rb, S1=S1b, S2=S2b, mf=mfb, M2=M2b)
        if state is None:
            state = cur
            continue
        a = state
        Wab = a["W"] + Wb
        frac = Wb / Wab
        ss, sc = a["ss"] + cur["ss"], a["sc"] + cur["sc"]
        rn = np.array([a["r"][0] + (rb[0] - a["r"][0]) * frac, a["r"][1] + (rb[1] - a["r"][1]) * frac, np.arctan2(ss, sc)])

        def moved(g):
            s = rn - g["r"]
            s[2] = pi2pi(s[2])
            S1 = g["S1"] - g["W"] * s
            S2 = g["S2"] - np.outer(s, g["S1"]) - np.outer(g["S1"], s) + g["W"] * np.outer(s, s)
            return S1, S2

        (S1a, S2a), (S1c, S2c) = moved(a), moved(cur)
        dlt = cur["mf"] - a["mf"]
        M2 = a["M2"] + cur["M2"] + _outer2(dlt[None])[0] * (a["W"] * frac)
        state = dict(W=Wab, W2=a["W2"] + cur["W2"], ss=ss, sc=sc, r=rn, S1=S1a + S1c, S2=S2a + S2c,
                     mf=a["mf"] + dlt * frac, M2=M2)
    W = state["W"]
    return Moments(W, W * W / state["W2"], state["r"], state["S2"] / W, state["mf"], state["M2"] / W)


def estimate_raw_ref(w, X, P, XF, PF, acc=np.float64):
    """Uncentred accumulation in `acc`: E[x x^T] - xbar xbar^T.  What a kernel that skips the centring would return."""
    w, X, P, XF, PF = (a.astype(acc) for a in (w, X, P, XF, PF))
    W = np.sum(w)
    m = np.array([np.sum(w * X[:, 0]) / W, np.sum(w * X[:, 1]) / W,
                  np.arctan2(np.sum(w * np.sin(X[:, 2])), np.sum(w * np.cos(X[:, 2])))], dtype=acc)
    Xr = X.copy()
    Xr[:, 2] = m[2] + pi2pi(X[:, 2] - m[2]).astype(acc)
    mr = np.einsum("n,ni->i", w, Xr) / W  # (the residuals' own mean, so that only the rounding differs from estimate_ref)
    Pv = np.einsum("n,nij->ij", w, P + Xr[:, :, None] * Xr[:, None, :]) / W - np.outer(mr, mr)
    mf = np.einsum("n,ncf->cf", w, XF) / W
    Pf = np.einsum("n,nef->ef", w, PF + _outer2(XF)) / W - _outer2(mf[None])[0]
    return Moments(float(W), float(W * W / np.sum(w * w)), m.astype(np.float64), Pv.astype(np.float64),
                   mf.astype(np.float64), Pf.astype(np.float64))


def best_ref(w, pick="max"):
    """First maximum (minimum) among the weights that are not NaN; 0 if there is none (slam.h:505-506's 'first')."""
    w = np.asarray(w, dtype=np.float64)
    ok = ~np.isnan(w)
    if not ok.any():
        return 0
    cand = np.nonzero(ok)[0]
    v = w[cand]
    best = v.max() if pick == "max" else v.min()
    return int(cand[np.nonzero(v == best)[0][0]])


def all_features_ref(XF):
    """slam.h:531-536: [n,2,nf] -> 2 x (n nf), particle p's block at column p nf."""
    n, _, nf = XF.shape
    return np.ascontiguousarray(XF.transpose(1, 0, 2).reshape(2, n * nf))


# ------------------------------------------------------------------------------------------------ tolerances
EPS32 = 2.0 ** -23


def mean_errors(got, ref, dtype, heading=None):
    """(error, bound) elementwise.  The engine accumulates in float64 and rounds ONCE to the handle's dtype: f32 within one
    rounding of the reference, given two (2 eps |ref|); f64 within 1e-12 of the largest magnitude (the float64 sums of both
    sides are good to ~1e-15 of it).  `heading`: index of an angle, compared modulo 2 pi."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = got - ref
    if heading is not None:
        err = err.copy()
        err[heading] = pi2pi(err[heading])
    if np.dtype(dtype) == np.float32:
        bound = 2.0 * EPS32 * np.abs(ref)
    else:
        bound = np.full(ref.shape, 1e-12 * max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0))
    return np.abs(err), bound


def cov_errors(got, ref, dtype):
    """Covariances: 1e-9 of the array's largest entry (centred float64 accumulation is good to ~1e-14 of it; an uncentred
    one far from the origin is not), plus the f32 output rounding where the handle is f32."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = float(np.max(np.abs(ref))) if ref.size else 0.0
    bound = np.full(ref.shape, 1e-9 * top)
    if np.dtype(dtype) == np.float32:
        bound = bound + 2.0 * EPS32 * np.abs(ref)
    return np.abs(got - ref), bound


def _judge(tag, name, err, bound):
    if err.size == 0:
        return
    worst = int(np.argmax(err - bound))  # the entry nearest to (or furthest past) its bound
    print(f"[estimate] {tag} {name}: err {float(err.reshape(-1)[worst]):.3e} against bound {float(bound.reshape(-1)[worst]):.3e}"
          f" at the tightest entry; largest err {float(err.max()):.3e}")
    assert np.all(err <= bound), (tag, name, float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]))


def assert_moments(tag, got, ref, dtype, want_map=True):
    """got: an Estimate of the engine; ref: Moments.  Figures are printed before they are judged."""
    assert abs(got.w_sum - ref.w_sum) <= 1e-12 * abs(ref.w_sum), (tag, got.w_sum, ref.w_sum)
    assert abs(got.neff - ref.neff) <= 1e-12 * abs(ref.neff), (tag, got.neff, ref.neff)
    _judge(tag, "Xv", *mean_errors(got.Xv, ref.Xv, dtype, heading=2))
    _judge(tag, "Pv", *cov_errors(got.Pv, ref.Pv, dtype))
    if want_map:
        _judge(tag, "XF", *mean_errors(got.XF, ref.XF, dtype))
        _judge(tag, "PF", *cov_errors(got.PF, ref.PF, dtype))
