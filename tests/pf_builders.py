"""Shared builders of the particle-filter tests (test_pf_gpu.py, test_pf_edges_gpu.py, test_pf_edges_cpu.py).

Three kinds of input:
  * `random_particles`: well-conditioned particles spread over 2 m (the convenient shapes of test_pf_gpu.py);
  * the TIGHT CLOUD (`tight_particles`, `proposal_case`): a particle set like a filter's after a resample, so that a
    product of up to 65 likelihood factors stays far inside the range of f32 for EVERY particle;
  * EXACT RESAMPLE INPUTS (`exact_resample_case`): integer weights over a power-of-two denominator, so that the sum,
    1/sum, the normalisation and every partial sum are exact in f32 and f64 and keep[] is decided by integer arithmetic.
test_pf_edges_cpu.py proves the stated properties of the last two on the oracle alone.
"""
from fractions import Fraction

import numpy as np

from helpers import assert_close
from pyoracle import Oracle, REF_EXACT

DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float32): 2e-5, np.dtype(np.float64): 1e-12}


def random_particles(np_, nf, dtype, seed=0):
    """Well-conditioned particles around a common pose with nf mapped features each."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(np_):
        Xv = np.array([rng.normal(0, 2.0), rng.normal(0, 2.0), rng.normal(0.2, 0.05)], dtype=dtype)
        A = rng.normal(size=(3, 3)) * np.array([0.3, 0.3, 0.02])[:, None]
        Pv = np.asfortranarray((A @ A.T + np.diag([0.05, 0.05, 1e-4])).astype(dtype))
        XF = np.asfortranarray(rng.uniform(-300, 300, size=(2, nf)).astype(dtype))
        PF = np.zeros((4, nf), dtype=dtype, order="F")
        for f in range(nf):
            B = rng.normal(size=(2, 2)) * 0.5
            PF[:, f] = (B @ B.T + 0.2 * np.eye(2)).reshape(-1, order="F")
        w = dtype(rng.uniform(0.5, 1.5) / np_)
        parts.append([w, Xv, Pv, XF, PF])
    return parts


def shard_from(parts, nfcap, dtype, quirks=REF_EXACT):
    from conan_slam_amd.pf import ParticleShard

    sh = ParticleShard(len(parts), nfcap, dtype=dtype, quirks=quirks)
    for i, (w, Xv, Pv, XF, PF) in enumerate(parts):
        sh.set_particle(i, w, Xv, Pv, XF, PF)
    return sh


def obs_for(parts, idf, dtype, seed=3):
    """Observations of the listed features as seen from the mean particle pose (+ noise)."""
    rng = np.random.default_rng(seed)
    X = np.mean([p[1] for p in parts], axis=0).astype(np.float64)
    XF = parts[0][3].astype(np.float64)
    Z = np.zeros((2, len(idf)))
    for i, f in enumerate(idf):
        dx, dy = XF[0, f - 1] - X[0], XF[1, f - 1] - X[1]
        Z[0, i] = np.hypot(dx, dy) + rng.normal() * 0.2
        Z[1, i] = np.arctan2(dy, dx) - X[2] + rng.normal() * 0.01
    return np.asfortranarray(Z.astype(dtype))


def compare(sh, parts, dtype, tag, wtol=None):
    tol = TOL[np.dtype(dtype)]
    for i, (w, Xv, Pv, XF, PF) in enumerate(parts):
        gw, gX, gP, gXF, gPF = sh.get_particle(i)
        assert_close(f"{tag} Xv[{i}]", gX, Xv, tol)
        assert_close(f"{tag} Pv[{i}]", gP, Pv, tol)
        assert_close(f"{tag} XF[{i}]", gXF, XF, tol)
        assert_close(f"{tag} PF[{i}]", gPF, PF, tol)
        rel = abs(float(gw) - float(w)) / max(abs(float(w)), 1e-300)
        assert rel <= (wtol if wtol is not None else 50 * tol), (tag, i, float(gw), float(w))


# ------------------------------------------------------------------------------------------------
# the tight cloud
# ------------------------------------------------------------------------------------------------
TRUE_POSE = (0.0, 0.0, 0.2)
Q_CTRL = np.diag([0.18, 6e-4])
R_OBS = np.diag([0.08, 0.0024])
PREDICT = (83.33, 0.03, 73.0, 0.01)  # v, swa, wheel base, dt of the fused-step cases


def tight_particles(np_, nf, dtype, seed=0):
    """A cloud like a filter's after a resample: ONE map (uniform in +-300 m) that every particle carries with 0.3 m of
    jitter, poses within 0.3 m / 0.006 rad of (0, 0, 0.2), Pv and PF as random_particles builds them, w = 1/np.
    -> (particles, the common map 2 x nf)."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-300, 300, size=(2, nf))
    parts = []
    for _ in range(np_):
        Xv = np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), rng.normal(0.2, 0.006)], dtype=dtype)
        A = rng.normal(size=(3, 3)) * np.array([0.3, 0.3, 0.02])[:, None]
        Pv = np.asfortranarray((A @ A.T + np.diag([0.05, 0.05, 1e-4])).astype(dtype))
        XF = np.asfortranarray((base + rng.normal(0, 0.3, size=(2, nf))).astype(dtype))
        PF = np.zeros((4, nf), dtype=dtype, order="F")
        for f in range(nf):
            B = rng.normal(size=(2, 2)) * 0.5
            PF[:, f] = (B @ B.T + 0.2 * np.eye(2)).reshape(-1, order="F")
        parts.append([dtype(1.0 / np_), Xv, Pv, XF, PF])
    return parts, base


def advance_pose(pose, v, swa, wb, dt):
    """The noise-free motion model of PF::predict applied to one pose."""
    x, y, phi = pose
    return (x + v * dt * np.cos(swa + phi), y + v * dt * np.sin(swa + phi), phi + v * dt * np.sin(swa) / wb)


def tight_obs(base, idf, dtype, seed=3, pose=TRUE_POSE):
    """Range / bearing of the listed (1-based) features of the common map from `pose`, noise 0.2 m / 0.01 rad."""
    rng = np.random.default_rng(seed)
    Z = np.zeros((2, len(idf)))
    for i, f in enumerate(idf):
        dx, dy = base[0, f - 1] - pose[0], base[1, f - 1] - pose[1]
        Z[0, i] = np.hypot(dx, dy) + rng.normal() * 0.2
        Z[1, i] = np.arctan2(dy, dx) - pose[2] + rng.normal() * 0.01
    return np.asfortranarray(Z.astype(dtype))


def shuffled_idf(nf, m, rng):
    """m distinct 1-based features in shuffled order, feature 1 and feature nf among them (the two ends of the
    xf[nf][2][np] / pf[nf][4][np] strides)."""
    assert 2 <= m <= nf
    inner = rng.permutation(np.arange(2, nf))[: m - 2]
    idf = np.concatenate([[1, nf], inner])
    return rng.permutation(idf).astype(np.int32)


class ProposalCase:
    """Inputs of one sampleProposal call (optionally behind a predict) on a tight cloud."""

    def __init__(self, m, np_, dtype, nf=None, seed=None, predict=False):
        self.m, self.np_, self.dtype, self.predict = m, np_, dtype, predict
        self.nf = nf if nf is not None else m + 3
        self.seed = seed if seed is not None else 1000 * m + np_
        self.parts, self.base = tight_particles(np_, self.nf, dtype, self.seed)
        rng = np.random.default_rng(self.seed + 77)
        self.idf = shuffled_idf(self.nf, m, rng)
        pose = advance_pose(TRUE_POSE, PREDICT[0], PREDICT[1], PREDICT[2], PREDICT[3]) if predict else TRUE_POSE
        self.Z = tight_obs(self.base, self.idf, dtype, seed=self.seed + 78, pose=pose)
        self.R = np.asfortranarray((R_OBS * (6.0 if m >= 64 else 1.0)).astype(dtype))
        self.Q = np.asfortranarray(Q_CTRL.astype(dtype))
        self.normals = rng.normal(size=(3, np_)).astype(dtype)

    def __repr__(self):
        return f"ProposalCase(m={self.m}, np={self.np_}, nf={self.nf}, {np.dtype(self.dtype).name}, predict={self.predict})"


def copy_parts(parts, dt):
    return [[dt(p[0])] + [np.array(a, dtype=dt, order="F") for a in p[1:]] for p in parts]


def oracle_chain(case, dt, quirks=REF_EXACT, feature_update=False):
    """[predict ->] sampleProposal [-> featureUpdate] of every particle of `case` on the CPU oracle in precision `dt`
    (the inputs are the case's own-dtype values converted, as the f64 fairness reference of test_pf_gpu.py takes them)."""
    o = Oracle(dt, quirks)
    ps = copy_parts(case.parts, dt)
    Z = np.asfortranarray(case.Z.astype(dt))
    R = np.asfortranarray(case.R.astype(dt))
    for i, p in enumerate(ps):
        if case.predict:
            o.pf_predict(p[1], p[2], PREDICT[0], PREDICT[1], case.Q.astype(dt), PREDICT[2], PREDICT[3])
        w = np.array([p[0]], dtype=dt)
        o.pf_sample_proposal(w, p[1], p[2], p[3], p[4], Z, case.idf, R, case.normals[:, i].astype(dt))
        p[0] = w[0]
        if feature_update:
            o.pf_feature_update(p[1], p[3], p[4], Z, case.idf, R)
    return ps


# every (m, np) the GPU file gives to the proposal kernel, with the map size and whether a predict rides along;
# test_pf_edges_cpu.py checks the weight range of each of them in both dtypes
PROPOSAL_M = [8, 9, 16, 17]
PROPOSAL_NP = [1, 7, 8, 9, 17]
STAGING_NP, STAGING_NF = 9, 68
STAGING_M = [64, 65, 8]  # in this order on ONE shard: no growth, the first growth of dObs / dIdx, back to one chunk
FUSED_NP = 73
FUSED_M = [9, 17]


def proposal_case_keys():
    keys = [(m, n, None, False) for m in PROPOSAL_M for n in PROPOSAL_NP]
    keys += [(m, STAGING_NP, STAGING_NF, False) for m in STAGING_M]
    keys += [(m, FUSED_NP, None, True) for m in FUSED_M]
    return keys


def proposal_case(key, dtype):
    m, n, nf, predict = key
    return ProposalCase(m, n, dtype, nf=nf, predict=predict)


def weight_errors(wg, wc, wh):
    """Relative errors against the f64 oracle: (device max, device median, CPU max, CPU median)."""
    wg, wc, wh = (np.asarray(a, dtype=np.float64) for a in (wg, wc, wh))
    e_gpu, e_cpu = np.abs(wg - wh) / wh, np.abs(wc - wh) / wh
    return float(e_gpu.max()), float(np.median(e_gpu)), float(e_cpu.max()), float(np.median(e_cpu))


def assert_weights_fair(tag, wg, wc, wh, dtype):
    """The weight rule of test_sample_proposal / test_config3 over EVERY particle (none is left out): f32 maximum and
    median relative error against the f64 oracle within 4x the CPU f32 oracle's (+1e-6 / +1e-7); f64 within 1e-9 of the
    oracle relative to its largest weight.  The figures are printed before they are judged."""
    wg, wc, wh = (np.asarray(a, dtype=np.float64) for a in (wg, wc, wh))
    assert np.all(np.isfinite(wg)) and np.all(wh > 0), tag
    gmax, gmed, cmax, cmed = weight_errors(wg, wc, wh)
    print(f"[weights] {tag} {np.dtype(dtype).name}: device max {gmax:.3e} median {gmed:.3e}; "
          f"cpu max {cmax:.3e} median {cmed:.3e}; f64-oracle range [{wh.min():.3e}, {wh.max():.3e}]")
    if np.dtype(dtype) == np.float64:
        assert np.abs(wg - wc).max() <= 1e-9 * np.abs(wc).max(), (tag, float(np.abs(wg - wc).max()), float(np.abs(wc).max()))
    else:
        assert gmax <= 4.0 * cmax + 1e-6, (tag, gmax, cmax)
        assert gmed <= 4.0 * cmed + 1e-7, (tag, gmed, cmed)


# ------------------------------------------------------------------------------------------------
# exact resample inputs
# ------------------------------------------------------------------------------------------------
class ExactResampleCase:
    """n integer weights k[i] >= 0 with sum G = 8 * 2^ceil(log2 n), and n strata positions t[c] / G with t[c] an integer
    inside stratum c: [c/n, (c+1)/n).  Everything the resample computes is then an integer over G:
        normalised weight  k[i] / G        running sum  K[i] / G        keep[c] = first i with K[i] > t[c]  (none: 0)
    and exact in f32 (G <= 2^18) and f64.  The raw weights are k * 8 / G (sum 8: the normalisation has work to do).
    About half of the partial sums are PUT on strata positions (ties select[c] == cum[i]); others are repeated (weights
    of zero, runs of them).  Unless `end`, every partial sum but the last is at or below the start of the last stratum,
    so the last slot keeps the last particle: a running sum that is wrong in its last elements cannot go unnoticed.
    `end`: the last stratum's position is 1.0 (what stratified_random gives for u = nextafter(1, 0)), not below
    cum[n-1] = 1.0, and the last weights are zeros: the slot finds nothing and keeps particle 0."""

    def __init__(self, n, seed=0, end=False, uniform=False):
        self.n, self.end, self.seed = n, end, seed
        rng = np.random.default_rng(10_000 + 31 * n + seed)
        p2 = 1
        while p2 < n:
            p2 *= 2
        self.pow2 = p2 == n
        G = self.G = 8 * p2
        c = np.arange(n, dtype=np.int64)
        lo = -((-c * G) // n)             # ceil(c G / n): first integer position of stratum c
        hi = -((-(c + 1) * G) // n) - 1   # last integer position below (c + 1) G / n
        assert np.all(hi >= lo)
        if uniform:
            assert self.pow2
            self.t = lo.copy()            # u = 0 everywhere: every position but the first ties with a running sum
            self.k = np.full(n, G // n, dtype=np.int64)
            self.K = np.cumsum(self.k)
        else:
            self.t = rng.integers(lo, hi + 1)
            if end or n == 1:             # (one particle: the only position that can tie with cum[0] = 1 is 1 itself)
                self.t[n - 1] = G
            nfree = n - 1
            cap = int(lo[n - 1])
            n_tie = (nfree + 1) // 2
            free = list(self.t[rng.choice(n - 1, size=n_tie, replace=False)]) if nfree else []
            rest = nfree - n_tie
            n_rep = rest // 2
            if n_rep:                     # repeated partial sums = weights of zero; one value four times over = a run
                reps = rng.choice(np.array(free), size=n_rep)
                if n_rep >= 4:
                    reps[:3] = reps[3]
                free += list(reps)
            free += list(rng.integers(0, cap + 1, size=rest - n_rep))
            K = np.sort(np.array(free, dtype=np.int64))
            if end and n >= 4:
                K[-2:] = G                # the last three partial sums are 1: two trailing weights of zero
            self.K = np.concatenate([K, [G]]).astype(np.int64)
            self.k = np.diff(self.K, prepend=0)
        assert self.k.min() >= 0 and int(self.k.sum()) == G and np.all(np.diff(self.t) > 0)
        keep = np.searchsorted(self.K, self.t, side="right")
        self.beyond = keep >= n           # slots whose position is not below the last running sum
        keep[self.beyond] = 0
        self.keep = keep.astype(np.int32)
        self.ties = int(np.isin(self.t, self.K).sum())
        self.neff = float(Fraction(G * G, int((self.k * self.k).sum())))

    def raw_weights(self, dtype):
        return (self.k.astype(np.float64) * (8.0 / self.G)).astype(dtype)

    def norm_weights(self, dtype):
        return (self.k.astype(np.float64) / self.G).astype(dtype)

    def cum_weights(self, dtype):
        return (self.K.astype(np.float64) / self.G).astype(dtype)

    def select(self, dtype):
        return (self.t.astype(np.float64) / self.G).astype(dtype)

    def uniforms(self, dtype):
        """Power-of-two n: the strata offsets (multiples of 1/8; nextafter(1, 0) for a position of 1.0) from which
        stratified_random builds exactly select()."""
        assert self.pow2
        u = ((self.t - 8 * np.arange(self.n)) / 8.0).astype(dtype)
        u[u >= 1] = np.nextafter(np.dtype(dtype).type(1), np.dtype(dtype).type(0))
        return u

    def __repr__(self):
        return f"ExactResampleCase(n={self.n}, end={self.end}, ties={self.ties})"


RESAMPLE_NP = [1, 2, 8, 9, 10, 255, 256, 257, 8192, 8193, 8199, 16384, 16389]
RESAMPLE_END_NP = [8, 8192, 16384]   # one LDS stage (8 and the full 8192) and the global-memory search
DECISION_NP = [1, 2, 8, 256, 8192]   # powers of two: uniform weights 1/np are exact
SHARDED = [(2, 8192), (4, 8192), (2, 16400), (4, 16400)]


def resample_case_keys():
    sharded_only = sorted({n for _, n in SHARDED} - set(RESAMPLE_NP))
    return [(n, False) for n in RESAMPLE_NP] + [(n, True) for n in RESAMPLE_END_NP] + [(n, False) for n in sharded_only]


def tagged_records(n, w, dtype, nf=1):
    """n packed particle records [w, xv(3), pv(9), xf(2 nf), pf(4 nf)] whose every field names its particle: the index
    itself in xv[0] (exact in f32 up to 2^24), values derived from it elsewhere."""
    i = np.arange(n, dtype=np.float64)
    rec = np.zeros((n, 13 + 6 * nf), dtype=np.float64)
    rec[:, 0] = w
    rec[:, 1] = i
    rec[:, 2] = 0.5 * (i % 7)
    rec[:, 3] = 0.125 * (i % 5) - 0.25
    for e in range(9):
        rec[:, 4 + e] = (i % 11) * 0.25 + e
    for e in range(6 * nf):
        rec[:, 13 + e] = i + 0.25 * (e + 1)
    out = rec.astype(dtype)
    assert np.array_equal(out.astype(np.float64), rec)
    return out
