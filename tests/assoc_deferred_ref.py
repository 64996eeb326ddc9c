"""Reference side of cslam_ekf_associate_deferred (test_assoc_deferred_cpu.py, test_assoc_deferred_gpu.py).

  * `decide_blocks`: the DECOMPOSED rule the two kernels implement -- per block of 256 features the smallest gated
    non-NaN nd with the lowest index holding it and the smallest nis, combined in block order with a strict `<` -- in plain
    numpy, with deliberate faults for the negative controls.  test_assoc_deferred_cpu.py proves it equal to the sequential
    rule `assoc_builders.decide` (EKF.cpp:235-326).
  * `deferred_block` / `panels_of`: the landmark's 2 x 2 block of P = Ps - Wp diag(s) Wp^T from the stored matrix, the
    pending panels and their signs.
  * `Pending`: a state with work pending -- a sparse map, two batch updates of 8 features each with a heading
    observation between them (variant 'pos'; 'la': three updates of 12, what a look-ahead window accepts; 'neg': one
    heading observation on P22 + R < 0, whose column enters with the opposite sign) -- applied by the oracle to get the
    true P, and observations built from that state: own-feature
    observations of updated and untouched features, observations far from every feature, and FLIP observations whose
    decision under the stale landmark blocks (the 2 x 2 blocks before the steps; 'neg': the blocks with the column's
    sign dropped) differs from the decision under the true P.  Every observation is decisive under the true P.
The seeds below were found by `search_seed_pending` at the end of this file.
"""
import numpy as np

from assoc_builders import GATES, R_OBS, Case, decide, pair_reference, predicted, sparse_state
from helpers import OracleState
from pyoracle import TEXTBOOK

BLOCK = 256  # features per workgroup of ekf_assoc_pair_kernel


# ------------------------------------------------------------------------------------------------
# the decomposed rule
# ------------------------------------------------------------------------------------------------
def block_partials(nis_row, nd_row, g1, lo, hi, fault=None):
    """(smallest gated non-NaN nd, lowest 1-based feature holding it or 0, smallest nis) of features lo .. hi - 1"""
    n_, d_ = nis_row[lo:hi], nd_row[lo:hi]
    gated = n_ < g1
    cand = np.where(gated & ~np.isnan(d_), d_, np.inf)
    pn = cand.min()
    pj = lo + int(np.argmin(cand)) + 1 if pn < np.inf else 0        # (argmin: the first of equal minima)
    pool = n_
    if fault == "outer_ungated_only":
        pool = n_[~gated]
    elif fault == "partial_nis_gated_only":
        pool = n_[gated]
    pool = pool[~np.isnan(pool)]
    return pn, pj, (pool.min() if pool.size else np.inf)


def decide_blocks(nis, nd, g1, g2, block=BLOCK, fault=None):
    """-> (idf[m], kind[m]).  fault: None, 'last_block_tie' (`<=` between blocks: the last block wins a tie),
    'outer_ungated_only', 'partial_nis_gated_only'."""
    m, nf = nis.shape
    idf, kind = np.zeros(m, np.int32), np.zeros(m, np.int32)
    for i in range(m):
        nbest, jbest, outer = np.inf, 0, np.inf
        for lo in range(0, nf, block):
            pn, pj, po = block_partials(nis[i], nd[i], g1, lo, min(nf, lo + block), fault)
            if (pn <= nbest if fault == "last_block_tie" else pn < nbest) and pj:
                nbest, jbest = pn, pj
            if po < outer:
                outer = po
        idf[i] = jbest
        kind[i] = 1 if jbest else (2 if outer > g2 else 0)
    return idf, kind


# ------------------------------------------------------------------------------------------------
# the deferred block
# ------------------------------------------------------------------------------------------------
def deferred_block(Ps, Wp, s, f):
    """2 x 2 block of 0-based feature f: Ps - sum_c s_c w_c w_c^T over the pending columns (rows fx, fx + 1 of Wp)"""
    fx = 3 + 2 * f
    w = Wp[fx:fx + 2, :]
    return Ps[fx:fx + 2, fx:fx + 2] - (w * s[None, :]) @ w.T


def _h_rows(X, idf):
    n = X.shape[0]
    H = np.zeros((2 * len(idf), n))
    for i, f in enumerate(idf):
        fx = 3 + 2 * (int(f) - 1)
        dx, dy = X[fx] - X[0], X[fx + 1] - X[1]
        d2 = dx * dx + dy * dy
        d = np.sqrt(d2)
        H[2 * i, [0, 1, fx, fx + 1]] = [-dx / d, -dy / d, dx / d, dy / d]
        H[2 * i + 1, [0, 1, 2, fx, fx + 1]] = [dy / d2, -dx / d2, -1.0, -dy / d2, dx / d2]
    return H


def panels_of(steps, X0, P0, R, sig2_heading):
    """f64 panels of a list of steps applied to (X0, P0): -> (Wp [n, kp], s [kp], P true).  A batch update with rows H
    contributes W = P H^T L^-T (S = H P H^T + R (x) I = L L^T, so W W^T = P H^T S^-1 H P, slam.h:235-266) with s = +1; a
    heading observation the column P[:, 2] / sqrt|S| with s = sign(S), S = P22 + sig2 (EKF.cpp:328-352).  X moves as the
    filter moves it (H is evaluated at the current X)."""
    X, P = np.array(X0, dtype=np.float64), np.array(P0, dtype=np.float64)
    cols, signs = [], []
    for st in steps:
        if st[0] == "update":
            Z, idf = np.asarray(st[1], dtype=np.float64), st[2]
            H = _h_rows(X, idf)
            S = H @ P @ H.T + np.kron(np.eye(len(idf)), np.asarray(R, dtype=np.float64))
            L = np.linalg.cholesky(0.5 * (S + S.T))
            W = np.linalg.solve(L, H @ P).T
            V = np.zeros(2 * len(idf))
            for i, f in enumerate(idf):
                zp = predicted(X, int(f) - 1, np.float64)
                V[2 * i], V[2 * i + 1] = Z[0, i] - zp[0], Z[1, i] - zp[1]
            X = X + W @ np.linalg.solve(L, V)
            cols.append(W)
            signs += [1.0] * W.shape[1]
        else:
            S = P[2, 2] + sig2_heading
            w = P[:, 2] / np.sqrt(abs(S))
            X = X + P[:, 2] / S * (st[1] - X[2])
            cols.append(w[:, None])
            signs.append(1.0 if S > 0 else -1.0)
        sg = np.array(signs[-cols[-1].shape[1]:])
        P = P - (cols[-1] * sg[None, :]) @ cols[-1].T
    return np.concatenate(cols, axis=1), np.array(signs), P


# ------------------------------------------------------------------------------------------------
# a state with work pending
# ------------------------------------------------------------------------------------------------
SIG2_HEADING = (0.01 * np.pi / 180.0) ** 2   # the heading variance of EKF.cpp:328-352
# variant -> the batch updates (1-based features) and whether a heading observation stands between the first two.
#   'pos'  two updates of 8 features and a heading observation (a pending column with s = +1)
#   'la'   three updates of 12 features and no heading step: what a look-ahead window accepts (more than 8 observations,
#          no heading column pending); an odd number, so that with CSLAM_LOOKAHEAD=1 the last one is still queued
#   'neg'  no update: one heading observation on P22 + R < 0
UPDATES = {"pos": [np.arange(1, 9, dtype=np.int32), np.arange(9, 17, dtype=np.int32)],
           "la": [np.arange(1, 13, dtype=np.int32), np.arange(13, 25, dtype=np.int32), np.arange(25, 37, dtype=np.int32)],
           "neg": []}
FLIP_FEATS = (2, 10, 5, 12)                   # 1-based, updated: targets nis = FLIP_TARGETS under the true P
FLIP_TARGETS = (12.5, 12.5, 6.5, 12.5)        # 12.5: between gate1 and gate2 of both pairs; 6.5: of the first pair only
NEG_N, NEG_P22 = 40, -0.5
NEG_SCALES = (1e-2, 1e-1, 1.0, 4.0)           # pose scale of the covariance: strength of the pose-landmark correlations
NEG_GAP = 0.25                                # a decision counts as depending on the sign when both nis lie this far from gate1
# seeds found by search_seed_pending: {(nf, dtype name, variant): seed}
PENDING_SEEDS = {(65, "float32", "pos"): 0, (65, "float64", "pos"): 0, (257, "float32", "pos"): 0,
                 (257, "float64", "pos"): 0, (65, "float32", "la"): 0, (65, "float64", "la"): 0,
                 (257, "float32", "la"): 0, (257, "float64", "la"): 0, (NEG_N, "float32", "neg"): 0,
                 (NEG_N, "float64", "neg"): 0}


def symmetric_lower(P):
    """P with its upper triangle replaced by the lower one (what every reader of the engine takes)"""
    L = np.tril(np.asarray(P))
    return np.asfortranarray(L + np.tril(L, -1).T)


def stale_blocks(P_true, P_before, negative=False):
    """P_true with every landmark's 2 x 2 block taken from the state before the steps -- what a read that ignores the
    pending panels sees (the pose rows live in the stripe and are current).  negative: the blocks with the sign of the
    column dropped, Ps - w w^T in place of Ps + w w^T = 2 Ps - P_true."""
    P = np.array(P_true, dtype=np.float64)
    B = np.asarray(P_before, dtype=np.float64)
    for fx in range(3, P.shape[0], 2):
        blk = B[fx:fx + 2, fx:fx + 2]
        P[fx:fx + 2, fx:fx + 2] = (2.0 * blk - P[fx:fx + 2, fx:fx + 2]) if negative else blk
    return P


class Pending:
    """steps: [('update', Z, idf) | ('heading', phi)] on (X0, P0); (X1, P1) the oracle's state after them (dtype);
    Z: the observations; own / far / flips: their column indices."""

    def __init__(self, nf, dtype, seed, variant="pos", pose_scale=None):
        negative = variant == "neg"
        self.nf, self.dtype, self.negative, self.variant = nf, np.dtype(dtype), negative, variant
        self.R = R_OBS
        rng = np.random.default_rng(90_000 + 1000 * nf + seed)
        if negative:
            X0, P0 = sparse_state(nf, 17_000 + seed, pose_scale=pose_scale)
            P0[2, 2] = NEG_P22
            self.steps = [("heading", float(X0[2]) + 1e-3)]
        else:
            X0, P0 = sparse_state(nf, 17_000 + seed)
            self.steps = []
        self.X0 = np.array(X0, dtype=dtype)
        self.P0 = np.array(P0, dtype=dtype, order="F")
        orc = OracleState(self.X0, self.P0, self.dtype, TEXTBOOK)
        if not negative:
            for k, feats in enumerate(UPDATES[variant]):
                if k == 1 and variant == "pos":
                    self.steps.append(("heading", float(orc.x()[2]) + 2e-3))
                    self._apply_one(orc, self.steps[-1])
                Zu = np.stack([predicted(orc.x(), int(f) - 1, dtype) + rng.normal(size=2) * (0.1, 0.004) for f in feats], axis=1)
                self.steps.append(("update", np.asfortranarray(Zu.astype(dtype)), feats))
                self._apply_one(orc, self.steps[-1])
        else:
            self._apply_one(orc, self.steps[0])
        self.X1, self.P1 = orc.x(), symmetric_lower(orc.p())
        self._observations(rng)

    def _apply_one(self, eng, st):
        if st[0] == "update":
            eng.update(st[1], self.R.astype(self.dtype), st[2], True)
        else:
            eng.observe_heading(st[1], True)

    def apply(self, eng):
        """the steps on an engine (EKF) or an OracleState"""
        for st in self.steps:
            self._apply_one(eng, st)

    def stale(self, P_true=None):
        return stale_blocks(self.P1 if P_true is None else P_true, self.P0, self.negative)

    def _flip_column(self, f, target, gates):
        """the observation of 0-based feature f on a fixed grid of range offsets: non-negative: the one whose nis under
        the true P is nearest the target while its nis under the stale blocks is inside every gate1; negative: the one
        with the widest gap true < gate1 < wrong-sign."""
        zp = predicted(self.X1, f, self.dtype)
        grid = np.linspace(0.02, 8.0, 800)
        Zg = np.stack([zp[0] + grid, np.full_like(grid, zp[1])]).astype(self.dtype)
        Rd = self.R.astype(self.dtype)
        nt = pair_reference(self.X1, self.P1, Zg, Rd)[0][:, f]
        ns = pair_reference(self.X1, self.stale(), Zg, Rd)[0][:, f]
        if self.negative:
            g1 = gates[0][0]
            gap = np.where((nt < g1) & (ns > g1), np.minimum(g1 - nt, ns - g1), -np.inf)
            return None if gap.max() < NEG_GAP else Zg[:, int(np.argmax(gap))].astype(np.float64)
        ok = ns < 0.5 * min(g[0] for g in gates)
        score = np.where(ok, -np.abs(nt - target), -np.inf)
        assert np.isfinite(score.max()), (f, target)
        return Zg[:, int(np.argmax(score))].astype(np.float64)

    def _observations(self, rng):
        nf, dt = self.nf, self.dtype
        upd = [] if self.negative else [0, 8]
        own_feats = upd + sorted({nf - 1, 29, min(63, nf - 1), min(64, nf - 1), 20})
        cols = [predicted(self.X1, f, dt) + rng.normal(size=2) * (0.03, 0.001) for f in own_feats]
        self.own = list(range(len(cols)))
        self.own_feats = own_feats
        far = [np.array([30.0, -0.4]), np.array([25.0, 1.3])]    # the nearest landmarks are 60 m from the pose
        self.far = list(range(len(cols), len(cols) + len(far)))
        cols += far
        self.flips, self.flip_feats = [], []
        targets = zip(range(nf), [None] * nf) if self.negative else zip([f - 1 for f in FLIP_FEATS], FLIP_TARGETS)
        for f, target in targets:
            z = self._flip_column(f, target, GATES[:1] if self.negative else GATES)
            if z is not None:
                self.flips.append(len(cols))
                self.flip_feats.append(f)
                cols.append(z)
            if self.negative and len(self.flips) == 4:
                break
        self.Z = np.asfortranarray(np.stack(cols, axis=1).astype(dt))
        self.gates = GATES[:1] if self.negative else GATES

    def case(self, X=None, P=None, name="pending"):
        """the Case of the observations on a state (default: the oracle's)"""
        return Case(name, "P", self.dtype.type, self.X1 if X is None else X, self.P1 if P is None else symmetric_lower(P),
                    self.Z, self.R, gates=self.gates)

    def stale_decisions(self, gates, X=None, P=None):
        X = self.X1 if X is None else X
        P = self.P1 if P is None else symmetric_lower(P)
        nis, nd = pair_reference(X, self.stale(P), self.Z, self.R.astype(self.dtype))[:2]
        return decide(nis, nd, *gates)[:2]


def check_pending(p, X=None, P=None):
    """What the builder promises, on the oracle's state or on a given one (the GPU test passes the twin's): every
    observation decisive under the true P; own observations find their feature, far ones are new; at least two flips per
    gate pair decide differently under the stale blocks.  -> the Case."""
    c = p.case(X, P)
    tau = c.tau()[0]
    for gates in p.gates:
        mg = c.margins(gates)
        assert np.all(mg >= tau), (p.nf, p.dtype, gates, mg, tau)
        idf, kind, _ = c.decisions(gates)
        assert [int(j) - 1 for j in idf[p.own]] == p.own_feats and np.all(kind[p.own] == 1), (gates, idf[p.own])
        assert np.all(kind[p.far] == 2), (gates, kind[p.far])
        idf_s, kind_s = p.stale_decisions(gates, X, P)
        differs = [i for i in p.flips if (idf_s[i], kind_s[i]) != (idf[i], kind[i])]
        assert len(differs) >= (1 if p.negative else 2), (p.nf, p.dtype, gates, differs)
    return c


# ------------------------------------------------------------------------------------------------
# a scan with all three kinds (the split on the device, the adapter run)
# ------------------------------------------------------------------------------------------------
SPLIT_NF = 65
_SPLIT = {}


def split_scan(dtype=np.float32):
    """On a sparse map: 30 own observations (kind 1), 5 far from everything (kind 2), 5 with their nearest nis between
    gate1 and gate2 (dropped).  -> Case with gates (4, 25), decisive for every observation (f32; built once)."""
    if "case" in _SPLIT:
        return _SPLIT["case"]
    X, P = sparse_state(SPLIT_NF, 18_000)
    Xd, Pd, Rd = np.asarray(X, dtype=dtype), np.asarray(P, dtype=dtype), R_OBS.astype(dtype)
    rng = np.random.default_rng(18_500)
    kinds = [1] * 30 + [2] * 5 + [0] * 5
    feats = rng.permutation(SPLIT_NF)[:40]
    cols = []
    for k, f in zip(kinds, feats):
        zp = predicted(X, int(f), dtype)
        if k == 1:
            cols.append(zp + rng.normal(size=2) * (0.05, 0.002))
        elif k == 2:
            cols.append(np.array([20.0 + 3.0 * len(cols) % 7, zp[1]]))
        else:
            grid = np.linspace(0.1, 12.0, 600)
            Zg = np.stack([zp[0] + grid, np.full_like(grid, zp[1])]).astype(dtype)
            nis = pair_reference(Xd, Pd, Zg, Rd)[0][:, int(f)]
            cols.append(Zg[:, int(np.argmin(np.abs(nis - 12.0)))].astype(np.float64))
    order = rng.permutation(40)
    case = Case("split", "S", dtype, X, P, np.stack(cols, axis=1)[:, order], R_OBS, gates=GATES[:1])
    assert np.all(case.margins(GATES[0]) >= case.tau()[0])
    assert sorted(case.decisions(GATES[0])[1]) == sorted(kinds)
    _SPLIT["case"] = case
    return case


_PENDING = {}


def get_pending(nf, dtype, variant="pos"):
    key = (nf, np.dtype(dtype).name, variant)
    if key not in _PENDING:
        _PENDING[key] = build_pending(nf, dtype, PENDING_SEEDS[key], variant)
    return _PENDING[key]


def build_pending(nf, dtype, seed, variant="pos"):
    if variant != "neg":
        return Pending(nf, dtype, seed, variant)
    for ps in NEG_SCALES:   # scale the pose-landmark correlations until a decision depends on the column's sign
        p = Pending(nf, dtype, seed, "neg", pose_scale=ps)
        if p.flips:
            return p
    raise AssertionError("no decision depends on the sign of the heading column")


def search_seed_pending(nf, dtype, variant="pos", limit=200):
    """First seed from 0 whose builder passes check_pending (numpy reference and the oracle's tau: no device)."""
    for seed in range(limit):
        try:
            check_pending(build_pending(nf, dtype, seed, variant))
        except AssertionError:
            continue
        return seed
    raise RuntimeError("no seed found")
