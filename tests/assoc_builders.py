"""Shared builders of the data-association edge tests (test_assoc_edges_cpu.py, test_assoc_edges_gpu.py).

`cslam_ekf_associate` returns integers (idf, kind), and the device is not bit-identical to the C oracle (FMA contraction,
its own sqrt / atan2 / log).  Equality of integers can only be demanded where the REFERENCE is decisive, so this module
  * restates EKF.cpp:131-144 in plain numpy f64, O(1) per (observation, feature) pair (`pair_reference`);
  * restates the sequential gate loop EKF.cpp:235-326 on those values (`decide`), with optional deliberate faults for the
    negative controls of test_assoc_edges_cpu.py;
  * measures tau per case = 64 x the largest |working-precision C oracle - f64 reference| over nis and nd of the pairs
    with nis < 4 gate2 (`Case.tau`; 64 covers FMA contraction and another libm, and stays far below the gaps between
    competing candidates), never anything the device computes;
  * builds families of cases (A dense cluster, B exact ties, C gate against rank, D `outer`, E structure of S,
    F a degenerate feature) in which EVERY observation is decisive: every comparison that fixes its (idf, kind) has an
    f64 margin of at least tau (`Case.margins`).  No observation is left out.
The seeds below were found by the deterministic searches at the end of this file (`search_seed_a` and friends).
"""
import numpy as np

from pyoracle import Oracle

GATES = ((4.0, 25.0), (9.0, 16.0))
POSE = (1.0, -2.0, 0.3)
R_OBS = np.array([[0.08, 0.004], [0.004, 0.0024]])          # correlated, symmetric
R_NONSYM = np.array([[0.08, 0.012], [-0.006, 0.0024]])      # R[1] (= r10) and R[2] (= r01) differ in size and sign
R_PIVOT = np.array([[0.0024, 0.006], [0.006, 0.08]])         # SPD with |r10| > r00: S10 can exceed S00 when P is small
CHUNK = 64                                                  # features per pass of ekf_assoc_scan_kernel


def pi2pi(a):
    a = np.fmod(a, 2.0 * np.pi)
    a = np.where(a > np.pi, a - 2.0 * np.pi, a)
    return np.where(a < -np.pi, a + 2.0 * np.pi, a)


def pair_reference(X, P, Z, R, r_from=None, no_swap_sign=False, drop_pose_cross=False, no_wrap=False):
    """nis[m, nf], nd[m, nf] (f64) of EKF.cpp:131-144 on the given (dtype-rounded) inputs, and per feature S[nf, 2, 2]
    and whether the 2 x 2 pivoted LU swaps rows.  It reads the 5 x 5 block of P that H touches and all four entries of R
    (not assumed symmetric).  The keyword faults are the negative controls of test_assoc_edges_cpu.py."""
    X, P, R = (np.asarray(a, dtype=np.float64) for a in (X, P, R))
    Z = np.asarray(Z, dtype=np.float64).reshape(2, -1, order="F")
    nf = (X.shape[0] - 3) // 2
    fx = 3 + 2 * np.arange(nf)
    dx, dy = X[fx] - X[0], X[fx + 1] - X[1]
    d2 = dx * dx + dy * dy
    d = np.sqrt(d2)
    zero, one = np.zeros(nf), np.ones(nf)
    H = np.stack([np.stack([-dx / d, -dy / d, zero, dx / d, dy / d], axis=1),
                  np.stack([dy / d2, -dx / d2, -one, -dy / d2, dx / d2], axis=1)], axis=1)      # nf x 2 x 5
    idx = np.stack([0 * fx, 0 * fx + 1, 0 * fx + 2, fx, fx + 1], axis=1)
    P5 = P[idx[:, :, None], idx[:, None, :]]
    if drop_pose_cross:
        P5 = P5.copy()
        P5[:, :3, 3:] = 0.0
        P5[:, 3:, :3] = 0.0
    if r_from == "r10":      # both off-diagonal entries read from R[1]
        R = np.array([[R[0, 0], R[1, 0]], [R[1, 0], R[1, 1]]])
    elif r_from == "r01":    # ... from R[2]
        R = np.array([[R[0, 0], R[0, 1]], [R[0, 1], R[1, 1]]])
    S = np.einsum("fri,fij,fcj->frc", H, P5, H) + R[None]
    a, b, c, dd = S[:, 0, 0], S[:, 0, 1], S[:, 1, 0], S[:, 1, 1]
    sw = np.abs(c) > np.abs(a)
    u00, u01 = np.where(sw, c, a), np.where(sw, dd, b)
    l10 = np.where(sw, a, c) / u00
    u11 = np.where(sw, b, dd) - l10 * u01
    det = np.where(sw & (not no_swap_sign), -(u00 * u11), u00 * u11)
    inv = np.zeros((nf, 2, 2))
    for col in range(2):
        x0 = np.where(sw, 1, 0) == col
        x1 = np.where(sw, 0, 1) == col
        x1 = (x1 - l10 * x0) / u11
        x0 = (x0 - u01 * x1) / u00
        inv[:, 0, col], inv[:, 1, col] = x0, x1
    v0 = Z[0][:, None] - d[None, :]
    v1 = Z[1][:, None] - (np.arctan2(dy, dx) - X[2])[None, :]
    if not no_wrap:
        v1 = pi2pi(v1)
    t0 = v0 * inv[None, :, 0, 0] + v1 * inv[None, :, 1, 0]
    t1 = v0 * inv[None, :, 0, 1] + v1 * inv[None, :, 1, 1]
    nis = t0 * v0 + t1 * v1
    with np.errstate(invalid="ignore", divide="ignore"):
        nd = nis + np.log(det)[None, :]
    return nis, nd, S, sw


def decide(nis, nd, gate1, gate2, fault=None):
    """The sequential rule of EKF.cpp:235-326 on given nis / nd -> (idf[m] 1-based or 0, kind[m], records): records[i] is
    the list of 0-based features that set a new best for observation i, in order.  fault: None or one of 'inclusive'
    (`<=` in the record test), 'last_tie' (the last index among equal minima), 'gate_on_nd', 'outer_ungated_only',
    'outer_first_chunk'."""
    m, nf = nis.shape
    idf, kind, records = np.zeros(m, np.int32), np.zeros(m, np.int32), []
    for i in range(m):
        jbest, nbest, outer, rec = 0, np.inf, np.inf, []
        for j in range(nf):
            gated = (nd[i, j] if fault == "gate_on_nd" else nis[i, j]) < gate1
            better = nd[i, j] <= nbest if fault == "inclusive" else nd[i, j] < nbest
            if gated and better:
                nbest, jbest = nd[i, j], j + 1
                rec.append(j)
            else:
                if fault == "outer_ungated_only" and gated:
                    continue
                if fault == "outer_first_chunk" and j >= CHUNK:
                    continue
                if nis[i, j] < outer:
                    outer = nis[i, j]
        if fault == "last_tie" and jbest:
            jbest = int(np.nonzero((nis[i] < gate1) & (nd[i] == nbest))[0][-1]) + 1
        idf[i] = jbest
        kind[i] = 1 if jbest else (2 if outer > gate2 else 0)
        records.append(rec)
    return idf, kind, records


class Case:
    """One associate() call: state (X, P), observations Z, R, the gate pairs it is run with, and the groups of twin
    features (identical by construction, so they tie exactly).  Reference values are computed once and cached."""

    def __init__(self, name, family, dtype, X, P, Z, R, gates=GATES, twins=()):
        self.name, self.family, self.dtype = name, family, np.dtype(dtype)
        self.X = np.array(X, dtype=dtype)
        self.P = np.array(P, dtype=dtype, order="F")
        self.Z = np.array(np.asarray(Z).reshape(2, -1, order="F"), dtype=dtype, order="F")
        self.R = np.array(R, dtype=dtype, order="F")
        assert np.array_equal(self.P, self.P.T), name
        self.gates, self.twins = tuple(gates), tuple(tuple(g) for g in twins)
        self.n = self.X.shape[0]
        self.nf, self.m = (self.n - 3) // 2, self.Z.shape[1]
        self._ref = self._tau = None
        self._dec, self._oracle = {}, {}

    def __repr__(self):
        return f"Case({self.name}, nf={self.nf}, m={self.m}, {self.dtype.name})"

    def ref(self):
        if self._ref is None:
            self._ref = pair_reference(self.X, self.P, self.Z, self.R)
        return self._ref

    def decisions(self, gates):
        """(idf, kind, records) of the f64 reference under one gate pair."""
        if gates not in self._dec:
            nis, nd = self.ref()[:2]
            self._dec[gates] = decide(nis, nd, *gates)
        return self._dec[gates]

    def twin_of(self, j):
        for g in self.twins:
            if j in g:
                return set(g)
        return {j}

    def near_pairs(self):
        nis = self.ref()[0]
        return np.argwhere(nis < 4.0 * max(g[1] for g in self.gates))

    def tau(self):
        """64 x the largest |C oracle in the case's dtype - f64 reference| over nis and nd of the pairs with
        nis < 4 gate2 (far pairs have huge nis and take no part in any decision).  Floor: 64 x one rounding of the
        largest of those values in the dtype, so that tau cannot shrink to nothing where the oracle happens to agree to
        the last bit.  -> (tau, largest oracle error)"""
        if self._tau is None:
            nis, nd = self.ref()[:2]
            o = Oracle(self.dtype)
            err, big = 0.0, 1.0
            for i, j in self.near_pairs():
                a, b = o.compute_association(self.X, self.P, self.n, self.Z[:, i].copy(), self.R, int(j) + 1)
                err, big = max(err, abs(float(a) - nis[i, j])), max(big, abs(nis[i, j]))
                assert np.isnan(float(b)) == np.isnan(nd[i, j]), (self, i, j)
                if not np.isnan(nd[i, j]):
                    err, big = max(err, abs(float(b) - nd[i, j])), max(big, abs(nd[i, j]))
            self._tau = (64.0 * max(err, float(np.finfo(self.dtype).eps) * big), err)
        return self._tau

    def margins(self, gates):
        """Per observation, the smallest f64 margin of the comparisons that fix its (idf, kind): every nis against gate1;
        the winner's nd against every other gated nd (twins of the winner excepted: they tie by design, and the lower
        index wins); when nothing wins, the minimum nis against gate2."""
        nis, nd = self.ref()[:2]
        idf = self.decisions(gates)[0]
        g1, g2 = gates
        out = np.zeros(self.m)
        for i in range(self.m):
            mg = np.abs(nis[i] - g1).min() if self.nf else np.inf
            if idf[i]:
                w = idf[i] - 1
                rivals = (nis[i] < g1) & ~np.isnan(nd[i])
                rivals[list(self.twin_of(w))] = False
                if rivals.any():
                    mg = min(mg, (nd[i, rivals] - nd[i, w]).min())
                assert min(self.twin_of(w)) == w and all(nd[i, t] == nd[i, w] for t in self.twin_of(w)), (self, i)
            elif self.nf:
                mg = min(mg, abs(nis[i].min() - g2))
            out[i] = mg
        return out

    def oracle_decisions(self, dtype, gates):
        """Oracle(dtype).data_associate on the case's inputs converted to dtype."""
        key = (np.dtype(dtype), gates)
        if key not in self._oracle:
            o = Oracle(dtype)
            self._oracle[key] = o.data_associate(self.X.astype(dtype), np.asfortranarray(self.P.astype(dtype)), self.n,
                                                 np.asfortranarray(self.Z.astype(dtype)), self.R.astype(dtype), *gates)
        return self._oracle[key]


# ------------------------------------------------------------------------------------------------
# states
# ------------------------------------------------------------------------------------------------
def _covariance(nf, rng, pose_scale, scale, twins, var=(0.3, 3.0), corr=0.5):
    """P = (D + U U^T) scaled: landmark variances var plus a rank-4 part with pose-landmark cross-covariances of the
    strength of helpers.make_scenario(corr=0.5).  scale: {feature: factor on its two rows / columns}.  Twins share D and
    the rows of U (and their scale), so their blocks, cross-covariances and everything computed from them are equal; P
    stays SPD (D > 0)."""
    n = 3 + 2 * nf
    D = np.ones(n)
    D[3:] = np.repeat(rng.uniform(var[0], var[1], size=nf), 2)
    U = rng.normal(size=(n, 4)) * corr
    s = np.ones(n)
    s[:3] = np.sqrt(pose_scale)
    for j, f in scale.items():
        s[3 + 2 * j: 5 + 2 * j] = f
    for g in twins:
        for t in g[1:]:
            for r in range(2):
                D[3 + 2 * t + r], U[3 + 2 * t + r], s[3 + 2 * t + r] = D[3 + 2 * g[0] + r], U[3 + 2 * g[0] + r], s[3 + 2 * g[0] + r]
    P = (np.diag(D) + U @ U.T) * s[:, None] * s[None, :]
    return 0.5 * (P + P.T)


def cluster_state(nf, seed, radius=1.5, pose_scale=1e-2, scale=None, twins=(), var=(0.3, 3.0)):
    """nf landmarks within `radius` of one centre 70 m from the pose: every observation near the centre has many
    features inside gate1."""
    rng = np.random.default_rng(seed)
    ang = POSE[2] + 0.4
    centre = np.array([POSE[0] + 70.0 * np.cos(ang), POSE[1] + 70.0 * np.sin(ang)])
    LM = centre[None, :] + rng.uniform(-radius, radius, size=(nf, 2))
    for g in twins:
        for t in g[1:]:
            LM[t] = LM[g[0]]
    P = _covariance(nf, rng, pose_scale, scale or {}, twins, var=var)
    return np.concatenate([POSE, LM.reshape(-1)]), P


def sparse_state(nf, seed, pose_scale=1e-4, scale=None, moved=None):
    """nf landmarks on a fan around the pose: 13 bearings 0.48 rad apart (-2.88 .. 2.88 relative to the heading, so some
    lie behind the vehicle) x ranges 60, 80, ... m; neighbours are tens of sigmas apart, so an observation has only the
    features inside a gate that the case puts there.  moved: {feature: (other feature, metres further out)}."""
    rng = np.random.default_rng(seed)
    k = np.arange(nf)
    rg, be = 60.0 + 20.0 * (k // 13), -2.88 + 0.48 * (k % 13)
    LM = np.stack([POSE[0] + rg * np.cos(be + POSE[2]), POSE[1] + rg * np.sin(be + POSE[2])], axis=1)
    for j, (other, dr) in (moved or {}).items():
        LM[j] = [POSE[0] + (rg[other] + dr) * np.cos(be[other] + POSE[2]), POSE[1] + (rg[other] + dr) * np.sin(be[other] + POSE[2])]
    P = _covariance(nf, rng, pose_scale, scale or {}, ())
    return np.concatenate([POSE, LM.reshape(-1)]), P


def predicted(X, j, dtype):
    """f64 range / bearing of 0-based feature j from the dtype-rounded state (bearing as observe_model gives it: not
    wrapped)."""
    X = np.asarray(np.asarray(X, dtype=dtype), dtype=np.float64)
    dx, dy = X[3 + 2 * j] - X[0], X[4 + 2 * j] - X[1]
    return np.array([np.hypot(dx, dy), np.arctan2(dy, dx) - X[2]])


# ------------------------------------------------------------------------------------------------
# family A: dense cluster
# ------------------------------------------------------------------------------------------------
A_NF = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257]
A_F64 = [65, 129, 257]
A_M = 12
A_SHRINK = 0.3
# seeds found by search_seed_a (first seed from 0 whose case is decisive with the coverage asserted in check_a)
A_SEEDS = {1: 0, 2: 4, 63: 0, 64: 3, 65: 3, 127: 55, 128: 1, 129: 79, 255: 110, 256: 34, 257: 46}


def a_targets(nf):
    return sorted({j for j in (0, 62, 63, 64, 65, nf - 1, 255, 256) if 0 <= j < nf})


def build_a(nf, dtype, seed):
    """12 observations in a cluster of nf landmarks: one at the predicted measurement (+ a little noise) of each
    intended winner (features at the ends of the 64-lane chunks, whose P rows / columns are shrunk by 0.3 so that their
    nd is the lowest), the rest at noisy measurements of other landmarks, where the winner is whoever the rule says."""
    tg = a_targets(nf)
    X, P = cluster_state(nf, 1000 * nf + seed, radius=1.5 if nf > 2 else 0.4, scale={j: A_SHRINK for j in tg})
    rng = np.random.default_rng(77_000 + 1000 * nf + seed)
    cols = []
    for i in range(A_M):
        j = tg[i] if i < len(tg) else int(rng.integers(nf))
        zp = predicted(X, j, dtype)
        noise = (0.05, 0.002) if i < len(tg) else (0.5, 0.02)
        cols.append(zp + rng.normal(size=2) * noise)
    return Case(f"A-nf{nf}", "A", dtype, X, P, np.stack(cols, axis=1), R_OBS)


def check_a(case):
    """The coverage family A promises, from the f64 reference.  -> dict of what was found."""
    nis = case.ref()[0]
    tg = a_targets(case.nf)
    found = {"gated": [], "winners": set(), "late": 0, "rank_differs": 0}
    for gates in case.gates:
        idf, kind, records = case.decisions(gates)
        ngated = (nis < gates[0]).sum(axis=1)
        assert np.all(ngated >= min(case.nf, 8)), (case, gates, ngated)
        assert np.all(kind == 1), (case, gates, kind)
        found["gated"] += [int(ngated.min()), int(ngated.max())]
        found["winners"] |= set(int(w) - 1 for w in idf)
        assert [int(w) - 1 for w in idf[: len(tg)]] == tg, (case, gates, idf)
        found["late"] += sum(1 for r in records if r[-1] // CHUNK > r[0] // CHUNK)
        masked = np.where(nis < gates[0], nis, np.inf)
        found["rank_differs"] += int((masked.argmin(axis=1) + 1 != idf).sum())
    if case.nf >= 65:
        assert found["late"] > 0, case
    if case.nf >= 63:
        assert any((w + 1) % 64 == 63 for w in found["winners"]), case   # rows 127 | 128 of P: two 128-row tiles
    return found


# ------------------------------------------------------------------------------------------------
# family B: exact ties
# ------------------------------------------------------------------------------------------------
B_NF = 257
B_TWINS = ((10, 40), (63, 64), (5, 200), (255, 256), (100, 101, 150))
B_SEED = 7


def build_b(dtype=np.float32, seed=B_SEED):
    """Twin landmarks (same position, same 2 x 2 block, same cross-covariances) tie bit for bit; the observation sits at
    their predicted measurement and the lower index must win.  The pairs lie in one chunk, on the two sides of a chunk
    boundary (63 | 64 and 255 | 256) and chunks apart; one triple."""
    scale = {g[0]: A_SHRINK for g in B_TWINS}
    X, P = cluster_state(B_NF, 5000 + seed, scale=scale, twins=B_TWINS)
    Z = np.stack([predicted(X, g[0], dtype) for g in B_TWINS], axis=1)
    return Case("B-ties", "B", dtype, X, P, Z, R_OBS, twins=B_TWINS)


def check_b(case):
    for gates in case.gates:
        idf, kind, _ = case.decisions(gates)
        assert [int(w) - 1 for w in idf] == [g[0] for g in B_TWINS] and np.all(kind == 1), (case, idf)
    for g in B_TWINS:
        for t in g[1:]:
            a, b = slice(3 + 2 * g[0], 5 + 2 * g[0]), slice(3 + 2 * t, 5 + 2 * t)
            assert np.array_equal(case.X[a], case.X[b]) and np.array_equal(case.P[a, a], case.P[b, b])
            assert np.array_equal(case.P[:3, a], case.P[:3, b])
    return {"groups": len(B_TWINS)}


# ------------------------------------------------------------------------------------------------
# family C: gate against rank
# ------------------------------------------------------------------------------------------------
C_NF = 130
C_GATES = ((4.0, 25.0),)
# (A, B): A is B's neighbour 1 m further out with a tiny P block.  Before / after B, in B's chunk and in another one.
C_PAIRS = ((20, 30), (45, 33), (8, 100), (110, 50))
C_LONE = (60, 120)          # A-like features with no B: dropped (gate1 < nis < gate2) and new (nis > gate2)
C_TINY = 0.02
C_SEED = 0


def _c_state(seed):
    scale = {a: C_TINY for a, _ in C_PAIRS}
    scale.update({a: C_TINY for a in C_LONE})
    return sparse_state(C_NF, 7000 + seed, scale=scale, moved={a: (b, 1.0) for a, b in C_PAIRS})


def build_c(dtype=np.float32, seed=C_SEED):
    """Feature A has the lowest nd of all (tiny S: a very negative log det) but lies outside gate1; B is inside with a
    higher nd: the answer is B.  The observation of each pair is the first point of a fixed grid of offsets from B's
    predicted measurement at which the f64 reference shows that pattern with the largest margin."""
    X, P = _c_state(seed)
    g1, g2 = C_GATES[0]
    cols = []
    grid = [(dr, db) for dr in np.linspace(-2.0, 2.0, 41) for db in np.linspace(-0.06, 0.06, 13)]
    for a, b in C_PAIRS:
        zb = predicted(X, b, dtype)
        Zg = np.stack([zb + np.array(o) for o in grid], axis=1).astype(dtype)
        nis, nd = pair_reference(np.asarray(X, dtype=dtype), np.asarray(P, dtype=dtype), Zg, R_OBS.astype(dtype))[:2]
        ok = (nis[:, a] > g1) & (nis[:, b] < g1) & (nd[:, a] < nd[:, b])
        mg = np.minimum(np.minimum(nis[:, a] - g1, g1 - nis[:, b]), np.minimum(nd[:, b] - nd[:, a], g2 - nis[:, a]))
        assert ok.any(), (a, b)
        cols.append(Zg[:, int(np.argmax(np.where(ok, mg, -np.inf)))].astype(np.float64))
    for a, dr in zip(C_LONE, (0.9, 1.8)):
        cols.append(predicted(X, a, dtype) + np.array([dr, 0.0]))
    return Case("C-gate-vs-rank", "C", dtype, X, P, np.stack(cols, axis=1), R_OBS, gates=C_GATES)


def check_c(case):
    nis, nd = case.ref()[:2]
    g1, g2 = case.gates[0]
    idf, kind, _ = case.decisions(case.gates[0])
    for i, (a, b) in enumerate(C_PAIRS):
        assert nis[i, a] > g1 and nis[i, b] < g1 and nd[i, a] == np.nanmin(nd[i]) and nd[i, a] < nd[i, b], (case, i)
        assert idf[i] == b + 1 and kind[i] == 1, (case, i, idf[i])
    k = len(C_PAIRS)
    assert g1 < nis[k, C_LONE[0]] < g2 and (idf[k], kind[k]) == (0, 0), (case, nis[k, C_LONE[0]])
    assert nis[k + 1].min() > g2 and (idf[k + 1], kind[k + 1]) == (0, 2), case
    return {"order": ["A<B same chunk", "A>B same chunk", "A<B other chunk", "A>B other chunk"]}


# ------------------------------------------------------------------------------------------------
# family D: outer
# ------------------------------------------------------------------------------------------------
D_NF = 130
D_TARGETS = (0, 63, 129, 64)   # lane 0 of the first of several chunks, lane 63, the last partial chunk, lane 0 of chunk 1
D_SEED = 0


def _nis_of(X, P, R, z, j, dtype):
    Zc = np.asarray(z, dtype=dtype).reshape(2, 1)
    return pair_reference(X, P, Zc, R)[0][0, j]


def build_d(gates, dtype=np.float32, seed=D_SEED):
    """Nothing is gated; the minimum nis of each observation belongs to one feature and lies 3 tau under or over gate2.
    The range at which that feature's nis crosses gate2 is found by bisection on the f64 reference; tau is measured on
    the oracle for the observations at the crossings; then each range is moved, over neighbouring values of the dtype,
    until the margin is within [2.5 tau, 3.5 tau]."""
    X, P = sparse_state(D_NF, 9000 + seed)
    Xd, Pd, Rd = np.asarray(X, dtype=dtype), np.asarray(P, dtype=dtype), R_OBS.astype(dtype)
    g2 = gates[1]
    t = np.dtype(dtype).type
    cross = []
    for j in D_TARGETS:
        zp = predicted(X, j, dtype)
        lo, hi = zp[0], zp[0] + 30.0              # nis increases with the range beyond the predicted one
        assert _nis_of(Xd, Pd, Rd, (lo, zp[1]), j, dtype) < g2 < _nis_of(Xd, Pd, Rd, (hi, zp[1]), j, dtype)
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if _nis_of(Xd, Pd, Rd, (mid, zp[1]), j, dtype) < g2 else (lo, mid)
        cross.append(np.array([lo, zp[1]]))
    tau = Case("probe", "D", dtype, X, P, np.stack(cross, axis=1), R_OBS, gates=(gates,)).tau()[0]
    cols = []
    for j, zc in zip(D_TARGETS, cross):
        f = lambda r: _nis_of(Xd, Pd, Rd, (r, zc[1]), j, dtype)   # noqa: E731
        slope = (f(zc[0] + 1e-3) - f(zc[0] - 1e-3)) / 2e-3
        for sign in (-1.0, 1.0):
            r = t(zc[0] + sign * 3.0 * tau / slope)
            for _ in range(4000):
                mg = sign * (f(r) - g2)
                if 2.5 * tau <= mg <= 3.5 * tau:
                    break
                r = np.nextafter(r, t(sign * np.inf) if mg < 2.5 * tau else t(-sign * np.inf))
            cols.append(np.array([float(r), float(t(zc[1]))]))
    return Case(f"D-outer-g{int(gates[0])}-{int(gates[1])}", "D", dtype, X, P, np.stack(cols, axis=1), R_OBS, gates=(gates,))


def check_d(case):
    nis = case.ref()[0]
    g1, g2 = case.gates[0]
    idf, kind, _ = case.decisions(case.gates[0])
    tau = case.tau()[0]
    assert not (nis < g1).any() and np.all(idf == 0), case
    for i in range(case.m):
        j = D_TARGETS[i // 2]
        assert nis[i].argmin() == j and np.sort(nis[i])[1] > 2.0 * g2, (case, i)
        mg = (g2 - nis[i, j]) if i % 2 == 0 else (nis[i, j] - g2)
        assert tau <= mg < 10.0 * tau, (case, i, mg, tau)
        assert kind[i] == (0 if i % 2 == 0 else 2), (case, i)
    return {"targets": D_TARGETS}


# ------------------------------------------------------------------------------------------------
# family E: structure of S
# ------------------------------------------------------------------------------------------------
E_NF = 65
E_M = 12
E_SEEDS = {"nonsym": 4, "pivot": 8}
E_WRAP_BEHIND, E_WRAP_AHEAD = 25, 33   # bearings 2.88 (behind: atan2 - phi < -pi) and 0.48 relative to the heading
E_PIVOT_SMALL = 0.05                   # landmarks with this scale have P_rr << r10 - r00: the LU swaps rows


def build_e_nonsym(dtype=np.float32, seed=None):
    """A small-P cluster (S is dominated by R) under a non-symmetric R.  nis and log det S depend on S01 + S10 and
    S01 * S10 only, so exchanging R[1] and R[2] cannot change a decision in exact arithmetic; what the case pins is that
    BOTH are read: taking either of them for both off-diagonal entries changes winners."""
    seed = E_SEEDS["nonsym"] if seed is None else seed
    X, P = cluster_state(E_NF, 11_000 + seed, radius=0.6, pose_scale=1e-5, var=(0.003, 0.03))
    rng = np.random.default_rng(11_500 + seed)
    cols = [predicted(X, int(rng.integers(E_NF)), dtype) + rng.normal(size=2) * (0.25, 0.004) for _ in range(E_M)]
    return Case("E-nonsym-R", "E", dtype, X, P, np.stack(cols, axis=1), R_NONSYM)


def build_e_pivot(dtype=np.float32, seed=None):
    """R with |r10| > r00 and a small P: for the landmarks scaled by E_PIVOT_SMALL |S10| > |S00| (the LU swaps rows and
    the determinant changes sign), for the others not.  Half of the observations aim at each kind."""
    seed = E_SEEDS["pivot"] if seed is None else seed
    small = {j: E_PIVOT_SMALL for j in range(0, E_NF, 2)}
    X, P = cluster_state(E_NF, 12_000 + seed, radius=15.0, pose_scale=1e-5, scale=small, var=(0.05, 0.2))
    rng = np.random.default_rng(12_500 + seed)
    cols = []
    for i in range(E_M):
        j = int(rng.integers(E_NF // 2)) * 2 + (i % 2)
        cols.append(predicted(X, j, dtype) + rng.normal(size=2) * (0.02, 0.05))
    return Case("E-pivot", "E", dtype, X, P, np.stack(cols, axis=1), R_PIVOT)


def build_e_wrap(dtype=np.float32):
    """Raw bearing innovations beyond +-pi: a landmark behind the vehicle (predicted bearing -3.40, observed +2.88), and
    an observation given with +2 pi.  Both must be associated."""
    X, P = sparse_state(D_NF, 13_000)
    zb, za = predicted(X, E_WRAP_BEHIND, dtype), predicted(X, E_WRAP_AHEAD, dtype)
    assert zb[1] < -np.pi
    Z = np.stack([zb + [0.1, 2.0 * np.pi + 0.004], za + [-0.1, 2.0 * np.pi - 0.003]], axis=1)
    return Case("E-wrap", "E", dtype, X, P, Z, R_OBS)


def check_e(case):
    nis, nd, S, sw = case.ref()
    out = {}
    if case.name == "E-pivot":
        win = set()
        for gates in case.gates:
            idf, kind, _ = case.decisions(gates)
            assert np.all(kind == 1), (case, kind)
            win |= set(int(w) - 1 for w in idf)
        swapped = [w for w in win if abs(S[w, 1, 0]) > abs(S[w, 0, 0])]
        assert swapped and len(swapped) < len(win), (case, sorted(win), swapped)
        assert all(bool(sw[w]) for w in swapped)
        out = {"winners_swapped": len(swapped), "winners_not": len(win) - len(swapped)}
    if case.name == "E-wrap":
        raw = case.Z.astype(np.float64)[1] - np.array([predicted(case.X, j, case.dtype)[1] for j in (E_WRAP_BEHIND, E_WRAP_AHEAD)])
        assert np.all(np.abs(raw) > np.pi), raw
        for gates in case.gates:
            idf, kind, _ = case.decisions(gates)
            assert list(idf) == [E_WRAP_BEHIND + 1, E_WRAP_AHEAD + 1] and np.all(kind == 1), (case, idf)
        out = {"raw_bearing_innovations": [float(r) for r in raw]}
    if case.name == "E-nonsym-R":
        assert case.R[0, 1] != case.R[1, 0]
        for r_from in ("r10", "r01"):
            n2, d2 = pair_reference(case.X, case.P, case.Z, case.R, r_from=r_from)[:2]
            assert any(not np.array_equal(decide(n2, d2, *g)[0], case.decisions(g)[0]) for g in case.gates), (case, r_from)
        out = {"kinds": sorted(set(int(k) for g in case.gates for k in case.decisions(g)[1]))}
    return out


# ------------------------------------------------------------------------------------------------
# family F: a degenerate feature
# ------------------------------------------------------------------------------------------------
F_BAD, F_WIN = 3, 20
F_LONE = 40
F_SEEDS = {"ahead": 0}


def build_f_ahead(dtype=np.float32, seed=None):
    """Feature 3 has an indefinite P block (det S < 0: nd is NaN) and sits ahead of the true winner 20 in the cluster;
    it is inside gate1 for some observations and must never set a record."""
    seed = F_SEEDS["ahead"] if seed is None else seed
    X, P = cluster_state(E_NF, 14_000 + seed, scale={F_WIN: A_SHRINK})
    a = slice(3 + 2 * F_BAD, 5 + 2 * F_BAD)
    P[a, a] = np.diag([-5.0, -5.0])
    rng = np.random.default_rng(14_500 + seed)
    cols = [predicted(X, F_WIN, dtype) + rng.normal(size=2) * (0.05, 0.002) for _ in range(3)]
    cols += [predicted(X, F_BAD, dtype) + rng.normal(size=2) * (0.3, 0.01) for _ in range(3)]
    return Case("F-nan-ahead", "F", dtype, X, P, np.stack(cols, axis=1), R_OBS)


def build_f_lone(dtype=np.float32):
    """An observation near only the degenerate feature: it is inside gate1 but sets no record, and its nis feeds
    `outer`, so the observation is dropped (kind 0), not declared new."""
    X, P = sparse_state(D_NF, 15_000)
    a = slice(3 + 2 * F_LONE, 5 + 2 * F_LONE)
    P[a, a] = np.diag([-5.0, -5.0])
    Z = np.stack([predicted(X, F_LONE, dtype) + [0.5, 0.001], predicted(X, F_LONE, dtype) + [-1.0, -0.002]], axis=1)
    return Case("F-nan-lone", "F", dtype, X, P, Z, R_OBS)


def check_f(case):
    nis, nd = case.ref()[:2]
    bad = F_BAD if case.name == "F-nan-ahead" else F_LONE
    assert np.all(np.isnan(nd[:, bad])) and not np.isnan(np.delete(nd, bad, axis=1)).any(), case
    out = {"gated_nan": 0}
    for gates in case.gates:
        idf, kind, _ = case.decisions(gates)
        out["gated_nan"] += int((nis[:, bad] < gates[0]).sum())
        assert not np.any(idf == bad + 1), case
        if case.name == "F-nan-ahead":
            assert np.all(idf[:3] == F_WIN + 1) and np.all(kind == 1), (case, idf, kind)
        else:
            assert np.all(nis[:, bad] < gates[0]) and np.all(idf == 0) and np.all(kind == 0), (case, nis[:, bad], kind)
    assert out["gated_nan"] > 0, case
    return out


# ------------------------------------------------------------------------------------------------
# family G: handle state (the device cases are in test_assoc_edges_gpu.py); here the one input it needs built
# ------------------------------------------------------------------------------------------------
G_WIDE_NF, G_WIDE_M = 8, 257


def build_g_wide(dtype=np.float32):
    """257 observations against 8 features (one workgroup per observation: a grid wider than the map).  Candidates are
    drawn in a fixed order and kept when every margin of the f64 reference is >= TAU_SEARCH."""
    X, P = cluster_state(G_WIDE_NF, 16_000)
    rng = np.random.default_rng(16_500)
    bound = TAU_SEARCH[np.dtype(dtype)]
    cols = []
    while len(cols) < G_WIDE_M:
        cand = np.stack([predicted(X, int(rng.integers(G_WIDE_NF)), dtype) + rng.normal(size=2) * (0.8, 0.02)
                         for _ in range(64)], axis=1)
        probe = Case("probe", "G", dtype, X, P, cand, R_OBS)
        keep = np.minimum(probe.margins(GATES[0]), probe.margins(GATES[1])) >= bound
        cols += [probe.Z[:, i].astype(np.float64) for i in np.nonzero(keep)[0]]
    return Case("G-m257-nf8", "G", dtype, X, P, np.stack(cols[:G_WIDE_M], axis=1), R_OBS)


def check_g(case):
    kinds = sorted(set(int(k) for g in case.gates for k in case.decisions(g)[1]))
    return {"kinds": kinds, "winners": sorted(set(int(w) for g in case.gates for w in case.decisions(g)[0]))}


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
CASE_KEYS = ([("A", nf, "float32") for nf in A_NF] + [("A", nf, "float64") for nf in A_F64] +
             [("B", 0, "float32"), ("C", 0, "float32"), ("D", 0, "float32"), ("D", 1, "float32"),
              ("E", "nonsym", "float32"), ("E", "pivot", "float32"), ("E", "wrap", "float32"),
              ("F", "ahead", "float32"), ("F", "lone", "float32"), ("G", "wide", "float32")])
CHECKS = {"A": check_a, "B": check_b, "C": check_c, "D": check_d, "E": check_e, "F": check_f, "G": check_g}
_CACHE = {}


def case_id(key):
    return f"{key[0]}-{key[1]}-{key[2]}"


def get_case(key):
    """The case of one key, built once per process (the oracle calls are the cost)."""
    if key not in _CACHE:
        fam, sub, dt = key
        dtype = np.dtype(dt).type
        if fam == "A":
            c = build_a(sub, dtype, A_SEEDS[sub])
        elif fam == "B":
            c = build_b(dtype)
        elif fam == "C":
            c = build_c(dtype)
        elif fam == "D":
            c = build_d(GATES[sub], dtype)
        elif fam == "E":
            c = {"nonsym": build_e_nonsym, "pivot": build_e_pivot, "wrap": build_e_wrap}[sub](dtype)
        elif fam == "F":
            c = {"ahead": build_f_ahead, "lone": build_f_lone}[sub](dtype)
        else:
            c = build_g_wide(dtype)
        _CACHE[key] = c
    return _CACHE[key]


def family_keys(fam):
    return [k for k in CASE_KEYS if k[0] == fam]


# ------------------------------------------------------------------------------------------------
# the searches that chose the committed seeds (no device)
# ------------------------------------------------------------------------------------------------
TAU_SEARCH = {np.dtype(np.float32): 1e-2, np.dtype(np.float64): 1e-9}   # demanded of a seed; the tests use measured tau


def _decisive_at(case, bound):
    return all(case.margins(g).min() >= bound for g in case.gates)


def search_seed(build, check, dtypes, limit=1000):
    """First seed from 0 whose case passes its coverage check and has every margin >= TAU_SEARCH (numpy reference only:
    cheap) and then >= 1.5 x the tau measured on the oracle, in every dtype."""
    for seed in range(limit):
        try:
            for dt in dtypes:
                c = build(dt, seed)
                check(c)
                assert _decisive_at(c, TAU_SEARCH[np.dtype(dt)])
                assert _decisive_at(c, 1.5 * c.tau()[0])
        except AssertionError:
            continue
        return seed
    raise RuntimeError("no seed found")


def search_seed_a(nf):
    dts = [np.float32, np.float64] if nf in A_F64 else [np.float32]
    return search_seed(lambda dt, s: build_a(nf, dt, s), check_a, dts)
