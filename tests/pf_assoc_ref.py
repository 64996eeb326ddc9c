"""Reference and case builders of the particle filter's data association (test_pf_assoc_cpu.py, test_pf_assoc_gpu.py).

`cslam_pf_associate` returns integers (idf, kind) per (particle, observation), and the device is not bit-identical to any
CPU evaluation.  Equality of integers can only be demanded where the REFERENCE is decisive, so this module
  * restates EKF.cpp:131-144 for a particle -- P = blockdiag(Pv, PF_f), S = HV Pv HV^T + HF PF_f HF^T + R -- in plain
    numpy, vectorised over particles, features and observations, in any dtype (`pair_reference_pf`; f64 is THE reference,
    the working dtype only serves to measure tau);
  * restates the rule of EKF.cpp:235-326 on those values: `decide` is assoc_builders.decide (sequential, with its
    deliberate faults), `decide_cloud` the same rule for a whole cloud at once (test_pf_assoc_cpu.py proves them equal);
  * restates the per-particle duplicate resolution (`resolve_duplicates`);
  * measures tau per case = 64 x the largest |numpy evaluation in the case's dtype - f64 evaluation| over nis and nd of the
    pairs with nis < 4 gate2 (`Case.tau`; the factor and the reasoning of assoc_builders.Case.tau), never anything the
    device computes;
  * builds the cases.  An observation enters a case only if EVERY particle decides it with margins of at least
    TAU_SEARCH: candidates are drawn in a fixed order from a seeded generator and the first ones that qualify are kept
    (`_search`), so the search is deterministic and is repeated whenever a case is built.  test_pf_assoc_cpu.py then
    proves, independently of the search, that every margin (`Case.margins`) is at least the measured tau;
  * restates the consumers per particle on the CPU oracle (`consumer_reference`).

Clouds come from pf_builders.tight_particles (poses, Pv, PF, the 0.3 m jitter of every particle's copy of the map); the
common map is re-centred on small clusters 15 - 45 m around the vehicle, so that several features compete for one
observation and f32 keeps a small tau.
"""
import numpy as np

from assoc_builders import decide, pi2pi  # noqa: F401  (decide is re-exported: the sequential rule with its faults)
from pf_builders import Q_CTRL, PREDICT, TRUE_POSE, tight_particles
from pyoracle import REF_EXACT, Oracle

FEAT_CHUNK, OBS_CHUNK = 32, 8      # kPfAssocFeatChunk / kPfAssocObsChunk of pf_assoc_kernels.hpp
GATES = ((4.0, 25.0), (9.0, 16.0))
R_OBS = np.array([[0.08, 0.004], [0.004, 0.0024]])   # correlated; all four entries are read
TAU_SEARCH = {np.dtype(np.float32): 2e-2, np.dtype(np.float64): 1e-9}   # demanded by the search; the tests use measured tau
CLUSTER = 3                        # features per cluster of the re-centred map


# ------------------------------------------------------------------------------------------------
# the pair quantities
# ------------------------------------------------------------------------------------------------
def cloud_arrays(parts, dtype):
    """[w, Xv, Pv, XF, PF] per particle -> w[np], Xv[np,3], Pv[np,3,3], XF[np,2,nf], PF[np,4,nf] in dtype."""
    w = np.array([p[0] for p in parts], dtype=dtype)
    Xv = np.array([p[1] for p in parts], dtype=dtype)
    Pv = np.array([np.asarray(p[2]).reshape(3, 3, order="F") for p in parts], dtype=dtype)
    nf = np.asarray(parts[0][3]).size // 2
    XF = np.array([np.asarray(p[3]).reshape(2, nf, order="F") for p in parts], dtype=dtype).reshape(len(parts), 2, nf)
    PF = np.array([np.asarray(p[4]).reshape(4, nf, order="F") for p in parts], dtype=dtype).reshape(len(parts), 4, nf)
    return w, Xv, Pv, XF, PF


def pair_reference_pf(Xv, Pv, XF, PF, Z, R, dtype=np.float64, drop_pose=False, no_wrap=False):
    """nis[np, m, nf], nd[np, m, nf] of EKF.cpp:131-144 on every particle's own state, all arithmetic in `dtype`.
    PF[:, e, f] is the column-major 2 x 2 block (e = r + 2 c); R is read entry by entry (not assumed symmetric).
    The keyword faults are negative controls."""
    dt = np.dtype(dtype).type
    Xv, Pv, XF, PF, R = (np.asarray(a, dtype=dtype) for a in (Xv, Pv, XF, PF, R))
    Z = np.asarray(Z, dtype=dtype).reshape(2, -1, order="F")
    npart, nf = XF.shape[0], XF.shape[2]
    dx, dy = XF[:, 0, :] - Xv[:, 0, None], XF[:, 1, :] - Xv[:, 1, None]
    d2 = dx * dx + dy * dy
    d = np.sqrt(d2)
    zb = pi2pi(np.arctan2(dy, dx) - Xv[:, 2, None]).astype(dtype)
    zero, one = np.zeros_like(d), np.ones_like(d)
    HV = np.stack([np.stack([-dx / d, -dy / d, zero], axis=-1), np.stack([dy / d2, -dx / d2, -one], axis=-1)], axis=-2)
    HF = np.stack([np.stack([dx / d, dy / d], axis=-1), np.stack([-dy / d2, dx / d2], axis=-1)], axis=-2)   # np, nf, 2, 2
    PFm = np.stack([np.stack([PF[:, 0, :], PF[:, 2, :]], axis=-1), np.stack([PF[:, 1, :], PF[:, 3, :]], axis=-1)], axis=-2)
    S = np.einsum("pfri,pfij,pfcj->pfrc", HF, PFm, HF) + R[None, None]
    if not drop_pose:
        S = np.einsum("pfri,pij,pfcj->pfrc", HV, Pv, HV) + S
    S = S.astype(dtype)
    a, b, c, dd = S[..., 0, 0], S[..., 0, 1], S[..., 1, 0], S[..., 1, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        sw = np.abs(c) > np.abs(a)
        u00, u01 = np.where(sw, c, a), np.where(sw, dd, b)
        l10 = np.where(sw, a, c) / u00
        u11 = np.where(sw, b, dd) - l10 * u01
        det = np.where(sw, -(u00 * u11), u00 * u11)
        inv = np.zeros(S.shape, dtype=dtype)
        for col in range(2):
            x0 = (np.where(sw, 1, 0) == col).astype(dtype)
            x1 = (np.where(sw, 0, 1) == col).astype(dtype)
            x1 = (x1 - l10 * x0) / u11
            x0 = (x0 - u01 * x1) / u00
            inv[..., 0, col], inv[..., 1, col] = x0, x1
        v0 = Z[0][None, :, None] - d[:, None, :]
        v1 = Z[1][None, :, None] - zb[:, None, :]
        if not no_wrap:
            v1 = pi2pi(v1).astype(dtype)
        t0 = v0 * inv[:, None, :, 0, 0] + v1 * inv[:, None, :, 1, 0]
        t1 = v0 * inv[:, None, :, 0, 1] + v1 * inv[:, None, :, 1, 1]
        nis = t0 * v0 + t1 * v1
        nd = nis + np.log(det)[:, None, :]
    assert nis.dtype == np.dtype(dtype) and nd.dtype == np.dtype(dtype), (nis.dtype, nd.dtype, dt)
    return nis, nd


# ------------------------------------------------------------------------------------------------
# the rule, for a whole cloud, and the duplicate resolution
# ------------------------------------------------------------------------------------------------
def decide_cloud(nis, nd, gate1, gate2, gate_on_nd=False):
    """EKF.cpp:235-326 with strict comparisons on nis / nd [np, m, nf] -> idf[m, np] (1-based, 0 = none), kind[m, np],
    nbest[m, np] (the winner's nd, inf where there is none).  A NaN takes part in no record; nf = 0 gives kind 2."""
    npart, m, nf = nis.shape
    if nf == 0:
        return np.zeros((m, npart), np.int32), np.full((m, npart), 2, np.int32), np.full((m, npart), np.inf)
    with np.errstate(invalid="ignore"):
        gated = (nd if gate_on_nd else nis) < gate1
        cand = np.where(gated & (nd < np.inf), nd, np.inf)
        nbest = cand.min(axis=2)
        has = nbest < np.inf
        jbest = np.where(has, cand.argmin(axis=2) + 1, 0)          # argmin: the first of equal minima
        outer = np.where(np.isnan(nis), np.inf, nis).min(axis=2)
    kind = np.where(has, 1, np.where(outer > gate2, 2, 0))
    return jbest.T.astype(np.int32), kind.T.astype(np.int32), nbest.T


def resolve_duplicates(idf, kind, nbest):
    """Per particle: among the observations that claim one feature the smallest nd keeps it, the lower observation index
    on equal nd; the others become idf 0 / kind 0.  idf, kind, nbest: [m, np] -> (idf, kind) resolved."""
    m = idf.shape[0]
    lost = np.zeros(idf.shape, bool)
    for j in range(m):
        for k in range(m):
            if k != j:
                same = (idf[j] != 0) & (idf[k] == idf[j])
                lost[j] |= same & ((nbest[k] < nbest[j]) | ((nbest[k] == nbest[j]) & (k < j)))
    return np.where(lost, 0, idf).astype(np.int32), np.where(lost, 0, kind).astype(np.int32)


# ------------------------------------------------------------------------------------------------
# a case
# ------------------------------------------------------------------------------------------------
class Case:
    """One associate() call on a cloud: particles, observations, R, the gate pairs it is run with, the groups of twin
    features (identical in every particle: they tie exactly) and the groups of identical observation columns."""

    def __init__(self, name, dtype, parts, Z, R=R_OBS, gates=GATES, twins=(), same_obs=()):
        self.name, self.dtype = name, np.dtype(dtype)
        self.parts = parts
        self.w, self.Xv, self.Pv, self.XF, self.PF = cloud_arrays(parts, dtype)
        self.Z = np.array(np.asarray(Z, dtype=np.float64).reshape(2, -1, order="F"), dtype=dtype, order="F")
        self.R = np.array(R, dtype=dtype, order="F")
        self.gates, self.twins, self.same_obs = tuple(gates), tuple(map(tuple, twins)), tuple(map(tuple, same_obs))
        self.np_, self.nf, self.m = len(parts), self.XF.shape[2], self.Z.shape[1]
        self._ref = self._tau = None
        self._dec = {}

    def __repr__(self):
        return f"Case({self.name}, np={self.np_}, nf={self.nf}, m={self.m}, {self.dtype.name})"

    def ref(self, **faults):
        """f64 nis / nd of the case's (dtype-rounded) inputs."""
        if faults:
            return pair_reference_pf(self.Xv, self.Pv, self.XF, self.PF, self.Z, self.R, np.float64, **faults)
        if self._ref is None:
            self._ref = pair_reference_pf(self.Xv, self.Pv, self.XF, self.PF, self.Z, self.R, np.float64)
        return self._ref

    def raw(self, gates):
        nis, nd = self.ref()
        return decide_cloud(nis, nd, *gates)

    def decisions(self, gates):
        """(idf[m, np], kind[m, np]) of the f64 reference, duplicates resolved."""
        if gates not in self._dec:
            self._dec[gates] = resolve_duplicates(*self.raw(gates))
        return self._dec[gates]

    def summary(self, gates):
        """[m, 4] = (sum w kind 1, kind 2, kind 0, count kind 1) in f64 from the case's (dtype-rounded) weights."""
        kind = self.decisions(gates)[1]
        w = self.w.astype(np.float64)
        return np.stack([((kind == 1) * w).sum(axis=1), ((kind == 2) * w).sum(axis=1), ((kind == 0) * w).sum(axis=1),
                         (kind == 1).sum(axis=1).astype(np.float64)], axis=1)

    def tau(self):
        """-> (tau, largest error of the working-dtype evaluation).  Floor: 64 roundings of the largest value."""
        if self._tau is None:
            nis, nd = self.ref()
            if self.nf == 0:
                self._tau = (0.0, 0.0)
                return self._tau
            lo_nis, lo_nd = pair_reference_pf(self.Xv, self.Pv, self.XF, self.PF, self.Z, self.R, self.dtype.type)
            with np.errstate(invalid="ignore"):
                near = nis < 4.0 * max(g[1] for g in self.gates)
            err, big = 0.0, 1.0
            if near.any():
                assert np.array_equal(np.isnan(lo_nd[near]), np.isnan(nd[near])), self
                e1 = np.abs(lo_nis.astype(np.float64) - nis)[near]
                ok = near & ~np.isnan(nd)
                e2 = np.abs(lo_nd.astype(np.float64) - nd)[ok]
                err = float(max(e1.max(), e2.max() if e2.size else 0.0))
                big = float(max(1.0, np.abs(nis[near]).max(), np.abs(nd[ok]).max() if e2.size else 0.0))
            self._tau = (64.0 * max(err, float(np.finfo(self.dtype).eps) * big), err)
        return self._tau

    def _twin_mask(self, win):
        """[np, m, nf] True at the twins of each (particle, observation)'s winner (the winner included)."""
        group = np.arange(self.nf)
        for g in self.twins:
            group[list(g)] = g[0]
        w0 = np.maximum(win - 1, 0)
        return group[None, None, :] == group[w0][:, :, None]

    def margins(self, gates, duplicates=True):
        """[m, np]: the smallest f64 margin of the comparisons that fix each (idf, kind): every nis against gate1; the
        winner's nd against every other gated nd (twins of the winner excepted: they tie by construction and the lower
        index wins); when nothing wins, the smallest nis against gate2; and, where several observations of a particle
        claim one feature, the nd of every pair of them (identical observation columns excepted: they tie by
        construction and the lower index wins)."""
        g1, g2 = gates
        nis, nd = self.ref()
        idf, kind, nbest = self.raw(gates)
        if self.nf == 0:
            return np.full((self.m, self.np_), np.inf)
        with np.errstate(invalid="ignore"):
            mg = np.where(np.isnan(nis), np.inf, np.abs(nis - g1)).min(axis=2)          # np, m
            win = idf.T                                                                   # np, m
            rivals = (nis < g1) & ~np.isnan(nd) & ~self._twin_mask(win)
            gap = np.where(rivals, nd - nbest.T[:, :, None], np.inf).min(axis=2)
            mg = np.where(win != 0, np.minimum(mg, gap), mg)
            outer = np.where(np.isnan(nis), np.inf, nis).min(axis=2)
            mg = np.where(win == 0, np.minimum(mg, np.abs(outer - g2)), mg)
        mg = mg.T.copy()                                                                  # m, np
        if not duplicates:      # (the search's first look at candidates that will not all enter the case)
            return mg
        same = np.arange(self.m)
        for g in self.same_obs:
            same[list(g)] = g[0]
        for j in range(self.m):
            for k in range(j + 1, self.m):
                if same[j] == same[k]:
                    continue
                clash = (idf[j] != 0) & (idf[j] == idf[k])
                with np.errstate(invalid="ignore"):
                    gapjk = np.where(clash, np.abs(nbest[j] - nbest[k]), np.inf)
                mg[j], mg[k] = np.minimum(mg[j], gapjk), np.minimum(mg[k], gapjk)
        return mg

    def check_twins(self):
        for g in self.twins:
            assert list(g) == sorted(g)
            for t in g[1:]:
                assert np.array_equal(self.XF[:, :, t], self.XF[:, :, g[0]]) and np.array_equal(self.PF[:, :, t], self.PF[:, :, g[0]])
        for g in self.same_obs:
            for t in g[1:]:
                assert np.array_equal(self.Z[:, t], self.Z[:, g[0]])


# ------------------------------------------------------------------------------------------------
# clouds
# ------------------------------------------------------------------------------------------------
def cluster_map(nf, seed, behind=False):
    """nf feature positions in clusters of CLUSTER: centres on rings 15 - 45 m around TRUE_POSE at least 12 m apart, the
    members within 3 m of the centre.  behind: the first cluster lies straight behind the vehicle (relative bearing
    pi), so its predicted bearings fall on both sides of the +-pi cut across the cloud."""
    rng = np.random.default_rng(40_000 + seed)
    ncl = (nf + CLUSTER - 1) // CLUSTER
    centres = []
    k = 0
    while len(centres) < ncl:
        ring = 18.0 + 9.0 * (k // 8)
        ang = TRUE_POSE[2] + 2.0 * np.pi * ((k % 8) + 0.37 * (k // 8)) / 8.0 + 0.3
        centres.append([TRUE_POSE[0] + ring * np.cos(ang), TRUE_POSE[1] + ring * np.sin(ang)])
        k += 1
    if behind and ncl:
        centres[0] = [TRUE_POSE[0] + 25.0 * np.cos(TRUE_POSE[2] + np.pi), TRUE_POSE[1] + 25.0 * np.sin(TRUE_POSE[2] + np.pi)]
    base = np.zeros((2, nf))
    for f in range(nf):
        rad, ang = rng.uniform(1.2, 3.0), rng.uniform(0.0, 2.0 * np.pi)
        off = np.zeros(2) if f % CLUSTER == 0 else rad * np.array([np.cos(ang), np.sin(ang)])
        base[:, f] = np.array(centres[f // CLUSTER]) + off
    return base


def cluster_cloud(np_, nf, dtype, seed, behind=False):
    """tight_particles with its map re-centred on cluster_map (every particle keeps its own jitter), random weights."""
    parts, base0 = tight_particles(np_, max(nf, 0), dtype, seed)
    base = cluster_map(nf, seed, behind)
    rng = np.random.default_rng(41_000 + seed)
    for p in parts:
        jitter = np.asarray(p[3], dtype=np.float64).reshape(2, nf) - base0
        p[3] = np.asfortranarray((base + jitter).astype(dtype))
        p[0] = dtype(rng.uniform(0.5, 1.5) / np_)
    return parts, base


def measure(base, f, pose=TRUE_POSE):
    dx, dy = base[0, f] - pose[0], base[1, f] - pose[1]
    return np.array([np.hypot(dx, dy), np.arctan2(dy, dx) - pose[2]])


# ------------------------------------------------------------------------------------------------
# the deterministic search for decisive observations
# ------------------------------------------------------------------------------------------------
def _search(name, dtype, parts, gen, m, seed, gates=GATES, twins=(), fixed=(), same_obs=(), limit=400, uniform=False,
            distinct=False):
    """The first m observations, in the order `gen(rng)` draws them (batches of 32), that EVERY particle decides with
    margins >= TAU_SEARCH under every gate pair, alone and against the observations kept before them (where two of a
    particle's observations claim one feature, their nd differ by that much).  fixed: columns already in the case.
    uniform: only observations that every particle matches to the SAME feature, a different one each.
    distinct: no two observations of a particle may claim one feature."""
    rng = np.random.default_rng(50_000 + seed)
    bound = TAU_SEARCH[np.dtype(dtype)]
    kept = [np.asarray(c, dtype=np.float64) for c in fixed]
    claims = {g: [] for g in gates}          # per gate pair: (idf[np], nbest[np]) of every kept column

    def note(case, i):
        for g in gates:
            idf, _, nbest = case.raw(g)
            claims[g].append((idf[i], nbest[i]))

    def clear_of_kept(case, i):
        for g in gates:
            idf, _, nbest = case.raw(g)
            if uniform and (idf[i, 0] == 0 or np.any(idf[i] != idf[i, 0]) or any(k[0][0] == idf[i, 0] for k in claims[g])):
                return False
            for kidf, knb in claims[g]:
                clash = (idf[i] != 0) & (kidf == idf[i])
                if distinct and clash.any():
                    return False
                if clash.any() and np.abs(knb[clash] - nbest[i][clash]).min() < bound:
                    return False
        return True

    if kept:
        have = Case("probe", dtype, parts, np.stack(kept, axis=1), gates=gates, twins=twins)
        for i in range(len(kept)):
            note(have, i)
    for _ in range(limit):
        if len(kept) >= m:
            break
        cand = Case("probe", dtype, parts, np.stack([gen(rng) for _ in range(32)], axis=1), gates=gates, twins=twins)
        ok = np.minimum.reduce([cand.margins(g, duplicates=False).min(axis=1) for g in gates]) >= bound
        for i in np.nonzero(ok)[0]:
            if len(kept) < m and clear_of_kept(cand, i):
                kept.append(cand.Z[:, i].astype(np.float64))
                note(cand, i)
    assert len(kept) >= m, (name, len(kept), m)
    return Case(name, dtype, parts, np.stack(kept[:m], axis=1), gates=gates, twins=twins, same_obs=same_obs)


def _near_feature(base, feats, sr=0.6, sb=0.02):
    """Observation generator: the measurement of a random one of `feats` from TRUE_POSE plus noise."""
    feats = list(feats)

    def gen(rng):
        return measure(base, feats[int(rng.integers(len(feats)))]) + rng.normal(size=2) * (sr, sb)
    return gen


# ------------------------------------------------------------------------------------------------
# family A: dense clusters, every size at which the kernels take another path
# ------------------------------------------------------------------------------------------------
C = FEAT_CHUNK
A_KEYS = [  # (np, nf, m, dtype)
    (1, 1, 1, "float32"), (1, 2 * C + 3, OBS_CHUNK + 1, "float32"), (63, C - 1, OBS_CHUNK, "float32"),
    (64, C, 1, "float32"), (65, C + 1, OBS_CHUNK + 1, "float32"), (65, 2 * C + 3, 33, "float32"),
    (130, 2 * C + 3, OBS_CHUNK, "float32"), (130, C + 1, 33, "float32"), (63, 2 * C + 3, 64, "float32"),
    (130, 1, 2, "float32"), (65, 0, OBS_CHUNK + 1, "float32"),
    (1, C, OBS_CHUNK, "float64"), (65, C - 1, 33, "float64"), (130, 2 * C + 3, OBS_CHUNK + 1, "float64"),
    (64, C + 1, 64, "float64"), (63, 1, 1, "float64"),
]


def build_a(np_, nf, m, dtype):
    seed = 1000 * np_ + 10 * nf + m
    parts, base = cluster_cloud(np_, nf, dtype, seed)
    if nf == 0:   # an empty map: whatever is observed is new
        rng = np.random.default_rng(seed)
        return Case(f"A-np{np_}-nf0-m{m}", dtype, parts, np.stack([rng.uniform(10, 40, m), rng.uniform(-3, 3, m)]))
    return _search(f"A-np{np_}-nf{nf}-m{m}", dtype, parts, _near_feature(base, range(nf)), m, seed)


# ------------------------------------------------------------------------------------------------
# the special families (np = 65: two waves of particles, the second with one lane)
# ------------------------------------------------------------------------------------------------
S_NP, S_NF = 65, 2 * C + 3
B_TWINS = ((3, 4), (C - 1, C), (6, 2 * C + 1), (9, 10, C + 10))   # in one chunk, across the boundary 31 | 32, chunks apart


def build_b(dtype):
    """Exact ties: twin features carry identical values in every particle; the observation sits at their measurement
    and the lower index must win, within a chunk of the scan and across chunks (the merge)."""
    parts, base = cluster_cloud(S_NP, S_NF, dtype, 7)
    for p in parts:
        for g in B_TWINS:
            for t in g[1:]:
                p[3][:, t], p[4][:, t] = p[3][:, g[0]], p[4][:, g[0]]
    for g in B_TWINS:
        base[:, list(g[1:])] = base[:, [g[0]]]
    firsts = [g[0] for g in B_TWINS]
    case = _search("B-ties", dtype, parts, _near_feature(base, firsts, sr=0.15, sb=0.004), 8, 7, twins=B_TWINS)
    case.check_twins()
    return case


def _bisect_range(parts, dtype, R, zb, f, target, lo, hi):
    """Range r at which nis of feature f for observation (r, zb) equals target on particle 0 (f64 reference; nis grows
    with r on [lo, hi])."""
    _, Xv, Pv, XF, PF = cloud_arrays(parts[:1], dtype)

    def nis_at(r):
        return pair_reference_pf(Xv, Pv, XF, PF, np.array([[r], [zb]]), np.asarray(R, dtype=dtype))[0][0, 0, f]
    assert nis_at(lo) < target < nis_at(hi), (nis_at(lo), target, nis_at(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if nis_at(mid) < target else (lo, mid)
    return lo


C_FEATS = (0, 6, C - 5, C)   # chunk 0 (first lane, inside, near its end) and the first feature of chunk 1


def build_c(dtype, gates):
    """Gate boundaries: a cloud of identical particles (every lane must agree) and one isolated feature per observation
    whose nis lies 4 TAU_SEARCH under / over gate1 and under / over gate2."""
    parts, base = cluster_cloud(S_NP, C + 1, dtype, 11)
    for p in parts:
        for f in range(C + 1):
            if f not in C_FEATS:                            # the targets have no neighbour inside a gate
                p[3][:, f] = p[3][:, f] + np.array([60.0, 60.0], dtype=dtype)
    parts = [[dtype(q[0])] + [np.array(a, order="F") for a in parts[0][1:]] for q in parts]   # copies of particle 0
    delta = 4.0 * TAU_SEARCH[np.dtype(dtype)]
    R = np.asfortranarray(R_OBS.astype(dtype))
    cols = []
    for f, (gate, sign) in zip(C_FEATS, ((gates[0], -1), (gates[0], 1), (gates[1], -1), (gates[1], 1))):
        z = measure(base, f, pose=tuple(np.asarray(parts[0][1], dtype=np.float64)))
        zb = float(dtype(z[1]))
        r = _bisect_range(parts, dtype, R, zb, f, gate + sign * delta, z[0], z[0] + 12.0)
        cols.append([float(dtype(r)), zb])
    return Case(f"C-gates-{int(gates[0])}-{int(gates[1])}", dtype, parts, np.array(cols).T, gates=(gates,))


def build_d(dtype):
    """Bearings straddling +-pi: the first cluster lies straight behind the vehicle, so across the cloud its predicted
    bearings fall on both sides of the cut; the observations are given near +pi, near -pi and with 2 pi added."""
    parts, base = cluster_cloud(S_NP, C + 1, dtype, 13, behind=True)

    def gen(rng):
        z = measure(base, int(rng.integers(CLUSTER))) + rng.normal(size=2) * (0.3, 0.004)
        z[1] = pi2pi(z[1]) + (0.0, 0.0, 2.0 * np.pi, -2.0 * np.pi)[int(rng.integers(4))]
        return z
    return _search("D-wrap", dtype, parts, gen, 8, 13)


E_FEATS = (0, C, 2 * C)   # an isolated claim each: the first member of three clusters in three chunks


def build_e(dtype):
    """Two and three observations of one particle claim one feature: the order of their nd decides who keeps it.  The
    last column repeats column 0 exactly: equal nd, the lower observation index keeps the feature."""
    parts, base = cluster_cloud(S_NP, S_NF, dtype, 17)
    gens = [_near_feature(base, [f], sr=0.5, sb=0.01) for f in E_FEATS]
    order = [0, 0, 1, 1, 1, 2, 0, 2]   # slot k draws around E_FEATS[order[k]]: two triples and a pair
    kept = []
    case = None
    for k, g in enumerate(order):
        case = _search("E-duplicates", dtype, parts, gens[g], len(kept) + 1, 17 + 100 * k, fixed=kept)
        kept = [case.Z[:, i].astype(np.float64) for i in range(case.m)]
    kept.append(kept[0])
    return Case("E-duplicates", dtype, parts, np.stack(kept, axis=1), same_obs=((0, len(kept) - 1),))


F_BAD, F_WIN, F_LONE = 3, 5, C   # F_BAD sits ahead of F_WIN in one cluster; F_LONE is alone (first feature of chunk 1)


def build_f(dtype):
    """One feature whose nd is NaN (an indefinite PF block: det S < 0) in every particle.  Inside gate1 it must never set
    a record: ahead of the true winner in its cluster the winner still wins; an observation that only the NaN feature
    gates is dropped (kind 0: its nis feeds `outer`), not declared new."""
    parts, base = cluster_cloud(S_NP, S_NF, dtype, 19)
    base[:, F_BAD] = base[:, F_WIN] + [0.2, -0.1]
    for p in parts:
        p[3][:, F_BAD] = p[3][:, F_WIN] + np.array([0.2, -0.1], dtype=dtype)
        for f in (F_BAD, F_LONE):                          # PF = -20 r r^T along the line of sight: S_rr < 0 < S_bb
            r = (base[:, f] - TRUE_POSE[:2]) / np.hypot(*(base[:, f] - TRUE_POSE[:2]))
            p[4][:, f] = (-20.0 * np.outer(r, r)).reshape(-1, order="F").astype(dtype)
        for f in (F_LONE - 2, F_LONE - 1):                 # its cluster mates leave: the lone NaN feature has no neighbour
            p[3][:, f] = p[3][:, f] + np.array([40.0, 40.0], dtype=dtype)
    a = _search("F-nan", dtype, parts, _near_feature(base, [F_WIN], sr=0.2, sb=0.004), 3, 19)
    b = _search("F-nan", dtype, parts, _near_feature(base, [F_LONE], sr=0.2, sb=0.004), 5, 23,
                fixed=[a.Z[:, i].astype(np.float64) for i in range(3)])
    return b


def build_regrow(dtype):
    """70 observations on 9 particles: more than the 64 the handle's tables start with.  -> (its first 9 columns as a
    case of their own, the whole)."""
    parts, base = cluster_cloud(9, C + 1, dtype, 29)
    big = _search("G-regrow-m70", dtype, parts, _near_feature(base, range(C + 1)), 70, 29)
    return Case("G-regrow-m9", dtype, parts, big.Z[:, :OBS_CHUNK + 1].astype(np.float64)), big


def build_uniform(np_, nf, m, dtype, n_new=0, seed=31):
    """m observations that EVERY particle matches to the same feature (a different one each: the table is uniform and
    complete), followed by n_new observations far from every feature (new for every particle)."""
    parts, base = cluster_cloud(np_, nf, dtype, seed + np_ + m)
    firsts = list(range(0, nf, CLUSTER))
    for p in parts:                                         # the cluster mates leave: nobody disputes a first member
        for f in range(nf):
            if f % CLUSTER:
                p[3][:, f] = p[3][:, f] + np.array([60.0, 60.0], dtype=dtype)
    case = _search(f"U-np{np_}-m{m}", dtype, parts, _near_feature(base, firsts, sr=0.15, sb=0.004), m, seed, uniform=True)
    if n_new:
        def far(rng):
            return np.array([rng.uniform(70.0, 90.0), rng.uniform(-3.0, 3.0)])
        case = _search(f"U-np{np_}-m{m}+{n_new}", dtype, parts, far, m + n_new, seed + 1,
                       fixed=[case.Z[:, i].astype(np.float64) for i in range(m)])
    return case


SPECIAL_KEYS = [(fam, dt) for fam in ("B", "C0", "C1", "D", "E", "F") for dt in ("float32", "float64")]
CASE_KEYS = [("A",) + k for k in A_KEYS] + SPECIAL_KEYS
# the cases of the other GPU tests: table growth, the consumers (uniform complete tables; a mixed table), the whole step
REGROW_KEYS = [("G9", "float32"), ("G70", "float32")]
UNIFORM_KEYS = [("U", 17, 30, 9, 0, "float32"), ("U", 17, 30, 9, 0, "float64"), ("U", 65, 60, 17, 0, "float32"),
                ("U", 65, 60, 17, 0, "float64")]
STEP_KEYS = [("U", 130, 20, 6, 3, "float32"), ("U", 130, 20, 6, 3, "float64")]
MIXED_KEYS = [("A", 65, C + 1, OBS_CHUNK + 1, "float32"), ("A", 130, 2 * C + 3, OBS_CHUNK + 1, "float64"), ("E", "float32")]
EKF_KEYS = [("X", 2 * C + 3, OBS_CHUNK + 1, "float32"), ("X", C + 1, OBS_CHUNK, "float64")]
ALL_KEYS = CASE_KEYS + REGROW_KEYS + UNIFORM_KEYS + STEP_KEYS + EKF_KEYS
_CACHE = {}


def case_id(key):
    return "-".join(str(k) for k in key)


def get_case(key):
    """The case of one key, built once per process."""
    if key not in _CACHE:
        dtype = np.dtype(key[-1]).type
        fam = key[0]
        if fam == "A":
            c = build_a(key[1], key[2], key[3], dtype)
        elif fam == "X":   # one particle in a dense map, no feature claimed twice: the cross-check against the EKF
            parts, base = cluster_cloud(1, key[1], dtype, 37)
            c = _search(f"X-nf{key[1]}-m{key[2]}", dtype, parts, _near_feature(base, range(key[1])), key[2], 37, distinct=True)
        elif fam == "U":
            c = build_uniform(key[1], key[2], key[3], dtype, n_new=key[4])
        elif fam in ("G9", "G70"):
            _CACHE[("G9", key[-1])], _CACHE[("G70", key[-1])] = build_regrow(dtype)
            return _CACHE[key]
        elif fam == "B":
            c = build_b(dtype)
        elif fam in ("C0", "C1"):
            c = build_c(dtype, GATES[int(fam[1])])
        elif fam == "D":
            c = build_d(dtype)
        elif fam == "E":
            c = build_e(dtype)
        else:
            c = build_f(dtype)
        _CACHE[key] = c
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------
# the consumers, per particle, on the CPU oracle
# ------------------------------------------------------------------------------------------------
def copy_parts(parts, dt):
    return [[dt(p[0])] + [np.array(a, dtype=dt, order="F") for a in p[1:]] for p in parts]


def predicted_parts(parts, dt, quirks=REF_EXACT):
    """Every particle after PF::predict with pf_builders.PREDICT / Q_CTRL (gives each a positive-definite Pv)."""
    o = Oracle(dt, quirks)
    ps = copy_parts(parts, dt)
    for p in ps:
        o.pf_predict(p[1], p[2], PREDICT[0], PREDICT[1], Q_CTRL.astype(dt), PREDICT[2], PREDICT[3])
    return ps


def consumer_reference(parts, dt, Z, R, idf, use, normals, miss, quirks=REF_EXACT, proposal=True):
    """Each particle through Oracle.pf_sample_proposal (when `proposal`) and pf_feature_update on ITS OWN compacted
    (Z, idf) -- the observations with use[j] = 1 and idf[j, p] != 0, in order -- then the miss_likelihood factor of every
    used observation it has no match for, in observation order.  idf: [m, np].  -> particles in precision dt."""
    o = Oracle(dt, quirks)
    ps = copy_parts(parts, dt)
    Z = np.asarray(Z, dtype=dt).reshape(2, -1, order="F")
    R = np.asfortranarray(np.asarray(R, dtype=dt))
    use = np.asarray(use)
    for i, p in enumerate(ps):
        sel = [j for j in range(Z.shape[1]) if use[j] and idf[j, i] != 0]
        Zc = np.asfortranarray(Z[:, sel])
        ic = np.array([idf[j, i] for j in sel], dtype=np.int32)
        if proposal:
            w = np.array([p[0]], dtype=dt)
            o.pf_sample_proposal(w, p[1], p[2], p[3], p[4], Zc, ic, R, np.asarray(normals)[:, i].astype(dt))
            for j in range(Z.shape[1]):
                if use[j] and idf[j, i] == 0:
                    w[0] = w[0] * dt(miss)
            p[0] = w[0]
        if len(sel):
            o.pf_feature_update(p[1], p[3], p[4], Zc, ic, R)
    return ps
