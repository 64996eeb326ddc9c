"""Inputs, the f64 reference drive and the check of test_batch_edges_gpu.py / test_batch_edges_cpu.py: the batched
Monte-Carlo engine's windows at the edges of their kernel dispatch (cslam_ekf_batch.hip: window(), flush(), queue_step()).

A SEGMENT is: get_state of every instance (drains everything, no pending column) -> update(m_prev) -> h x (predict +
observe_heading) -> optionally one more, held, predict -> update(m) -> get_state.  The second update's flush applies
kp = 2 m_prev + h pending columns (a 129th column forces a flush of 128 first), the final get_state's 2 m.  The reference
re-runs the same calls on OracleState in f32 and f64 from the state read at the start of the segment.

Every handle first runs a PRELUDE of four m = 32 steps through run(): two windows of 128 columns, which leave both
pending regions full of data, so a column that flush() fails to zero-fill is a stale value and not the zero of a fresh
allocation.

The scenario (edge_scenario) gives the heading a variance of R_phi / 50, 80 % of it shared with two or three map rows, one
per 128-row tile, of landmarks that no update observes (reserved_rows), and the control noise on the steering angle is
small.  A heading step then removes about 2 % of that correlation instead of all of it, so the LAST of 65 heading columns
still changes P by more than P_RTOL allows.  With helpers.make_scenario's pose block (P22 = 1e-2 against R_phi = 3e-8)
the first heading step takes everything and every later column changes P by ~1e-7, invisible to any check; a low-rank
correlation is gone after the first update.  The column j steps on changes P_ii by at most rho_0^2 P_ii / (4 j), reached
at P22 = R_phi / j: that is why P22 starts near R_phi / 64.  P_xx and P_yy keep make_scenario's 1e-2 scale, so the pose
stripe of an update stays visible too.
"""
import collections

import numpy as np

from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs
from pyoracle import Oracle, REF_EXACT, TEXTBOOK  # noqa: F401  (REF_EXACT: for the callers)

F32 = np.dtype(np.float32)
FAIR = 4.0
Q = np.diag([0.18, 4e-8]).astype(np.float32)   # (sigma_swa = 0.011 deg: a predict adds 5e-12 rad^2 to P22)
R = np.diag([0.08, 0.0024]).astype(np.float32)
V, WB, DT = 83.33, 73.0, 0.01
# observeHeading's noise, as the engine forms it: float sigmaPhi = 0.01F * pi / 180.0F; R = pow(sigmaPhi, 2)
_SIGMA_PHI = np.float32((float(np.float32(0.01)) * np.pi) / 180.0)
R_PHI = float(_SIGMA_PHI * _SIGMA_PHI)
P22_TARGET = R_PHI / 50.0
PRELUDE_STEPS, PRELUDE_M = 4, 32

CONTROLS = ("no_last_heading_column", "drop_last_observation", "stale_column", "predict_after_update", "swap_gain_rows")

Segment = collections.namedtuple("Segment", "family N I m_prev h hold m env seed")


def seg_id(s):
    env = "".join(f"-{k.replace('CSLAM_', '')}={v}" for k, v in s.env)
    return f"N{s.N}-I{s.I}-mp{s.m_prev}-h{s.h}{'-held' if s.hold else ''}-m{s.m}{env}"


def _seg(family, m_prev, h, m, N=70, I=2, hold=False, env=()):
    seed = 1000 * N + 100 * m_prev + 10 * h + m + (5000 if hold else 0)
    return Segment(family, N, I, m_prev, h, hold, m, tuple(env), seed)


# (m_prev, h -> kp at the second update's flush); m = 16.  64|65 and 96|97: the P-GEMM classes <0,2,32> | <0,4,24> |
# <0,4,32>; 65, 97, 127, 37, 3: a zero-filled column below k8; 128: nothing to fill; 129: the forced flush, then kp = 1
PGEMM = [_seg("pgemm", mp, h, 16) for mp, h in
         ((32, 0), (32, 1), (32, 8), (32, 32), (32, 33), (32, 63), (32, 64), (32, 65), (1, 0), (1, 1), (16, 5))]
# the chain <16 | 32 | 64> at m = 8|9 and 16|17, the wide kernel general | k64 at 31|32 (k = 62: two padded factor
# columns), each with and without a held predict riding inside the window (pp_a.valid)
CHAIN = [_seg("chain", 16, 2, m, hold=hold) for hold in (False, True) for m in (8, 9, 16, 17, 31, 32)]
# n = 127, 129, 255, 257: the last row at and just past a 128-row tile edge
TILES = [_seg("tiles", mp, h, m, N=N) for N in (62, 63, 126, 127) for mp, h, m in ((32, 1, 17), (16, 0, 9))]
COUNT = [_seg("count", 32, 33, 31, I=I) for I in (1, 2, 3)]
AB = [_seg("ab", 32, 1, 32, env=(("CSLAM_LA_K64", "0"),)), _seg("ab", 16, 2, 17, env=(("CSLAM_BATCH_WIDE_PAIRS", "1"),))]
SEGMENTS = PGEMM + CHAIN + TILES + COUNT + AB
FAMILIES = ("pgemm", "chain", "tiles", "count", "ab")


def pending_columns(seg):
    """kp at the second update's flush (after a forced flush: what is left), and the columns the P-GEMM class reads"""
    kp = 2 * seg.m_prev + seg.h
    if kp > 128:
        kp -= 128
    k8 = (kp + 7) // 8 * 8
    return kp, (64 if k8 <= 64 else (96 if k8 <= 96 else 128))


def applicable(seg, control):
    if control == "no_last_heading_column":
        return seg.h > 0
    if control == "predict_after_update":
        return seg.hold
    if control == "stale_column":
        kp, cover = pending_columns(seg)
        return kp < cover  # (kp = 64, 96, 128: nothing is zero-filled)
    return True


def reserved_rows(N):
    """Rows of P that carry the heading's correlation with the map: x of landmark 2, y of landmark 64 (row 130, the second
    tile; when the map has it) and x of landmark N - 1 (the last tile but for landmark N).  No update observes these
    landmarks, so the correlation is still there when the last heading column is formed."""
    return [5] + ([130] if N >= 66 else []) + [3 + 2 * (N - 2)]


def reserved_landmarks(N):
    return sorted({(r - 3) // 2 + 1 for r in reserved_rows(N)})


def pick_landmarks(N, m, seed):
    """m distinct 1-based landmarks: the tile-straddling ones (f = 63 mod 64: rows 127|128, 255|256) and the last one
    first, then random among those not reserved (the pattern of test_kernel_edges_gpu.py)."""
    rng = np.random.default_rng(seed)
    special = list(dict.fromkeys([f for f in range(63, N + 1, 64)] + [N]))[:m]
    skip = set(special) | set(reserved_landmarks(N))
    rest = [f for f in rng.permutation(N) + 1 if f not in skip]
    idf = np.array(special + rest[: m - len(special)], dtype=np.int32)
    return idf[rng.permutation(m)]


def straddling_landmark(N):
    return 63 if N >= 63 else N


def edge_scenario(N, seed, corr=0.5):
    """B = s (I + U U^T) s as helpers.make_scenario builds it (P_xx, P_yy at 1e-2), with a heading that is independent in
    B and has 0.2 x R_phi / 50 of variance; then P0 = T B T^T with T = I + e_2 g^T: the heading gains g . x, g equal on
    reserved_rows(N), sized so that P22 = R_phi / 50 and 80 % of it is shared with those rows.  SPD by construction."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    U = rng.normal(size=(n, 4)) * corr
    U[2, :] = 0.0
    B = np.eye(n) + U @ U.T
    s = np.ones(n)
    s[:2] = 0.1
    s[2] = np.sqrt(0.2 * P22_TARGET)
    B = B * s[:, None] * s[None, :]
    rows = reserved_rows(N)
    g = np.zeros(n)
    g[rows] = np.sqrt(0.8 * P22_TARGET / B[np.ix_(rows, rows)].sum())
    T = np.eye(n)
    T[2, :] += g
    P = T @ B @ T.T
    P = 0.5 * (P + P.T)
    X = np.concatenate([[1.0, -2.0, 0.3], rng.uniform(-500, 500, size=2 * N)])
    return X.astype(np.float32), np.array(P, dtype=np.float32, order="F")


def seg_states(seg):
    """instance i's scenario depends on (N, i) only: instance 0 is the same filter in a batch of 1, 2 or 3"""
    return [edge_scenario(seg.N, seed=7 * seg.N + i) for i in range(seg.I)]


def _swa(t):
    return 0.02 * ((t % 3) - 1)


def _factor_panel(o64, X, P, n, idf):
    """W1 = P H^T L^-T (S = L L^T) in f64: what a textbook update of these landmarks leaves pending, n x 2m"""
    H = np.zeros((2 * len(idf), n))
    for i, f in enumerate(idf):
        H[2 * i:2 * i + 2] = o64.observe_model(np.ascontiguousarray(X, dtype=np.float64), n, int(f))[1]
    P = np.asarray(P, dtype=np.float64)
    PHT = P @ H.T
    S = H @ PHT + np.kron(np.eye(len(idf)), R.astype(np.float64))
    L = np.linalg.cholesky(0.5 * (S + S.T))
    return np.linalg.solve(L, PHT.T).T


Prelude = collections.namedtuple("Prelude", "ctrl obs ends codes panels")


def prelude(states, quirks=TEXTBOOK):
    """PRELUDE_STEPS x (predict + update of 32 landmarks) per instance on the f32 oracle.  obs[t][i] = (Z, idf);
    ends[i]: the oracle's state afterwards; panels[i]: n x 128, a model (f64) of what the first window leaves in the
    region that the segment's first update writes to -- the stale values behind its columns."""
    N = (states[0][0].shape[0] - 3) // 2
    o64 = Oracle(np.float64)
    ctrl = [(V, _swa(t + 1)) for t in range(PRELUDE_STEPS)]
    orc = [OracleState(X, P, np.float32, quirks) for X, P in states]
    obs, codes, panels = [], [], [[] for _ in states]
    for t, (v, swa) in enumerate(ctrl):
        row = []
        for i, s in enumerate(orc):
            s.predict(v, swa, Q, WB, DT)
            idf = pick_landmarks(N, PRELUDE_M, seed=31 * N + 7 * t + i)
            Z = make_obs(s.x(), idf, np.float32, seed=900 + 13 * t + i)
            if t < 2:
                panels[i].append(_factor_panel(o64, s.x(), s.p(), s.n, idf))
            codes.append(s.update(Z, R, idf, True))
            row.append((Z, idf))
        obs.append(row)
    return Prelude(ctrl, obs, [(s.x(), s.p()) for s in orc], codes, [np.hstack(p) for p in panels])


def np_update(s, Z, idf, swap=None):
    """The textbook batch update of an f64 OracleState in numpy: X += K V, P -= K S K^T, K = P H^T S^-1.  swap = f:
    the two rows of landmark f are exchanged in K (a negative control)."""
    n, o = s.n, s.o
    m = len(idf)
    H, Vv = np.zeros((2 * m, n)), np.zeros(2 * m)
    X = s.x()
    for i, f in enumerate(idf):
        zp, h = o.observe_model(X, n, int(f))
        H[2 * i:2 * i + 2] = h
        Vv[2 * i] = Z[0, i] - zp[0]
        Vv[2 * i + 1] = o.pi2pi(Z[1, i] - zp[1])
    P = s.p()
    PHT = P @ H.T
    S = H @ PHT + np.kron(np.eye(m), R.astype(np.float64))
    S = 0.5 * (S + S.T)
    K = np.linalg.solve(S, PHT.T).T
    if swap is not None:
        r = 3 + 2 * (swap - 1)
        K[[r, r + 1]] = K[[r + 1, r]]
    s.X[:n] = X + K @ Vv
    s.P[:n, :n] = P - K @ S @ K.T


Drive = collections.namedtuple("Drive", "states inputs codes s_min")


def drive(seg, starts, dtype, inputs=None, fault=None, stale=None, quirks=TEXTBOOK):
    """The segment on OracleState in `dtype` from `starts` (one (X, P) per instance).  inputs = None (f64 only): the
    observations are made from this drive's own estimate at the time of each update, the heading angles are instance 0's
    current heading plus a fixed perturbation; they are returned for the f32 drive and the device.  fault: one of CONTROLS
    (stale: per instance the n-vector added as w w^T to the map block's downdate)."""
    dt = np.dtype(dtype)
    gen = inputs is None
    assert not gen or dt == np.float64
    assert fault is None or (dt == np.float64 and fault in CONTROLS and applicable(seg, fault))
    if gen:
        inputs = {"obs1": [], "obs2": [], "phi": []}
    st = [OracleState(X.astype(dt), np.asfortranarray(P.astype(dt)), dt, quirks) for X, P in starts]
    n = st[0].n
    Rd = R.astype(dt)
    codes, s_min = [], np.inf

    def observe(key, i, s, m, seed):
        if gen:
            idf = pick_landmarks(seg.N, m, seed=seed + 17 * i)
            inputs[key].append((make_obs(s.x(), idf, np.float32, seed=seed + 3 + i), idf))
        return inputs[key][i]

    for i, s in enumerate(st):
        Z, idf = observe("obs1", i, s, seg.m_prev, seg.seed)
        codes.append(s.update(Z.astype(dt), Rd, idf, True))
    for t in range(seg.h):
        for s in st:
            s.predict(V, _swa(t), Q, WB, DT)
        if gen:
            inputs["phi"].append(float(st[0].X[2]) + 5e-5 * np.cos(1.0 + t))
        for s in st:
            s_min = min(s_min, float(s.P[2, 2]) + R_PHI)
            keep = s.P[3:n, 3:n].copy() if (fault == "no_last_heading_column" and t == seg.h - 1) else None
            s.observe_heading(inputs["phi"][t], True)
            if keep is not None:
                s.P[3:n, 3:n] = keep
    if seg.hold and fault != "predict_after_update":
        for s in st:
            s.predict(V, _swa(seg.h), Q, WB, DT)
    for i, s in enumerate(st):
        Z, idf = observe("obs2", i, s, seg.m, seg.seed + 50)
        if fault == "drop_last_observation":
            Z, idf = np.asfortranarray(Z[:, :-1]), idf[:-1]
        if fault == "swap_gain_rows":
            np_update(s, Z.astype(dt), idf, swap=straddling_landmark(seg.N))
            codes.append(0)
        else:
            codes.append(s.update(Z.astype(dt), Rd, idf, True))
    if seg.hold and fault == "predict_after_update":
        for s in st:
            s.predict(V, _swa(seg.h), Q, WB, DT)
    if fault == "stale_column":
        for i, s in enumerate(st):
            w = np.asarray(stale[i], dtype=np.float64)[3:n]
            s.P[3:n, 3:n] -= np.outer(w, w)
    return Drive([(s.x(), s.p()) for s in st], inputs, codes, s_min)


def stale_columns(seg, pre):
    """per instance: column kp of the modelled prelude panel, the value a missing zero-fill would read"""
    kp, _ = pending_columns(seg)
    return [p[:, kp] for p in pre.panels]


def check_segment(tag, got, lo, hi):
    """THE check: every instance's (X, P) against the f32 oracle, the f64 oracle as the fairness reference, at the
    project's per-call tolerances and fair = 4."""
    assert len(got) == len(lo) == len(hi)
    for i, ((X, P), (Xl, Pl), (Xh, Ph)) in enumerate(zip(got, lo, hi)):
        assert_close(f"{tag} X[{i}]", X, Xl, X_RTOL[F32], Xh, fair=FAIR)
        assert_close(f"{tag} P[{i}]", P, Pl, P_RTOL[F32], Ph, fair=FAIR)


def assert_symmetric(P):
    """Exactly symmetric outside the 3 x 3 pose block (one stored copy / explicit mirrors).  The pose block is the dense
    Gv Pvv Gv^T + Gu Q Gu^T of EKF.cpp:430-440 kept in the pose stripe: symmetric to 16 roundings at the size of its diagonal, as
    in the reference (the f32 oracle's pose block differs from its transpose by 4e-10 on these inputs)."""
    M = np.array(P, dtype=np.float64)
    V = M[:3, :3].copy()
    M[:3, :3] = 0
    assert np.array_equal(M, M.T), "P must be exactly symmetric outside the pose block"
    d = np.sqrt(np.abs(np.diag(V)))
    assert np.all(np.abs(V - V.T) <= 16 * np.finfo(np.float32).eps * np.outer(d, d)), "pose block: not symmetric to rounding"


def errors(got, hi):
    """max over the instances of |got - hi|_max for X and P"""
    ex = max(float(np.abs(np.asarray(g[0], np.float64) - h[0]).max()) for g, h in zip(got, hi))
    ep = max(float(np.abs(np.asarray(g[1], np.float64) - h[1]).max()) for g, h in zip(got, hi))
    return ex, ep


def control_margin(bad, lo, hi):
    """What a fault changes over what the check lets pass, fair * e_ref + rtol * scale: per instance the larger of the X
    and the P ratio, then the SMALLEST over the instances (> 1: every instance alone rejects the fault)."""
    out = []
    for (Xb, Pb), (Xl, Pl), (Xh, Ph) in zip(bad, lo, hi):
        r = []
        for b, l, h, rtol in ((Xb, Xl, Xh, X_RTOL[F32]), (Pb, Pl, Ph, P_RTOL[F32])):
            l64 = np.asarray(l, np.float64)
            scale = max(1.0, float(np.abs(l64).max()))
            r.append(float(np.abs(b - h).max()) / (FAIR * float(np.abs(l64 - h).max()) + rtol * scale))
        out.append(max(r))
    return min(out)


# ------------------------------------------------------------------------------------------------ run() windows
RunCase = collections.namedtuple("RunCase", "quirks N m steps same")
RUN_CASES = [
    RunCase(TEXTBOOK, 70, 17, 4, False),   # k = 34: the K = 64 chain first applies; kp = 68: the first 96-class P-GEMM
    RunCase(TEXTBOOK, 70, 25, 4, False),   # kp = 100: the first 128-class P-GEMM
    RunCase(TEXTBOOK, 70, 31, 4, False),   # k = 62: two padded factor columns; the general wide kernel's last size
    RunCase(TEXTBOOK, 63, 32, 3, False),   # the k64 wide kernel at n = 129; the last window holds one update
    RunCase(TEXTBOOK, 62, 9, 2, False),    # the K = 32 chain's first size at n = 127
    RunCase(TEXTBOOK, 70, 17, 4, True),    # every step observes the same landmarks: the carry step does the most work
    RunCase(REF_EXACT, 70, 17, 4, False),  # the reference's gain on the healthy scenario
]


def run_case_id(c):
    return f"{'ref_exact' if c.quirks == REF_EXACT else 'textbook'}-N{c.N}-m{c.m}-steps{c.steps}{'-same' if c.same else ''}"


def run_loads(case, instances=2):
    """Workloads as test_batch_gpu.py builds them (seeded per instance; the healthy scenario for REF_EXACT), whose
    observed sets come from pick_landmarks: landmark 63 and the last one are in every set."""
    from conan_slam_amd.synth import Workload, normal

    class EdgeWorkload(Workload):
        def observations(self, t):
            s = 1000 * self.seed
            pick = pick_landmarks(self.N, self.m, seed=s + (0 if case.same else 7919 * (t + 1))) - 1
            if case.same:
                pick = pick[np.random.default_rng(s + t).permutation(self.m)]
            pose = self.true_pose_after(t)
            dx, dy = self.LM[0, pick] - pose[0], self.LM[1, pick] - pose[1]
            nz = normal(s + 5 + 104729 * (t + 1), np.arange(2 * self.m, dtype=np.uint64))
            Z = np.empty((2, self.m), dtype=np.float64)
            Z[0] = np.sqrt(dx * dx + dy * dy) + nz[0::2] * np.sqrt(float(self.R[0, 0]))
            Z[1] = np.arctan2(dy, dx) - pose[2] + nz[1::2] * np.sqrt(float(self.R[1, 1]))
            return np.asfortranarray(Z.astype(self.dtype)), (pick + 1).astype(np.int32)

    healthy = case.quirks == REF_EXACT
    loads = [EdgeWorkload(case.N, case.m, np.float32, seed=300 + r, corr=0.02 if healthy else 0.5) for r in range(instances)]
    if healthy:
        for w in loads:
            s = np.ones(w.n, np.float32)
            s[:3] = 0.1
            w.P0 = np.asfortranarray(w.P0 * s[:, None] * s[None, :])
    ctrl = [Workload(case.N, case.m, np.float32, seed=0, build_p=False).controls(t) for t in range(case.steps)]
    return loads, ctrl


def run_oracle(w, ctrl, obs, quirks, dtype):
    """predict + update per step on the oracle (its dense-order fast path, as test_batch_gpu.py) -> (X, P, codes)"""
    o = Oracle(dtype, quirks)
    X, P = w.X0.astype(dtype), np.array(w.P0, dtype=dtype, order="F")
    codes = []
    for (v, swa), (Z, idf) in zip(ctrl, obs):
        o.predict(X, P, w.n, v, swa, w.QE.astype(dtype), w.wb, w.dt)
        codes.append(o.update(X, P, w.n, Z.astype(dtype), w.RE.astype(dtype), idf, True, fast=True))
    return X, P, codes
