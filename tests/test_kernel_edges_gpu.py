"""The single-filter update path at the edges of its kernel dispatch (cslam_ekf.hip: launch_factor_args, launch_gain,
launch_downdate and the gather's pending-column corrections), look-ahead windows whose second update re-observes the
first one's landmarks, and device-resident inputs that the caller rewrites between calls.

Each stage is checked against a float64 computation of the SAME operation on the kernel's own inputs (debug_last_update)
with a rounding bound built from the operands' magnitudes, and every such check is shown to be tight: the same check
must reject the kernel's output with one element moved by 1e-4 (f32) / 1e-9 (f64) relative (host side, in numpy).

Landmark f occupies rows 3 + 2(f - 1) and 4 + 2(f - 1): for f = 63 (mod 64) the two rows fall into different 128-row
tiles of the block-lower storage, so the observed sets always include those landmarks (when the map has them) and the
last one.
"""
import numpy as np
import pytest

from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs, make_scenario
from pyoracle import Oracle, REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu

REL = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-9}
R22 = np.diag([0.08, 0.0024])


def _u(dtype):
    return float(np.finfo(dtype).eps) / 2  # unit roundoff


def pick_landmarks(N, m, seed):
    """m distinct 1-based landmarks: the tile-straddling ones (f = 63 mod 64) and the last one first, then random."""
    rng = np.random.default_rng(seed)
    special = [f for f in range(63, N + 1, 64)] + [N]
    special = list(dict.fromkeys(special))[:m]
    rest = [f for f in rng.permutation(N) + 1 if f not in special]
    idf = np.array(special + rest[: m - len(special)], dtype=np.int32)
    return idf[rng.permutation(m)]


def check_bound(name, got, ref, bound, rel, scale=None):
    """|got - ref| <= bound element by element; then the negative control: the element where the check is most
    sensitive (largest |ref| / bound) moved by rel * |ref| away from ref must be rejected.  `scale` replaces |ref| as
    what the perturbation is relative to, for a result that is itself a cancellation of larger operands."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    mag = np.abs(ref) if scale is None else np.broadcast_to(np.asarray(scale, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    worst = float((err / bound).max())
    assert worst <= 1.0, f"{name}: error / bound = {worst:.3g} (max error {float(err.max()):.3e})"
    i = np.unravel_index(int(np.argmax(mag / bound)), ref.shape)
    bad = got.copy()
    s = 1.0 if got[i] >= ref[i] else -1.0
    bad[i] = ref[i] + s * (err[i] + rel * mag[i])
    assert float((np.abs(bad - ref) / bound).max()) > 1.0, f"{name}: the bound does not catch a {rel:g} relative error"
    return worst


def innovation_and_jacobian(X, idf, Z):
    """f64 V and H of a batch at X (slam.h:243 inputs), from the f64 oracle's observation model."""
    o = Oracle(np.float64)
    X = np.asarray(X, dtype=np.float64)
    n, k = X.shape[0], 2 * len(idf)
    H = np.zeros((k, n))
    V = np.zeros(k)
    Zp = np.zeros(k)
    Z = np.asarray(Z, dtype=np.float64)
    for i, f in enumerate(idf):
        zp, h = o.observe_model(X, n, int(f))
        H[2 * i:2 * i + 2, :] = h
        Zp[2 * i:2 * i + 2] = zp
        V[2 * i] = Z[0, i] - zp[0]
        V[2 * i + 1] = o.pi2pi(Z[1, i] - zp[1])
    return V, H, Zp


def check_stages(d, X, P, idf, Z, R, dtype, quirks):
    """Every stage of the last update against f64 on the kernel's own inputs."""
    dt = np.dtype(dtype)
    u, rel = _u(dtype), REL[dt]
    k = 2 * len(idf)
    assert d["PHT"].shape[1] == k
    P64 = np.asarray(P, dtype=np.float64)
    V64, H, Zp = innovation_and_jacobian(X, idf, Z)
    aH = np.abs(H)
    # V: Z - h(X): range / bearing evaluated in the working precision, then a cancellation of Z and h(X) (so the
    # negative control perturbs V relative to those operands)
    zs = np.abs(np.asarray(Z, np.float64).reshape(-1, order="F")) + np.abs(Zp) + np.pi
    check_bound("V", d["V"], V64, 16 * u * zs, rel, scale=zs)
    # PHT = P H^T: five non-zero columns per row of H, H itself rounded
    pht = d["PHT"].astype(np.float64)
    check_bound("PHT", pht, P64 @ H.T, 16 * u * (np.abs(P64) @ aH.T) + 1e-300, rel)
    # S = H PHT + R from the kernel's own PHT (symmetrised, slam.h:246)
    R64 = np.kron(np.eye(len(idf)), np.asarray(R, np.float64))
    S64 = H @ pht + R64
    S64 = 0.5 * (S64 + S64.T)
    Sg = d["S"].astype(np.float64)
    # (a kernel may form S from the compact block of P rather than from PHT: the bound is at the size of H P H^T's terms)
    hph = aH @ (np.abs(P64) @ aH.T)
    check_bound("S", Sg, S64, 16 * u * (hph + aH @ np.abs(pht) + np.abs(R64)) + 1e-300, rel)
    assert np.array_equal(Sg, Sg.T), "S must be exactly symmetric"
    # G = gain_factor(S) of the kernel's own S: Cholesky forward error ~ k u cond(S^), S^ = D^-1/2 S D^-1/2
    G64, code = Oracle(np.float64, quirks).gain_factor(np.asfortranarray(Sg))
    assert code == 0
    dsq = np.sqrt(np.diag(Sg))
    Shat = Sg / np.outer(dsq, dsq)
    kappa = float(np.linalg.cond(Shat))
    lower = quirks == REF_EXACT  # G = L^-1 (reference quirk) or L^-T (textbook)
    scale = (lambda G: G * dsq[None, :]) if lower else (lambda G: G * dsq[:, None])
    Gg = d["G"].astype(np.float64)
    gh = scale(G64)
    check_bound("G", scale(Gg), gh, k * u * kappa * float(np.abs(gh).max()), rel)
    if quirks == TEXTBOOK:
        E = Gg.T @ Sg @ Gg - np.eye(k)
        assert float(np.abs(E).max()) <= (k + 8) * u * kappa, f"|G^T S G - I| = {float(np.abs(E).max()):.3e}"
    # W1 = PHT G: a dot product of length k (the rounding bound of the P-GEMM test)
    check_bound("W1", d["W1"], pht @ Gg, (k + 2) * u * (np.abs(pht) @ np.abs(Gg)) + 1e-300, rel)
    return kappa


KS_F32 = [2, 4, 6, 16, 18, 32, 34, 64, 66, 96, 98, 126, 128, 130, 136, 138, 194, 196]
KS_F64 = [2, 4, 6, 16, 18, 32, 34, 64, 66, 94, 96, 98, 126, 128, 136]
SMALL_N = [62, 63, 64]  # n = 127, 129, 131: the last rows at, just past and two past a 128-row tile edge
MULTI_N = 317           # n = 637: five tiles, landmarks 63, 127, 191, 255 straddle


def _a_cases():
    out = []
    for dtype, ks in ((np.float32, KS_F32), (np.float64, KS_F64)):
        for i, k in enumerate(ks):
            small = SMALL_N[i % 3]
            for N in (small, MULTI_N):
                if k // 2 <= N:
                    out.append(pytest.param(dtype, k, N, id=f"{np.dtype(dtype).name}-k{k}-N{N}"))
    return out


def scenario(N, dtype, seed):
    """A well-conditioned covariance (small pose block, weak correlations): S^ stays near the identity, so the gain's
    rounding bound is tight, and the oracle's codes are 0 under both quirk sets."""
    return make_scenario(N, dtype, seed=seed, corr=0.1, pose_scale=1e-4)


@pytest.mark.parametrize("quirks", [TEXTBOOK, REF_EXACT], ids=["textbook", "ref_exact"])
@pytest.mark.parametrize("dtype,k,N", _a_cases())
def test_update_stages_at_every_dispatch_edge(gpu_required, dtype, k, N, quirks):
    from conan_slam_amd import EKF

    m = k // 2
    X, P = scenario(N, dtype, seed=1000 + 7 * k + N)
    idf = pick_landmarks(N, m, seed=k + N)
    Z = make_obs(X, idf, dtype, seed=k)
    R = R22.astype(dtype)
    eng = EKF(N, dtype=dtype, quirks=quirks)
    eng.set_state(X, P)
    eng.update(Z, R, idf, batch=True)
    d = eng.debug_last_update()
    orc = OracleState(X, P, dtype, quirks)
    hi = OracleState(X.astype(np.float64), P.astype(np.float64), np.float64, quirks)
    assert orc.update(Z, R, idf, True) == 0
    hi.update(Z.astype(np.float64), R.astype(np.float64), idf, True)
    assert eng.factor_status() == 0
    check_stages(d, X, P, idf, Z, R, dtype, quirks)
    Xg, Pg = eng.get_state()
    dt = np.dtype(dtype)
    assert_close("X", Xg, orc.x(), X_RTOL[dt], hi.x())
    assert_close("P", Pg, orc.p(), P_RTOL[dt], hi.p())
    eng.close()


# ------------------------------------------------------------------------------------------------ B: gather corrections
def _heading(s, step):
    s.observe_heading(0.3 + 1e-3 * step, True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("defer", [128, 256])
@pytest.mark.parametrize("pending", ["h1", "h16", "h17", "k64", "k64+h1"])
def test_gather_corrects_for_pending_columns(gpu_required, monkeypatch, dtype, defer, pending):
    """PHT of an update under 1, 16 (inside the gather), 17 (the <T, 64, 2> form), 64 (one batch panel) and 65 (Y = H Wp
    and the correction kernel) pending columns, against P_eff H^T in f64, where P_eff is what a twin handle driven
    through the same calls returns from get_state (which applies the pending columns)."""
    from conan_slam_amd import EKF

    monkeypatch.setenv("CSLAM_LOOKAHEAD", "0")
    N = 200
    X, P = scenario(N, dtype, seed=31)
    R = R22.astype(dtype)
    engs = []
    for _ in range(2):
        e = EKF(N, dtype=dtype, quirks=TEXTBOOK, sync_mode=False)
        e.set_state(X, P)
        e.set_deferred(defer)
        engs.append(e)
    heads = {"h1": 1, "h16": 16, "h17": 17, "k64": 0, "k64+h1": 1}[pending]
    idf0 = pick_landmarks(N, 32, seed=5)
    Z0 = make_obs(X, idf0, dtype, seed=3)
    for e in engs:
        if pending.startswith("k64"):
            e.update(Z0, R, idf0, True)
        for step in range(heads):
            _heading(e, step)
    Xe, Pe = engs[1].get_state()
    idf = pick_landmarks(N, 24, seed=6)
    Z = make_obs(Xe, idf, dtype, seed=4)
    engs[0].update(Z, R, idf, True)
    d = engs[0].debug_last_update()
    assert engs[0].factor_status() == 0
    _, H, _ = innovation_and_jacobian(Xe, idf, Z)
    kp = heads + (64 if pending.startswith("k64") else 0)
    u = _u(dtype)
    P0 = np.abs(P.astype(np.float64))
    sd = np.sqrt(np.diag(P0))
    bound = 16 * u * (P0 @ np.abs(H).T) + 4 * (kp + 4) * u * (np.outer(sd, sd) @ np.abs(H).T)
    check_bound(f"PHT under {pending}", d["PHT"], Pe.astype(np.float64) @ H.T, bound, REL[np.dtype(dtype)])
    for e in engs:
        e.close()


# ------------------------------------------------------------------------------------------------ C: P-GEMM variants
def _pgemm_case(monkeypatch, dtype, k, N, env):
    from conan_slam_amd import EKF

    for key, val in env.items():
        monkeypatch.setenv(key, val)
    X, P = scenario(N, dtype, seed=500 + k + N)
    idf = pick_landmarks(N, k // 2, seed=k * N)
    Z = make_obs(X, idf, dtype, seed=k)
    e = EKF(N, dtype=dtype, quirks=TEXTBOOK)
    e.set_state(X, P)
    e.update(Z, R22.astype(dtype), idf, batch=True)
    W1 = e.debug_last_update()["W1"].astype(np.float64)[3:, :]
    _, Pg = e.get_state()
    assert e.factor_status() == 0
    e.close()
    M = Pg.copy()
    M[:3, :3] = 0
    assert np.array_equal(M, M.T), "P must be exactly symmetric outside the pose block"
    P0 = P[3:, 3:].astype(np.float64)
    expected = P0 - W1 @ W1.T
    u = _u(dtype)
    # the subtraction rounds at the size of its operands; the dot product of length k at (k + 1) u of sum |w_ik w_jk|
    bound = u * (np.abs(P0) + np.abs(expected)) + (k + 1) * u * (np.abs(W1) @ np.abs(W1).T) + 1e-300
    check_bound(f"P-GEMM k={k} N={N}", Pg[3:, 3:], expected, bound, REL[np.dtype(dtype)])


PGEMM_NS = [62, 63, 127, 600]  # n = 127, 129, 257 and a multi-tile 1203


def _c_cases():
    out = []
    for k in (2, 34, 62, 66, 94, 98, 128):
        for N in PGEMM_NS:
            if k // 2 <= N:
                out.append(pytest.param(np.float32, k, N, {}, id=f"psym4-k{k}-N{N}"))
    for N in PGEMM_NS:
        if 65 <= N:
            for storage in ("lower", "full"):
                out.append(pytest.param(np.float32, 130, N, {"CSLAM_STORAGE": storage}, id=f"psym_f32-{storage}-N{N}"))
    for k in (2, 18, 66):
        for N in PGEMM_NS:
            if k // 2 <= N:
                for cb in ("2", "4"):
                    out.append(pytest.param(np.float64, k, N, {"CSLAM_F64_CB": cb}, id=f"f64-cb{cb}-k{k}-N{N}"))
    return out


@pytest.mark.parametrize("dtype,k,N,env", _c_cases())
def test_pgemm_variants_against_an_f64_product_of_the_same_panel(gpu_required, monkeypatch, dtype, k, N, env):
    """One immediate update: P_map -= W1 W1^T checked element by element against f64 from the same panel."""
    _pgemm_case(monkeypatch, dtype, k, N, env)


# ------------------------------------------------------------------------------------------------ D: re-observed landmarks
def _reobserve(prev, N, m, pattern, rng):
    """landmarks of the second update of a window from those of the first one"""
    if pattern == "same":
        base = list(prev)
    elif pattern == "permuted":
        base = list(prev[rng.permutation(len(prev))])
    elif pattern == "half":
        base = list(prev[: len(prev) // 2])
    else:  # "none"
        base = []
    base = base[:m]
    pool = [f for f in rng.permutation(N) + 1 if f not in set(base) and (pattern != "none" or f not in set(prev))]
    out = np.array(base + pool[: m - len(base)], dtype=np.int32)
    return out


def _window_run(monkeypatch, dtype, N, lookahead, quirks=TEXTBOOK):
    from conan_slam_amd import EKF

    monkeypatch.setenv("CSLAM_LOOKAHEAD", lookahead)
    X0, P0 = scenario(N, dtype, seed=77 + N)
    eng = EKF(N, dtype=dtype, quirks=quirks, sync_mode=False)
    eng.set_state(X0, P0)
    eng.set_deferred(128)
    monkeypatch.delenv("CSLAM_LOOKAHEAD")
    return eng, X0, P0


def _window_plan(N, seed):
    """(m, idf) of each update: pairs (a, b) where b re-observes a's landmarks in every pattern, at m = 9 and 32."""
    rng = np.random.default_rng(seed)
    plan = []
    for pattern in ("same", "permuted", "half", "none"):
        for ma, mb in ((32, 32), (9, 32), (32, 9), (9, 9)):
            if max(ma, mb) > N:
                continue
            a = pick_landmarks(N, ma, seed=int(rng.integers(1 << 30)))
            b = _reobserve(a, N, mb, pattern, rng)
            plan += [a, b]
    return plan


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [62, 63, 700])
def test_lookahead_windows_with_reobserved_landmarks(gpu_required, monkeypatch, dtype, N):
    """Windows whose second update sees the first one's landmarks again (same order, another order, half, none;
    m_a != m_b at m = 9 / 32; tile-straddling and last landmarks included): against the oracle and f64, and against the
    same sequence without windows."""
    plan = _window_plan(N, seed=N)
    R = R22.astype(dtype)
    Q = np.diag([0.18, 6e-4]).astype(dtype)
    X0, P0 = scenario(N, dtype, seed=77 + N)
    orc = OracleState(X0, P0, dtype, TEXTBOOK)
    hi = OracleState(X0.astype(np.float64), P0.astype(np.float64), np.float64, TEXTBOOK)
    obs = []
    for t, idf in enumerate(plan):
        for s in (orc, hi):
            s.predict(83.33, 0.01 * (t % 5), Q.astype(s.X.dtype), 73.0, 0.01)
        Z = make_obs(orc.x(), idf, dtype, seed=t)
        obs.append(Z)
        assert orc.update(Z, R, idf, True) == 0
        hi.update(Z.astype(np.float64), R.astype(np.float64), idf, True)
    results = {}
    for la in ("1", "0"):
        eng, _, _ = _window_run(monkeypatch, dtype, N, la)
        for t, idf in enumerate(plan):
            eng.predict(83.33, 0.01 * (t % 5), Q, 73.0, 0.01)
            eng.update(obs[t], R, idf, True)
        results[la] = eng.get_state()
        assert eng.factor_status() == 0
        # every pair formed one window (none with look-ahead off)
        assert eng.lookahead_windows() == (len(plan) // 2 if la == "1" else 0)
        eng.close()
    dt = np.dtype(dtype)
    X1, P1 = results["1"]
    assert_close("lookahead X", X1, orc.x(), 4 * X_RTOL[dt], hi.x(), fair=8.0)
    assert_close("lookahead P", P1, orc.p(), 4 * P_RTOL[dt], hi.p(), fair=8.0)
    X0_, P0_ = results["0"]
    assert_close("windows vs none X", X1, X0_, 2e-5 if dt == np.float32 else 1e-11)
    assert_close("windows vs none P", P1, P0_, 2e-4 if dt == np.float32 else 1e-9)


def test_timed_path_sequence_with_reobserved_landmarks(gpu_required, monkeypatch):
    """N = 5000 f32 on the timed path's calls (update_device, held predicts, 8 steps): every second update re-observes
    the previous one's landmarks.  Windows on (four pairs, counted) against the oracle and against windows off."""
    import torch

    from conan_slam_amd import EKF
    from conan_slam_amd.synth import Workload

    N, m = 5000, 32
    w = Workload(N, m, np.float32)
    rng = np.random.default_rng(3)
    steps = []
    prev = None
    for t in range(8):
        v, swa = w.controls(t)
        Z, idf = w.observations(t)
        if t % 2 == 1:
            idf = prev[rng.permutation(m)].astype(np.int32)
            X = w.X0  # (observations of re-observed landmarks from the workload's initial state: any Z will do)
            Z = make_obs(X, idf, np.float32, seed=t)
        prev = idf
        steps.append((v, swa, np.ascontiguousarray(Z.reshape(-1, order="F")), np.ascontiguousarray(idf)))
    dZ = torch.from_numpy(np.stack([s[2] for s in steps])).cuda()
    dI = torch.from_numpy(np.stack([s[3] for s in steps])).cuda()
    torch.cuda.synchronize()
    out = {}
    for la in ("1", "0"):
        monkeypatch.setenv("CSLAM_LOOKAHEAD", la)
        e = EKF(N, dtype=np.float32, quirks=TEXTBOOK, sync_mode=False)
        e.set_state(w.X0, w.P0)
        e.set_deferred(128)
        for t, (v, swa, _, _) in enumerate(steps):
            e.predict(v, swa, w.QE, w.wb, w.dt)
            e.update_device(dZ.data_ptr() + t * 2 * m * 4, m, w.RE, dI.data_ptr() + t * m * 4, batch=True)
        out[la] = e.get_state()
        assert e.factor_status() == 0
        assert e.lookahead_windows() == (len(steps) // 2 if la == "1" else 0)
        e.close()
    assert_close("X", out["1"][0], out["0"][0], 2e-5)
    assert_close("P", out["1"][1], out["0"][1], 2e-4)
    o = Oracle(np.float32, TEXTBOOK)  # (the oracle's dense-order fast path, as test_full_size_5000_landmarks_one_update)
    X, P = w.X0.copy(), w.P0.copy(order="F")
    for v, swa, z, idf in steps:
        o.predict(X, P, w.n, v, swa, w.QE, w.wb, w.dt)
        assert o.update(X, P, w.n, z.reshape(2, -1, order="F"), w.RE, idf, True, fast=True) == 0
    assert_close("lookahead X vs oracle", out["1"][0], X, 4 * X_RTOL[np.dtype(np.float32)])
    assert_close("lookahead P vs oracle", out["1"][1], P, 4 * P_RTOL[np.dtype(np.float32)])


def _batch_cases():
    out = []
    for path in ("run", "update_device"):
        for m in (8, 9, 32):
            if path == "run" and m < 9:
                continue  # (cslam_ekf_batch_run takes 9..32 observations)
            for N in (63, 200):
                out.append(pytest.param(path, m, N, id=f"{path}-m{m}-N{N}"))
    return out


@pytest.mark.parametrize("path,m,N", _batch_cases())
def test_batched_windows_with_reobserved_landmarks(gpu_required, path, m, N):
    """The batched engine on the same patterns: instance i's odd steps re-observe its previous step's landmarks (all of
    them in the same order, in another order, half of them), tile-straddling and last landmarks included, at m = 8
    (the k <= 16 chain, update_device only), 9 and 32, and at n = 129 (one row past a tile edge).  run() pairs the
    updates into windows (the carry step applies update a to the rows update b observes); update_device launches a
    window per update.  Every instance against its own oracle and f64."""
    import torch

    from conan_slam_amd import EKFBatch

    patterns = ("same", "permuted", "half")
    I, steps, dtype = len(patterns), 6, np.float32
    Q = np.diag([0.18, 6e-4]).astype(dtype)
    R = R22.astype(dtype)
    wb, dt = 73.0, 0.01
    ctrl = [(83.33, 0.02 * ((t % 3) - 1)) for t in range(steps)]
    states = [scenario(N, dtype, seed=600 + 10 * i + N) for i in range(I)]
    plans, obs = [], []
    for i, pattern in enumerate(patterns):
        rng = np.random.default_rng(900 + i + N + m)
        plan, prev = [], None
        for t in range(steps):
            idf = (_reobserve(prev, N, m, pattern, rng) if t % 2 == 1
                   else pick_landmarks(N, m, seed=int(rng.integers(1 << 30))))
            plan.append(idf)
            prev = idf
        plans.append(plan)
        obs.append([make_obs(states[i][0], idf, dtype, seed=31 * t + i) for t, idf in enumerate(plan)])
    dZ = [torch.from_numpy(np.stack([z.reshape(-1, order="F") for z in obs[i]])).cuda() for i in range(I)]
    dI = [torch.from_numpy(np.stack(plans[i]).astype(np.int32)).cuda() for i in range(I)]
    torch.cuda.synchronize()
    b = EKFBatch(I, N, quirks=TEXTBOOK)
    for i, (X0, P0) in enumerate(states):
        b.set_state(i, X0, P0)
    if path == "run":
        b.run(steps, [c[0] for c in ctrl], [c[1] for c in ctrl], Q, wb, dt, [z.data_ptr() for z in dZ],
              [d.data_ptr() for d in dI], m, R)
        expected_windows = (steps + 1) // 2
    else:
        for t, (v, swa) in enumerate(ctrl):
            b.predict(v, swa, Q, wb, dt)
            b.update_device([z.data_ptr() + t * 2 * m * 4 for z in dZ], [d.data_ptr() + t * m * 4 for d in dI], m, R)
        expected_windows = steps
    got = [b.get_state(i) for i in range(I)]
    assert b.factor_status() == [0] * I
    assert b.windows() == expected_windows
    b.close()
    for i, (X0, P0) in enumerate(states):
        orc = OracleState(X0, P0, dtype, TEXTBOOK)
        hi = OracleState(X0.astype(np.float64), P0.astype(np.float64), np.float64, TEXTBOOK)
        for t, (v, swa) in enumerate(ctrl):
            orc.predict(v, swa, Q, wb, dt)
            hi.predict(v, swa, Q.astype(np.float64), wb, dt)
            assert orc.update(obs[i][t], R, plans[i][t], True) == 0
            hi.update(obs[i][t].astype(np.float64), R.astype(np.float64), plans[i][t], True)
        assert_close(f"batch X[{i}]", got[i][0], orc.x(), 4 * X_RTOL[np.dtype(dtype)], hi.x(), fair=8.0)
        assert_close(f"batch P[{i}]", got[i][1], orc.p(), 4 * P_RTOL[np.dtype(dtype)], hi.p(), fair=8.0)


# ------------------------------------------------------------------------------------------------ E: reused device inputs
def _reuse_plan(N):
    rng = np.random.default_rng(N)
    ms = [32, 24, 32, 20, 9, 32, 16, 32]
    plan, prev = [], None
    for i, m in enumerate(ms):
        if prev is not None and i % 2 == 1:
            idf = _reobserve(prev, N, m, "permuted", rng)
        else:
            idf = pick_landmarks(N, m, seed=int(rng.integers(1 << 30)))
        plan.append(idf)
        prev = idf
    return plan


def _run_one_engine(N, X0, P0, lookahead, monkeypatch, drive):
    """One handle, alone in the process (the single-engine schedule: the chain kernel is launched ahead of the window's
    rows / blocks kernels and waits for them on a counter), driven by `drive(eng)`; returns what drive returns, the
    final state and the number of look-ahead windows launched."""
    from conan_slam_amd import EKF

    monkeypatch.setenv("CSLAM_LOOKAHEAD", lookahead)
    e = EKF(N, dtype=np.float32, quirks=TEXTBOOK, sync_mode=False)
    monkeypatch.delenv("CSLAM_LOOKAHEAD")
    e.set_state(X0, P0)
    e.set_deferred(128)
    got = drive(e)
    X, P = e.get_state()
    assert e.factor_status() == 0
    wins = e.lookahead_windows()
    e.close()
    return got, X, P, wins


@pytest.mark.parametrize("lookahead", ["1", "0"])
@pytest.mark.parametrize("ending", ["flush", "get_x"])
@pytest.mark.parametrize("wait", ["handle", "device"])
def test_reused_device_buffers_match_host_updates(gpu_required, monkeypatch, lookahead, ending, wait):
    """One device buffer for Z and one for idf, rewritten before every update_device call, after the caller has waited
    for everything the update enqueued: bitwise the same filter as the host-pointer update() of the same sequence (whose
    inputs are staged).  The two sequences run one after the other, each handle alone in the process.
    wait = "device": a device-wide synchronisation only.  The first update of each window stays queued across it, so
    with look-ahead on the windows pair up (checked), and the queued update must not read the caller's buffer when
    its window launches during the next call.  wait = "handle": cslam_ekf_synchronize, which launches a queued update
    on its own -- with look-ahead on every update is then a window of one (checked), never a pair."""
    import torch

    N, dtype = 420, np.float32
    X0, P0 = scenario(N, dtype, seed=4)
    R = R22.astype(dtype)
    Q = np.diag([0.18, 6e-4]).astype(dtype)
    plan = _reuse_plan(N)
    obs = [make_obs(X0, idf, dtype, seed=100 + t) for t, idf in enumerate(plan)]
    dZ = torch.zeros(64, dtype=torch.float32, device="cuda")
    dI = torch.zeros(32, dtype=torch.int32, device="cuda")

    def drive(on_device):
        def run(e):
            for t, idf in enumerate(plan):
                m = len(idf)
                e.predict(83.33, 0.01 * t, Q, 73.0, 0.01)
                if on_device:
                    dZ[: 2 * m].copy_(torch.from_numpy(np.ascontiguousarray(obs[t].reshape(-1, order="F"))))
                    dI[:m].copy_(torch.from_numpy(idf))
                    torch.cuda.synchronize()
                    e.update_device(dZ.data_ptr(), m, R, dI.data_ptr(), batch=True)
                else:
                    e.update(obs[t], R, idf, True)
                if wait == "handle":
                    e.synchronize()
                else:
                    torch.cuda.synchronize()
            if ending == "flush":
                e.flush()
                e.synchronize()
                return None
            return e.get_x()
        return run

    xh, Xh, Ph, wh = _run_one_engine(N, X0, P0, lookahead, monkeypatch, drive(False))
    xd, Xd, Pd, wd = _run_one_engine(N, X0, P0, lookahead, monkeypatch, drive(True))
    expected = 0 if lookahead == "0" else (len(plan) if wait == "handle" else len(plan) // 2)
    assert wh == wd == expected, (wh, wd, expected)
    if ending == "get_x":
        assert np.array_equal(xh, xd), "X differs"
    assert np.array_equal(Xh, Xd) and np.array_equal(Ph, Pd), (
        f"max |dX| {float(np.abs(Xh - Xd).max()):.3e}, max |dP| {float(np.abs(Ph - Pd).max()):.3e}")


def test_simulator_buffers_feed_update_device_across_steps(gpu_required, monkeypatch):
    """Simulator.device_ptrs() (the simulator's fixed ZF / idf buffers, rewritten by every scan) feeding update_device
    over several steps with look-ahead windows forced on, a device-wide synchronisation after each update (windows stay
    open across it): bitwise the host path run over the same scans, each handle alone in the process."""
    import torch

    from conan_slam_amd import Simulator

    N, dtype = 300, np.float32
    X0, P0 = scenario(N, dtype, seed=21)
    LM = np.asfortranarray(X0[3:].reshape(2, N, order="F").astype(dtype))
    sim = Simulator(LM)
    sim.table = np.arange(1, N + 1, dtype=np.int32)  # every landmark already known: a scan's ZF is the whole scan
    R = R22.astype(dtype)
    Q = np.diag([0.18, 6e-4]).astype(dtype)
    rng = np.random.default_rng(8)
    poses = []
    for trial in range(400):  # scans with 9..32 observations: the sizes a window takes
        xv = np.array([rng.uniform(-400, 400), rng.uniform(-400, 400), rng.uniform(-3.1, 3.1)], dtype=dtype)
        if 9 <= len(sim.get_observations(xv, 110.0)[1]) <= 32:
            poses.append(xv)
            if len(poses) == 8:
                break
    assert len(poses) == 8

    def drive(on_device):
        def run(e):
            for t, xv in enumerate(poses):
                Z, tags = sim.get_observations(xv, 110.0)
                ZF, ZN, idf = sim.data_associate_table(N)
                assert ZN.shape[1] == 0 and len(idf) == len(tags)
                e.predict(83.33, 0.01 * t, Q, 73.0, 0.01)
                if on_device:
                    p = sim.device_ptrs()
                    e.update_device(p["ZF"], len(idf), R, p["idf"], batch=True)
                else:
                    e.update(ZF, R, idf, True)
                torch.cuda.synchronize()
        return run

    _, Xh, Ph, wh = _run_one_engine(N, X0, P0, "1", monkeypatch, drive(False))
    _, Xd, Pd, wd = _run_one_engine(N, X0, P0, "1", monkeypatch, drive(True))
    sim.close()
    assert wh == wd == len(poses) // 2
    assert np.array_equal(Xh, Xd) and np.array_equal(Ph, Pd), (
        f"max |dX| {float(np.abs(Xh - Xd).max()):.3e}, max |dP| {float(np.abs(Ph - Pd).max()):.3e}")


# ------------------------------------------------------------------------------------------------ I * FLT_MIN
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_heading_adds_flt_min_to_the_pose_block_only(gpu_required, dtype):
    """slam.h:719 adds I * FLT_MIN to the whole diagonal; the engine adds it to the pose block only.  With
    a zero pose block the heading step changes nothing else, so a map diagonal entry of 0 and one of 2^-103 (below
    2^-102, where adding FLT_MIN still changes an f32) stay as they are on the engine and move on the oracle."""
    from conan_slam_amd import EKF

    N = 3
    X = np.array([0.0, 0.0, 0.0, 10.0, 5.0, -7.0, 3.0, 20.0, 1.0], dtype=dtype)
    P = np.zeros((9, 9), dtype=dtype, order="F")
    small = dtype(2.0 ** -103)
    diag = [0.0, 0.0, 0.0, 0.0, small, 1.0, 0.5, 2.0, 0.25]
    P[np.diag_indices(9)] = np.array(diag, dtype=dtype)
    eng = EKF(N, dtype=dtype, quirks=REF_EXACT)
    eng.set_state(X, P)
    eng.observe_heading(0.2, True)
    Xg, Pg = eng.get_state()
    Xo, Po = X.copy(), P.copy(order="F")
    Oracle(dtype, REF_EXACT).observe_heading(Xo, Po, 9, 0.2, True)
    tiny = dtype(np.finfo(np.float32).tiny)
    expected = P.copy()
    expected[np.diag_indices(3)] = tiny
    assert np.array_equal(Pg, expected), np.diag(Pg)
    assert np.array_equal(Xg, X)
    assert Pg[3, 3] == 0 and Pg[4, 4] == small
    # the oracle adds FLT_MIN to every diagonal entry: both small map entries change, the others absorb it
    assert Po[3, 3] == tiny and Po[4, 4] == small + tiny and Po[4, 4] != small
    assert np.array_equal(np.diag(Po)[5:], np.diag(P)[5:])
    eng.close()
