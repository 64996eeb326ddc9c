"""The landmark reads (cslam_ekf_get_landmarks / cslam_ekf_batch_get_landmarks, EKF.landmarks / EKFBatch.landmarks):
means, 2 x 2 marginal blocks and pose-landmark blocks read from P = Ps - Wp Wp^T without applying the pending columns.

Every read is compared with a TWIN handle driven by the same calls and then read with get_state (which flushes: the
engine is flushed after each comparison too, so the two stay in lockstep across checkpoints), and
with the oracle of the same calls (f32 / f64 at the handle's dtype, the f64 oracle as fairness reference):
  - X and the pose-landmark block are exact on both paths (the pose stripe is always current): bitwise;
  - the 2 x 2 block is bitwise where nothing is pending (after a flush; rows appended by the last augment), and
    elsewhere within  2 (KP + 2) u (|P_ab| + sqrt(D_a D_b))  of the twin, D_a >= sum_c w_ac^2 the pending columns'
    share of P_aa (from the f64 oracle's history: landmark variances only decrease, so D_a <= max_t P_aa(t) - P_aa);
  - a host-side negative control shows the bound rejects a 1e-4 (f32) / 1e-9 (f64) relative error.
Reading never perturbs the run (bitwise against the same run without reads) and never launches a P-GEMM.
"""
import numpy as np
import pytest

from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs, make_scenario
from pyoracle import REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu

Q = np.diag([0.18, 6e-4])
R = np.diag([0.08, 0.0024])
WB, DT = 73.0, 0.01
KP_BOUND = 256  # more pending columns than any scenario here holds (batch regions: 128; deferred(128) + one update)
REL = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-9}


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _blocks(X, P, first, count):
    """The twin's blocks from a full state: x [c,2], P_ll [c,2,2] (off-diagonals from P[fx+1, fx]), P_vl [c,3,2]."""
    fx = 3 + 2 * (np.arange(first, first + count) - 1)
    x = np.stack([X[fx], X[fx + 1]], axis=1)
    ll = np.empty((count, 2, 2), dtype=P.dtype)
    ll[:, 0, 0] = P[fx, fx]
    ll[:, 1, 0] = ll[:, 0, 1] = P[fx + 1, fx]
    ll[:, 1, 1] = P[fx + 1, fx + 1]
    vl = np.stack([P[:3, fx].T, P[:3, fx + 1].T], axis=2)
    return x, ll, vl


def _bound(dtype, Ptw_ll, D, extra=None):
    """Elementwise bound on |read - twin| of the 2 x 2 blocks."""
    u = float(np.finfo(dtype).eps) / 2
    Dc = np.sqrt(np.maximum(D, 0.0))  # [c, 2]
    A = Dc[:, :, None] * Dc[:, None, :]
    if extra is not None:
        A = A + extra
    return 2 * (KP_BOUND + 2) * u * (np.abs(Ptw_ll.astype(np.float64)) + A)


def _within(got, ref, bound):
    return bool(np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= bound))


def _check(tag, dtype, read, twin, orc, hi, Hmax, exact=None, extra=None):
    """read / twin: (x, ll, vl); orc / hi: the oracle's blocks; Hmax [c, 2]: history max of the landmark variances
    (f64 oracle); exact: mask [c] of landmarks whose 2 x 2 block must be bitwise."""
    dt = np.dtype(dtype)
    x, ll, vl = read
    tx, tll, tvl = twin
    assert x.dtype == dt and ll.dtype == dt and vl.dtype == dt
    assert np.array_equal(x, tx), f"{tag}: x differs from the twin"
    assert np.array_equal(vl, tvl), f"{tag}: P_vl differs from the twin"
    assert np.array_equal(ll[:, 0, 1], ll[:, 1, 0]), f"{tag}: P_ll not exactly symmetric"
    P_now = np.stack([tll[:, 0, 0], tll[:, 1, 1]], axis=1).astype(np.float64)
    D = Hmax * (1 + 1e-3) - P_now
    b = _bound(dt, tll, D, extra)
    assert _within(ll, tll, b), f"{tag}: P_ll off the twin: max |d| {np.abs(ll.astype(float) - tll).max():.3e}"
    # negative control: the same bound rejects a relative error of REL
    assert not _within(ll * (1 + REL[dt]), tll, b), f"{tag}: the bound is too loose to reject {REL[dt]}"
    if exact is not None and np.any(exact):
        assert np.array_equal(ll[exact], tll[exact]), f"{tag}: P_ll of landmarks with nothing pending not bitwise"
    ox, oll, ovl = orc
    hx, hll, hvl = hi
    assert_close(f"{tag} x", x, ox, 4 * X_RTOL[dt], hx, fair=8.0)
    assert_close(f"{tag} P_ll", ll, oll, 4 * P_RTOL[dt], hll, fair=8.0)
    assert_close(f"{tag} P_vl", vl, ovl, 4 * P_RTOL[dt], hvl, fair=8.0)


# ------------------------------------------------------------------------------------------------ single filter


class Single:
    """An engine `a` (read with landmarks()), its twin `t` (read with get_state), the f32/f64 oracles of the same calls."""

    def __init__(self, monkeypatch, N, dtype, quirks=TEXTBOOK, env=None, deferred=0, sync=True, extra=0, seed=0,
                 state=None):
        from conan_slam_amd import EKF

        self.dtype = np.dtype(dtype)
        X, P = state if state is not None else make_scenario(N, self.dtype, seed=seed, corr=0.1)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        self.a = EKF(N + extra, dtype=dtype, quirks=quirks, sync_mode=sync)
        self.t = EKF(N + extra, dtype=dtype, quirks=quirks, sync_mode=sync)
        for k in (env or {}):
            monkeypatch.delenv(k)
        for e in (self.a, self.t):
            e.set_state(X, P)
            if deferred:
                e.set_deferred(deferred)
        self.orc = OracleState(X, P, self.dtype, quirks, extra)
        self.hi = OracleState(X.astype(np.float64), P.astype(np.float64), np.float64, quirks, extra)
        self.H = np.diagonal(self.hi.P)[: self.hi.n].copy()
        self.new_from = None  # first landmark appended by the last augment

    def _hist(self):
        d = np.diagonal(self.hi.P)[: self.hi.n].copy()
        H = np.zeros_like(d)
        H[: self.H.shape[0]] = self.H
        self.H = np.maximum(H, d)

    def predict(self, v, swa):
        for e in (self.a, self.t):
            e.predict(v, swa, Q.astype(self.dtype), WB, DT)
        for s in (self.orc, self.hi):
            s.predict(v, swa, Q.astype(s.X.dtype), WB, DT)
        self.new_from = None

    def heading(self, phi):
        for e in (self.a, self.t):
            e.observe_heading(phi, True)
        for s in (self.orc, self.hi):
            s.observe_heading(phi, True)
        self._hist()
        self.new_from = None

    def update(self, idf, seed, batch=True):
        idf = np.asarray(idf, dtype=np.int32)
        Z = make_obs(self.orc.x(), idf, self.dtype, seed=seed)
        for e in (self.a, self.t):
            e.update(Z, R.astype(self.dtype), idf, batch)
        self.orc.update(Z, R.astype(self.dtype), idf, batch)
        self.hi.update(Z.astype(np.float64), R, idf, batch)
        self._hist()
        self.new_from = None

    def augment(self, Zn):
        Zn = np.asfortranarray(Zn, dtype=self.dtype)
        nf = (self.orc.n - 3) // 2
        for e in (self.a, self.t):
            e.augment(Zn, R.astype(self.dtype))
        self.orc.augment(Zn, R.astype(self.dtype))
        self.hi.augment(Zn.astype(np.float64), R)
        self._hist()
        self.new_from = nf + 1

    def check(self, tag, first=1, count=None, extra=None, exact_all=False):
        nf = (self.orc.n - 3) // 2
        count = nf - first + 1 if count is None else count
        read = self.a.landmarks(first, count)
        X, P = self.t.get_state()
        twin = _blocks(X, P, first, count)
        orc = _blocks(self.orc.X, self.orc.P, first, count)  # (the padded oracle arrays: no copy of P)
        hi = _blocks(self.hi.X, self.hi.P, first, count)
        fx = 3 + 2 * (np.arange(first, first + count) - 1)
        Hmax = np.stack([self.H[fx], self.H[fx + 1]], axis=1)
        f = np.arange(first, first + count)
        exact = np.ones(count, bool) if exact_all else (f >= self.new_from if self.new_from else None)
        _check(tag, self.dtype, read, twin, orc, hi, Hmax, exact=exact, extra=extra)
        self.a.flush()  # (the twin's get_state has applied its pending columns: keep the two handles in lockstep)
        return read

    def close(self):
        self.a.close()
        self.t.close()


def _ids(N, m, rng, must=()):
    ids = list(must) + [int(f) for f in rng.permutation(N) + 1 if int(f) not in must]
    return np.array(ids[:m], dtype=np.int32)


DTYPES = [np.float32, np.float64]
STORAGE = ["lower", "full"]


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [62, 63])
def test_single_immediate_mode(gpu_required, monkeypatch, dtype, storage, N):
    """Immediate mode: each update's P-GEMM is applied at once -- nothing pending after an update, so the read is
    bitwise the twin's; the heading steps that follow leave rank-1 columns pending.  N = 62 / 63: n = 127 / 129."""
    s = Single(monkeypatch, N, dtype, env={"CSLAM_STORAGE": storage})
    rng = np.random.default_rng(N)
    s.predict(83.33, 0.02)
    s.update(_ids(N, 20, rng, must=(1, N)), seed=1)
    s.check("immediate, after update", exact_all=True)
    for t in range(3):
        s.predict(83.33, 0.01 * t)
        s.heading(float(s.hi.x()[2]) + 1e-3)
    s.check("immediate, heading columns pending")
    s.close()


@pytest.mark.parametrize("storage", STORAGE)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N", [62, 63])
def test_single_deferred_windows(gpu_required, monkeypatch, dtype, storage, N):
    """Deferred mode (set_deferred(128), look-ahead off): panels of several updates and heading columns pending; a
    sequential update; every f = 63 mod 64 landmark (fx = 127 mod 128, straddling two row tiles), the first and the
    last observed.  Then a flush: bitwise."""
    s = Single(monkeypatch, N, dtype, env={"CSLAM_STORAGE": storage, "CSLAM_LOOKAHEAD": "0"}, deferred=128, sync=False)
    rng = np.random.default_rng(100 + N)
    must = tuple(sorted({1, N} | {f for f in range(63, N + 1, 64)}))
    s.predict(83.33, 0.02)
    s.update(_ids(N, 12, rng, must=must), seed=2)
    s.check("deferred, one panel")
    s.predict(83.33, -0.01)
    s.heading(float(s.hi.x()[2]) - 1e-3)
    s.update(_ids(N, 9, rng, must=must), seed=3)
    s.check("deferred, two panels and a heading column")
    s.update(_ids(N, 4, rng, must=must), seed=4, batch=False)  # sequential
    s.check("deferred, after a sequential update")
    for e in (s.a, s.t):
        e.flush()
    s.check("deferred, flushed", exact_all=True)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_single_negative_heading_column(gpu_required, monkeypatch, dtype):
    """set_state with P22 + R < 0: the heading column is stored with S < 0 (sign word set) and enters P with the
    opposite sign; the read must apply it as P + w w^T."""
    N = 40
    X, P = make_scenario(N, np.dtype(dtype), seed=9, corr=0.1)
    P = P.astype(np.float64)
    P[2, 2] = -0.5
    P = np.asfortranarray(P.astype(dtype))
    s = Single(monkeypatch, N, dtype, state=(X, P), env={"CSLAM_LOOKAHEAD": "0"}, deferred=128, sync=False)
    s.heading(float(X[2]) + 1e-3)
    sig2 = (0.01 * np.pi / 180.0) ** 2
    Sabs = abs(float(P[2, 2]) + sig2)
    fx = 3 + 2 * np.arange(N)
    p = np.abs(np.stack([P[2, fx], P[2, fx + 1]], axis=1).astype(np.float64))
    extra = p[:, :, None] * p[:, None, :] / Sabs
    s.H = np.maximum(s.H, np.abs(np.diag(P.astype(np.float64))) + np.concatenate([[0, 0, 0], (p ** 2).reshape(-1) / Sabs]))
    read = s.check("negative heading column", extra=extra)
    # the column really is there: the read differs from the stored Ps by the positive rank-1 term
    assert np.all(read[1][:, 0, 0] >= P[fx, fx] - 1e-3 * np.abs(P[fx, fx]))
    s.close()


def test_single_lookahead_queued_update(gpu_required, monkeypatch):
    """Look-ahead windows forced (CSLAM_LOOKAHEAD=1): after an odd number of updates one is still queued; the read
    launches it alone as a window of one, as get_x does, and the twin's get_state does the same."""
    N = 300
    s = Single(monkeypatch, N, np.float32, env={"CSLAM_LOOKAHEAD": "1"}, deferred=128, sync=False)
    rng = np.random.default_rng(5)
    for t in range(3):
        s.predict(83.33, 0.01 * t)
        s.update(_ids(N, 16, rng, must=(1, 63, N)), seed=10 + t)
    s.check("look-ahead, update queued")
    assert s.a.lookahead_windows() == s.t.lookahead_windows() == 2
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_single_n5000(gpu_required, monkeypatch, dtype):
    """N = 5000 on the default engine, deferred: a pending m = 32 panel, the whole map read."""
    N = 5000
    s = Single(monkeypatch, N, dtype, deferred=128, sync=False)
    rng = np.random.default_rng(7)
    s.predict(83.33, 0.02)
    s.update(_ids(N, 32, rng, must=(1, 63, 127, 4991, N)), seed=1)
    s.predict(83.33, 0.01)
    s.update(_ids(N, 32, rng, must=(1, 63, 127, N)), seed=2)
    s.check("N=5000")
    s.close()


def test_single_edges_and_bad_arguments(gpu_required, monkeypatch):
    import ctypes as C

    from conan_slam_amd._capi import ERR_BAD_ARG

    N = 70
    s = Single(monkeypatch, N, np.float32, env={"CSLAM_LOOKAHEAD": "0"}, deferred=64, sync=False)
    rng = np.random.default_rng(11)
    s.predict(83.33, 0.02)
    s.update(_ids(N, 10, rng, must=(1, 63, N)), seed=1)
    full = s.a.landmarks()
    for first, count in ((1, 1), (N, 1), (63, 2), (62, 9), (1, N)):
        part = s.a.landmarks(first, count)
        for a, b in zip(part, full):
            assert np.array_equal(a, b[first - 1: first - 1 + count]), (first, count)
    L, h = s.a._L, s.a._h
    buf = np.zeros(12 * (N + 2), np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.cslam_ekf_get_landmarks(h, 1, 0, p, p, p) == 0
    assert L.cslam_ekf_get_landmarks(h, N + 1, 0, p, None, None) == 0
    for first, count in ((0, 1), (-1, 2), (1, N + 1), (N, 2), (N + 1, 1), (2, -1), (N + 2, 0)):
        assert L.cslam_ekf_get_landmarks(h, first, count, p, p, p) == ERR_BAD_ARG, (first, count)
    assert L.cslam_ekf_get_landmarks(h, 1, 1, None, None, None) == ERR_BAD_ARG
    assert not np.any(buf)
    for i, part in enumerate(("x", "ll", "vl")):  # each output alone
        args = [None, None, None]
        out = np.zeros(6 * N, np.float32)
        args[i] = out.ctypes.data_as(C.c_void_p)
        assert L.cslam_ekf_get_landmarks(h, 1, N, *args) == 0
        assert np.array_equal(out[: full[i].size], np.ascontiguousarray(full[i].transpose(0, 2, 1) if i else full[i]).reshape(-1)), part
    s.check("after the edge reads")  # (state unchanged by the refused calls)
    s.close()


def _single_script(e, N, dtype, read, rng_seed=3):
    rng = np.random.default_rng(rng_seed)
    Xs = e.get_x()
    for t in range(6):
        e.predict(83.33, 0.02 * np.sin(t), Q.astype(dtype), WB, DT)
        e.observe_heading(float(Xs[2]) + 1e-3 * t, True)
        idf = _ids(N, 12 + 4 * t, rng, must=(1, 63, N))
        e.update(make_obs(Xs, idf, dtype, seed=t), R.astype(dtype), idf, True)
        if read:
            e.landmarks()
        if t == 3:
            e.augment(np.asfortranarray(np.array([[300.0, 410.0], [0.2, -0.4]], dtype)), R.astype(dtype))
            if read:
                e.landmarks()


@pytest.mark.parametrize("mode", ["immediate", "deferred"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_single_reads_do_not_perturb(gpu_required, monkeypatch, dtype, mode):
    """A run that reads its landmarks after every update ends bitwise where the same run without reads ends; the
    reads launch no P-GEMM (profiling mode 2 counts every downdate launch)."""
    from conan_slam_amd import EKF

    N = 130
    X, P = make_scenario(N, np.dtype(dtype), seed=21, corr=0.1)
    out = {}
    monkeypatch.setenv("CSLAM_LOOKAHEAD", "0")
    for read in (True, False):
        e = EKF(N + 2, dtype=dtype, quirks=TEXTBOOK, sync_mode=(mode == "immediate"))
        e.set_state(X, P)
        if mode == "deferred":
            e.set_deferred(128)
        e.set_profiling(2)
        _single_script(e, N, dtype, read)
        before = e.stage_times()["downdate"][1]
        e.landmarks()
        e.landmarks(5, 3)
        assert e.stage_times()["downdate"][1] == before, "a read launched a P-GEMM"
        out[read] = (e.get_state(), before)
        e.close()
    (Xa, Pa), na = out[True]
    (Xb, Pb), nb = out[False]
    assert np.array_equal(Xa, Xb) and np.array_equal(Pa, Pb)
    assert na == nb


def test_single_pipeline_mode(gpu_required, monkeypatch):
    """Two-stream mode (CSLAM_PIPELINE=1): the read waits for the P-GEMM in flight on stream B."""
    N = 400
    s = Single(monkeypatch, N, np.float32, env={"CSLAM_PIPELINE": "1", "CSLAM_LOOKAHEAD": "0"}, sync=False)
    rng = np.random.default_rng(31)
    for t in range(3):
        s.predict(83.33, 0.01)
        s.update(_ids(N, 32, rng, must=(1, 63, N)), seed=t)
        s.check(f"pipelined, update {t}")
    s.close()


# ------------------------------------------------------------------------------------------------ batched engine

F32 = np.dtype(np.float32)


class Batch:
    """EKFBatch `a` (read with landmarks()), its twin `t` (read with get_state), per instance the f32 / f64 oracles."""

    def __init__(self, I, N, quirks=TEXTBOOK, extra=0, seed=0, ncap=None):
        from conan_slam_amd import EKFBatch

        self.I = I
        states = [make_scenario(N, F32, seed=seed + i, corr=0.1) for i in range(I)]
        self.a = EKFBatch(I, n_landmarks=N, max_landmarks=N + extra, quirks=quirks)
        self.t = EKFBatch(I, n_landmarks=N, max_landmarks=N + extra, quirks=quirks)
        for b in (self.a, self.t):
            for i, (X, P) in enumerate(states):
                b.set_state(i, X, P)
        self.orc = [OracleState(X, P, F32, quirks, extra) for X, P in states]
        self.hi = [OracleState(X.astype(np.float64), P.astype(np.float64), np.float64, quirks, extra) for X, P in states]
        self.H = [np.diag(h.p()).copy() for h in self.hi]
        self.keep = []
        self.new_from = None

    def _hist(self):
        for i, h in enumerate(self.hi):
            d = np.diag(h.p())
            H = np.zeros_like(d)
            H[: self.H[i].shape[0]] = self.H[i]
            self.H[i] = np.maximum(H, d)

    def predict_each(self, v, s):
        for b in (self.a, self.t):
            b.predict_each(v, s, Q.astype(np.float32), WB, DT)
        for i in range(self.I):
            for o in (self.orc[i], self.hi[i]):
                o.predict(v[i], s[i], Q.astype(o.X.dtype), WB, DT)
        self.new_from = None

    def heading(self, phi):
        for b in (self.a, self.t):
            b.observe_heading(phi, True)
        for o in self.orc + self.hi:
            o.observe_heading(phi, True)
        self._hist()
        self.new_from = None

    def obs(self, m, rng, seed, must=()):
        nf = (self.orc[0].n - 3) // 2
        out = []
        for i in range(self.I):
            idf = _ids(nf, m, rng, must=must)
            out.append((make_obs(self.orc[i].x(), idf, np.float32, seed=seed + 97 * i), idf))
        return out

    def update(self, obs):
        m = len(obs[0][1])
        dz = [_dev(Z.reshape(-1, order="F")) for Z, _ in obs]
        di = [_dev(np.asarray(idf, np.int32)) for _, idf in obs]
        self.keep += dz + di
        for b in (self.a, self.t):
            b.update_device([t.data_ptr() for t in dz], [t.data_ptr() for t in di], m, R.astype(np.float32))
        for i, (Z, idf) in enumerate(obs):
            self.orc[i].update(Z, R.astype(np.float32), idf, True)
            self.hi[i].update(Z.astype(np.float64), R, idf, True)
        self._hist()
        self.new_from = None

    def run(self, steps, m, rng, seed):
        ctrls = [(83.33, 0.01 * np.sin(t)) for t in range(steps)]
        obs_steps, dzs, dis = [], [[] for _ in range(self.I)], [[] for _ in range(self.I)]
        for t in range(steps):
            o = self.obs(m, rng, seed + t, must=(1,))
            obs_steps.append(o)
            for i in range(self.I):
                dzs[i].append(o[i][0].reshape(-1, order="F"))
                dis[i].append(o[i][1])
        dz = [_dev(np.concatenate(z)) for z in dzs]
        di = [_dev(np.concatenate(d).astype(np.int32)) for d in dis]
        self.keep += dz + di
        v = np.array([c[0] for c in ctrls])
        sw = np.array([c[1] for c in ctrls])
        for b in (self.a, self.t):
            b.run(steps, v, sw, Q.astype(np.float32), WB, DT, [t.data_ptr() for t in dz], [t.data_ptr() for t in di], m,
                  R.astype(np.float32))
        for t in range(steps):
            for o in self.orc + self.hi:
                o.predict(ctrls[t][0], ctrls[t][1], Q.astype(o.X.dtype), WB, DT)
            for i in range(self.I):
                Z, idf = obs_steps[t][i]
                self.orc[i].update(Z, R.astype(np.float32), idf, True)
                self.hi[i].update(Z.astype(np.float64), R, idf, True)
            self._hist()
        self.new_from = None

    def augment(self, Zns):
        nf = (self.orc[0].n - 3) // 2
        q = Zns[0].shape[1]
        dz = [_dev(np.asfortranarray(Zn, np.float32).reshape(-1, order="F")) for Zn in Zns]
        self.keep += dz
        for b in (self.a, self.t):
            b.augment_device([t.data_ptr() for t in dz], q, R.astype(np.float32))
        for i in range(self.I):
            self.orc[i].augment(np.asfortranarray(Zns[i], np.float32), R.astype(np.float32))
            self.hi[i].augment(np.asfortranarray(Zns[i], np.float64), R)
        self._hist()
        self.new_from = nf + 1

    def check(self, tag, first=1, count=None, exact_all=False):
        nf = (self.orc[0].n - 3) // 2
        count = nf - first + 1 if count is None else count
        x, ll, vl = self.a.landmarks(first, count)
        assert x.shape == (self.I, count, 2) and ll.shape == (self.I, count, 2, 2) and vl.shape == (self.I, count, 3, 2)
        fx = 3 + 2 * (np.arange(first, first + count) - 1)
        f = np.arange(first, first + count)
        exact = np.ones(count, bool) if exact_all else (f >= self.new_from if self.new_from else None)
        for i in range(self.I):
            X, P = self.t.get_state(i)
            Hmax = np.stack([self.H[i][fx], self.H[i][fx + 1]], axis=1)
            _check(f"{tag} [{i}]", F32, (x[i], ll[i], vl[i]), _blocks(X, P, first, count),
                   _blocks(self.orc[i].x(), self.orc[i].p(), first, count),
                   _blocks(self.hi[i].x(), self.hi[i].p(), first, count), Hmax, exact=exact)
        self.a.flush()  # (the twin's get_state has applied its pending columns: keep the two batches in lockstep)
        return x, ll, vl

    def close(self):
        self.a.close()
        self.t.close()


def _new_features(I, q, cycle):
    return [np.array([[250.0 + 40 * cycle + 10 * i + 15 * j for j in range(q)],
                      [0.5 - 0.4 * cycle + 0.1 * i - 0.3 * j for j in range(q)]], np.float32) for i in range(I)]


@pytest.mark.parametrize("stop", ["run", "update", "heading", "augment"])
def test_batch_states(gpu_required, stop):
    """After run() (window panels pending), after a window of one update, after heading steps (rank-1 columns), after
    augment (the new rows have nothing pending: bitwise)."""
    I, N = 3, 200
    b = Batch(I, N, extra=4, seed=50)
    rng = np.random.default_rng(1)
    b.run(3, 16, rng, seed=1)
    if stop != "run":
        b.predict_each([83.0, 83.4, 82.8], [0.01, -0.02, 0.0])
        b.update(b.obs(7, rng, 100, must=(1, 63, N)))
    if stop in ("heading", "augment"):
        for t in range(3):
            b.predict_each([83.0, 83.4, 82.8], [0.01 * t, 0.0, -0.01])
            b.heading(float(b.hi[0].x()[2]) + 1e-3)
    if stop == "augment":
        b.augment(_new_features(I, 2, 0))
    b.check(f"batch after {stop}")
    for bb in (b.a, b.t):
        bb.flush()
    b.check(f"batch after {stop}, flushed", exact_all=True)
    b.close()


def test_batch_growth_across_a_row_tile(gpu_required):
    """N = 62 (n = 127) grows to 64 landmarks (n = 131) with panels pending, then updates observe the new rows and
    the tile-straddling landmark 63."""
    I, N = 2, 62
    b = Batch(I, N, extra=2, seed=60)
    rng = np.random.default_rng(2)
    b.predict_each([83.0, 83.3], [0.01, 0.0])
    b.update(b.obs(5, rng, 1, must=(1, 62)))
    b.augment(_new_features(I, 2, 1))
    assert b.a.n == 131
    b.check("grown")
    b.predict_each([83.0, 83.3], [0.0, 0.02])
    b.heading(float(b.hi[0].x()[2]))
    b.update(b.obs(6, rng, 2, must=(63, 64, 1)))
    b.check("grown, after an update of the new rows")
    b.check("grown, f = 63 alone", first=63, count=1)
    b.check("grown, last", first=64, count=1)
    b.close()


def test_batch_bad_arguments_and_edges(gpu_required):
    import ctypes as C

    from conan_slam_amd._capi import ERR_BAD_ARG

    I, N = 2, 70
    b = Batch(I, N, seed=70)
    rng = np.random.default_rng(3)
    b.predict_each([83.0, 83.3], [0.01, 0.0])
    b.update(b.obs(9, rng, 1, must=(1, 63, N)))
    full = b.a.landmarks()
    for first, count in ((1, 1), (N, 1), (63, 2), (1, N)):
        part = b.a.landmarks(first, count)
        for p_, f_ in zip(part, full):
            assert np.array_equal(p_, f_[:, first - 1: first - 1 + count]), (first, count)
    L, h = b.a._L, b.a._h
    buf = np.zeros(I * 12 * (N + 2), np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.cslam_ekf_batch_get_landmarks(h, 1, 0, p, p, p) == 0
    for first, count in ((0, 1), (1, N + 1), (N, 2), (N + 1, 1), (2, -1), (N + 2, 0)):
        assert L.cslam_ekf_batch_get_landmarks(h, first, count, p, p, p) == ERR_BAD_ARG, (first, count)
    assert L.cslam_ekf_batch_get_landmarks(h, 1, 1, None, None, None) == ERR_BAD_ARG
    assert L.cslam_ekf_batch_get_landmarks(None, 1, 1, p, p, p) == ERR_BAD_ARG
    assert not np.any(buf)
    b.check("after the refused calls")
    b.close()


def _batch_script(b, dz, di, read, nan_in=None):
    """Six observation cycles of the demo cadence: predict_each + heading per step, update (m = 5) + augment (q = 1)."""
    I = b.instances
    zo = io = 0
    for c in range(6):
        for t in range(3):
            v = [83.0 + 0.2 * i for i in range(I)]
            if nan_in is not None and c == 2 and t == 1:
                v[nan_in] = float("nan")
            b.predict_each(v, [0.01 * (t - i) for i in range(I)], Q.astype(np.float32), WB, DT)
            b.observe_heading(0.02 * (3 * c + t), True)
        b.update_device([z.data_ptr() + 4 * zo for z in dz], [d.data_ptr() + 4 * io for d in di], 5, R.astype(np.float32))
        zo, io = zo + 10, io + 5
        if read:
            b.landmarks()
        b.augment_device([z.data_ptr() + 4 * zo for z in dz], 1, R.astype(np.float32))
        zo += 2
        if read:
            b.landmarks()


def _batch_inputs(I, N, seed):
    rng = np.random.default_rng(seed)
    states = [make_scenario(N, F32, seed=seed + i, corr=0.1) for i in range(I)]
    dz, di = [], []
    for i in range(I):
        zs, ids = [], []
        for c in range(6):
            idf = _ids(N, 5, rng, must=(1 + c, N))
            zs.append(make_obs(states[i][0], idf, np.float32, seed=c + 11 * i).reshape(-1, order="F"))
            ids.append(idf)
            zs.append(np.array([280.0 + 10 * c + i, 0.3 - 0.1 * c], np.float32))
        dz.append(_dev(np.concatenate(zs)))
        di.append(_dev(np.concatenate(ids).astype(np.int32)))
    return states, dz, di


def test_batch_reads_do_not_perturb(gpu_required):
    """The demo cadence with a read after every update and every augment ends bitwise where the run without reads
    ends; the reads move neither the P-GEMM launch count (set_profiling(1)) nor windows()."""
    from conan_slam_amd import EKFBatch

    I, N = 3, 120
    states, dz, di = _batch_inputs(I, N, seed=80)
    out = {}
    for read in (True, False):
        b = EKFBatch(I, n_landmarks=N, max_landmarks=N + 6, quirks=TEXTBOOK)
        for i, (X, P) in enumerate(states):
            b.set_state(i, X, P)
        b.set_profiling(1)
        _batch_script(b, dz, di, read)
        launches, wins = b.pgemm_time()[1], b.windows()
        b.landmarks()
        b.landmarks(3, 4)
        assert b.pgemm_time()[1] == launches and b.windows() == wins, "a read launched a P-GEMM or a window"
        out[read] = ([b.get_state(i) for i in range(I)], launches, wins)
        b.close()
    for i in range(I):
        (Xa, Pa), (Xb, Pb) = out[True][0][i], out[False][0][i]
        assert np.array_equal(Xa, Xb) and np.array_equal(Pa, Pb), i
    assert out[True][1:] == out[False][1:]


def test_batch_instance_isolation(gpu_required):
    """A NaN speed in instance 1 leaves the reads of instances 0 and 2 bitwise as in the run with that control finite."""
    from conan_slam_amd import EKFBatch

    I, N = 3, 120
    states, dz, di = _batch_inputs(I, N, seed=90)
    reads = []
    for nan_in in (None, 1):
        b = EKFBatch(I, n_landmarks=N, max_landmarks=N + 6, quirks=TEXTBOOK)
        for i, (X, P) in enumerate(states):
            b.set_state(i, X, P)
        _batch_script(b, dz, di, False, nan_in=nan_in)
        reads.append(b.landmarks())
        b.close()
    for a, c in zip(*reads):
        for i in (0, 2):
            assert np.array_equal(a[i], c[i]), i
    assert not np.all(np.isfinite(reads[1][0][1]))


def test_batch_noisy_demo_cadence(gpu_required):
    """The noisy demo study (tools/mc_demo.py's calls, 4 runs x 600 steps, a growing map): the read at the end matches
    the twin and the oracles."""
    from test_batch_mc_demo_gpu import _replay, _study

    recs, refs, his = _study(TEXTBOOK, 600, seeds=[1000, 1001, 1002, 1003])
    a, _ = _replay(recs, TEXTBOOK)
    b, _ = _replay(recs, TEXTBOOK)
    x, ll, vl = a.landmarks()
    I = len(recs)
    for i in range(I):
        X, P = b.get_state(i)
        tx, tll, tvl = _blocks(X, P, 1, a.n_landmarks)
        assert np.array_equal(x[i], tx) and np.array_equal(vl[i], tvl), i
        assert_close(f"demo P_ll[{i}] vs twin", ll[i], tll, 1e-5)
        assert_close(f"demo x[{i}] vs oracle", x[i], _blocks(refs[i]["X"], refs[i]["P"], 1, a.n_landmarks)[0], 1e-4,
                     _blocks(his[i]["X"], his[i]["P"], 1, a.n_landmarks)[0], fair=8.0)
    a.close()
    b.close()
