"""cslam_ekf_augment_device (ekf_augment_kernels.hpp): Slam::augment with the new features read from device memory, all of a
call's features in one launch per 64.

References: a twin handle given the same Z through cslam_ekf_augment (one launch per feature), BIT FOR BIT, and the CPU
oracle's augment with the per-call tolerances of test_ekf_gpu.py (helpers.X_RTOL / P_RTOL with the x4 fairness rule
against the f64 oracle).
  1  twin parity over the shapes (N0 landmarks before, q new): the empty map, features across the 128-row tile boundary
     (N0 = 62: rows 127 | 128) and the 256-thread block boundary (N0 = 126: len0 = 255), a chunk and one feature more, a
     call that fills the capacity exactly; block-lower and full storage
  2  entries of dZ beyond 2q are never read
  3  pending columns stay pending: an update observing a new and an old feature afterwards, the downdate launches
  4  a held predict and 5 a queued look-ahead update are launched first, as by cslam_ekf_augment
  6  the launch count  7  errors change nothing  8  the simulator's device ZN
  9  the eight-step loop of augment_loop.py through EKF.associate_update_augment"""
import ctypes as C

import numpy as np
import pytest

from assoc_builders import GATES, R_OBS
from augment_loop import CTRL, N_NEW, NF0, NF_END, get_loop, initial_state
from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs, make_scenario
from pyoracle import REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
R22 = np.array([[0.08, 0.004], [0.004, 0.0024]])
Q_CTRL = np.diag([0.18, 6e-4])
CHUNK = 64
# (N0, q, spare capacity)
SHAPES = [(0, 1, 2), (0, 3, 2), (4, 2, 2), (60, 5, 2), (62, 1, 2), (62, 4, 2), (63, 2, 2), (126, 2, 2), (126, 40, 2),
          (10, CHUNK + 1, 2), (30, 7, 0)]
_INPUTS = {}


def inputs(dtype, N0, q, seed=0):
    """(X0, P0, Z[2, q], R) of one shape: built once and never written to"""
    key = (np.dtype(dtype).name, N0, q, seed)
    if key not in _INPUTS:
        X, P = make_scenario(N0, dtype, seed=500 + N0 + q + seed)
        rng = np.random.default_rng(900 + N0 + 13 * q + seed)
        Z = np.asfortranarray(np.stack([rng.uniform(5.0, 40.0, q), rng.uniform(-3.0, 3.0, q)]).astype(dtype))
        _INPUTS[key] = (X, P, Z, R22.astype(dtype))
        for a in _INPUTS[key]:
            a.setflags(write=False)
    return _INPUTS[key]


def engine(monkeypatch, nmax, dtype, quirks=TEXTBOOK, deferred=0, env=None, sync=False):
    from conan_slam_amd import EKF

    env = {"CSLAM_LOOKAHEAD": "0", **(env or {})}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = EKF(nmax, dtype=dtype, quirks=quirks, sync_mode=sync)
    for k in env:
        monkeypatch.delenv(k)
    e.set_deferred(deferred)
    return e


def to_device(a, dtype=None):
    import torch

    a = np.asarray(a) if dtype is None else np.asarray(a, dtype=dtype)
    t = torch.from_numpy(np.array(a.reshape(-1, order="F"))).cuda()  # (column-major, a copy)
    torch.cuda.synchronize()
    return t


def bits_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_oracle(e, X, P, Zs, R, dtype, steps=None):
    """the engine's state against the oracle's augment of the same columns (both dtypes of the fairness rule)"""
    q = Zs.shape[1]
    orc = OracleState(X, P, dtype, TEXTBOOK, extra=q)
    hi = OracleState(X.astype(F64), np.asfortranarray(P.astype(F64)), F64, TEXTBOOK, extra=q)
    orc.augment(np.asfortranarray(Zs), R)
    hi.augment(np.asfortranarray(Zs.astype(F64)), R.astype(F64))
    Xg, Pg = e.get_state()
    dt = np.dtype(dtype)
    assert_close("X", Xg, orc.x(), X_RTOL[dt], hi.x())
    assert_close("P", Pg, orc.p(), P_RTOL[dt], hi.p())


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("storage", ["lower", "full"])
@pytest.mark.parametrize("N0,q,spare", SHAPES, ids=[f"{a}+{b}" + ("" if c else "-full-capacity") for a, b, c in SHAPES])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_twin_parity(gpu_required, monkeypatch, dtype, N0, q, spare, storage):
    X, P, Z, R = inputs(dtype, N0, q)
    a = engine(monkeypatch, N0 + q + spare, dtype, env={"CSLAM_STORAGE": storage})
    t = engine(monkeypatch, N0 + q + spare, dtype, env={"CSLAM_STORAGE": storage})
    for e in (a, t):
        e.set_state(X, P)
    dZ = to_device(Z)
    a.augment_device(dZ.data_ptr(), q, R)
    t.augment(Z, R)
    assert a.n == t.n == 3 + 2 * (N0 + q)
    assert a.augment_launches() == (q + CHUNK - 1) // CHUNK and t.augment_launches() == q
    got, want = a.get_state(), t.get_state()
    dX, dP = (float(np.abs(g.astype(F64) - w.astype(F64)).max()) for g, w in zip(got, want))
    print(f"twin parity {np.dtype(dtype).name} {N0}+{q} {storage}: max |dX| {dX:.3e}, max |dP| {dP:.3e}")
    assert bits_equal(got, want), f"max |dX| {dX:.3e}, max |dP| {dP:.3e}"
    for e in (a, t):
        check_oracle(e, X, P, Z, R, dtype)
    a.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_entries_beyond_2q_are_never_read(gpu_required, monkeypatch, dtype):
    N0, q = 62, 4
    X, P, Z, R = inputs(dtype, N0, q)
    tail = np.array([np.nan, 1e30, -np.inf, 3e38 if dtype == F32 else 1e300, np.nan, 0.0], dtype=dtype)
    states = []
    for buf in (Z.reshape(-1, order="F"), np.concatenate([Z.reshape(-1, order="F"), tail])):
        e = engine(monkeypatch, N0 + q + 3, dtype)
        e.set_state(X, P)
        d = to_device(buf)
        e.augment_device(d.data_ptr(), q, R)
        states.append(e.get_state())
        e.close()
    assert bits_equal(*states)
    assert all(np.all(np.isfinite(s)) for s in states[1])


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("storage", ["lower", "full"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_pending_columns_stay_pending(gpu_required, monkeypatch, dtype, storage):
    N0, q = 62, 2
    X, P, Z, R = inputs(dtype, N0, q)
    idf1 = np.array([3, 17, 40, 62, 9, 25, 51, 33, 60], dtype=np.int32)
    Z1 = make_obs(X, idf1, dtype, seed=5)
    out = []
    for device in (True, False):
        e = engine(monkeypatch, N0 + q, dtype, deferred=128, env={"CSLAM_STORAGE": storage})
        e.set_profiling(2)
        e.set_state(X, P)
        e.update(Z1, R, idf1, batch=True)          # 18 columns, left pending
        assert e.stage_times()["downdate"][1] == 0
        if device:
            d = to_device(Z)
            e.augment_device(d.data_ptr(), q, R)
        else:
            e.augment(Z, R)
        assert e.stage_times()["downdate"][1] == 0  # still pending
        idf2 = np.array([N0 + 2, 17], dtype=np.int32)   # one new and one old feature
        Z2 = make_obs(e.get_x(), idf2, dtype, seed=6)
        e.update(Z2, R, idf2, batch=True)
        st = e.get_state()
        out.append((st, e.stage_times()["downdate"][1], e.factor_status(), Z2))
        e.close()
    (sa, la, fa, za), (st, lt, ft, zt) = out
    assert np.array_equal(za, zt)   # (X after the augment carried the same bits already)
    assert fa == ft == 0 and la == lt
    assert bits_equal(sa, st)
    assert not np.array_equal(sa[0][:3], X[:3])


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_a_held_predict_is_applied_first(gpu_required, monkeypatch, dtype):
    N0, q = 60, 5
    X, P, Z, R = inputs(dtype, N0, q)
    states = []
    for device in (True, False):
        e = engine(monkeypatch, N0 + q, dtype)
        e.set_state(X, P)
        e.predict(83.33, 0.02, Q_CTRL.astype(dtype), 73.0, 0.01)
        if device:
            d = to_device(Z)
            e.augment_device(d.data_ptr(), q, R)
        else:
            e.augment(Z, R)
        states.append(e.get_state())
        e.close()
    assert bits_equal(*states)
    assert not np.array_equal(states[0][0][:3], X[:3])   # (the predicted pose is what the new features hang on)
    orc = OracleState(X, P, dtype, TEXTBOOK, extra=q)
    orc.predict(83.33, 0.02, Q_CTRL.astype(dtype), 73.0, 0.01)
    orc.augment(np.asfortranarray(Z), R)
    dt = np.dtype(dtype)
    assert_close("X", states[0][0], orc.x(), 2 * X_RTOL[dt])   # (two calls)
    assert_close("P", states[0][1], orc.p(), 2 * P_RTOL[dt])


# ------------------------------------------------------------------------------------------------ 5
def test_a_queued_lookahead_update_is_launched_first(gpu_required, monkeypatch):
    """N = 70, 17 observations, a deferral window of 128 columns, CSLAM_LOOKAHEAD=1: the shape at which
    test_update_counted_gpu.py gets its window."""
    N0, q, m = 70, 2, 17
    X, P, Z, R = inputs(F32, N0, q)
    idf = (np.random.default_rng(3).permutation(N0) + 1)[:m].astype(np.int32)
    Zu = make_obs(X, idf, F32, seed=11)
    out = []
    for device in (True, False):
        e = engine(monkeypatch, N0 + q, F32, deferred=128, env={"CSLAM_LOOKAHEAD": "1"})
        e.set_state(X, P)
        du, di = to_device(Zu), to_device(idf, np.int32)
        e.update_device(du.data_ptr(), m, R, di.data_ptr(), batch=True)
        assert e.lookahead_windows() == 0   # (queued: a window needs a second update or a drain)
        if device:
            d = to_device(Z)
            e.augment_device(d.data_ptr(), q, R)
        else:
            e.augment(Z, R)
        assert e.lookahead_windows() == 1
        out.append(e.get_state())
        assert e.factor_status() == 0
        e.close()
    assert bits_equal(*out)
    assert not np.array_equal(out[0][0][:3], X[:3])   # (the update ran)


# ------------------------------------------------------------------------------------------------ 6
def test_launch_count(gpu_required, monkeypatch):
    N0, q = 60, 5
    X, P, Z, R = inputs(F32, N0, q)
    e = engine(monkeypatch, N0 + 2 * q, F32)
    e.set_state(X, P)
    d = to_device(Z)
    assert e.augment_launches() == 0
    e.augment_device(d.data_ptr(), 0, R)
    e.augment_device(0, 0, R)
    e.augment(np.zeros((2, 0), F32), R)
    assert e.augment_launches() == 0 and e.n == 3 + 2 * N0
    e.augment_device(d.data_ptr(), q, R)
    assert e.augment_launches() == 1
    e.augment(Z, R)
    assert e.augment_launches() == 1 + q and e.n == 3 + 2 * (N0 + 2 * q)
    e.close()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_errors_change_nothing(gpu_required, monkeypatch, dtype):
    from conan_slam_amd._capi import ERR_BAD_ARG, ERR_CAPACITY

    N0, q = 4, 2
    X, P, Z, R = inputs(dtype, N0, q)
    R = np.asfortranarray(R)
    e = engine(monkeypatch, N0 + q, dtype)
    e.set_state(X, P)
    before = e.get_state()
    big = to_device(np.ones(2 * (q + 1), dtype=dtype))
    vp = C.c_void_p

    def call(dz, qq, r=True):
        return e._L.cslam_ekf_augment_device(e._h, vp(dz) if dz else None, C.c_int(qq), R.ctypes.data_as(vp) if r else None)

    assert call(big.data_ptr(), -1) == ERR_BAD_ARG
    assert call(big.data_ptr(), q, r=False) == ERR_BAD_ARG
    assert call(0, q) == ERR_BAD_ARG
    assert call(0, 0, r=False) == ERR_BAD_ARG
    assert e._L.cslam_ekf_augment_device(None, None, C.c_int(0), None) == ERR_BAD_ARG
    assert e._L.cslam_ekf_augment_launches(e._h, None) == ERR_BAD_ARG
    assert call(big.data_ptr(), q + 1) == ERR_CAPACITY
    assert e.n == 3 + 2 * N0 and e.augment_launches() == 0
    assert bits_equal(e.get_state(), before)
    assert call(0, 0) == 0
    d = to_device(Z)
    assert call(d.data_ptr(), q) == 0      # (the same call is accepted once nothing is wrong with it)
    assert e.n == 3 + 2 * (N0 + q)
    assert call(d.data_ptr(), 1) == ERR_CAPACITY and e.n == 3 + 2 * (N0 + q)
    e.close()


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_the_simulators_device_zn(gpu_required, monkeypatch, dtype):
    from conan_slam_amd import Simulator

    N0, NLM = 20, 27
    X, P = make_scenario(N0, dtype, seed=61, corr=0.2)
    rng = np.random.default_rng(62)
    LM = np.zeros((2, NLM), dtype=dtype, order="F")
    LM[:, :N0] = X[3:].reshape(2, N0, order="F")
    LM[:, N0:] = X[:2, None] + rng.uniform(-30.0, 30.0, size=(2, NLM - N0))
    sim = Simulator(LM, dtype=dtype)
    table = np.zeros(NLM, dtype=np.int32)
    table[:N0] = np.arange(1, N0 + 1)
    sim.table = table                                    # the first N0 landmarks are known, the rest new
    sim.get_observations(X[:3].astype(dtype), 1e6)
    ZF, ZN, idf = sim.data_associate_table(N0)
    mn = ZN.shape[1]
    assert 0 < mn <= NLM - N0     # (the new landmarks in front of the vehicle)
    R = R22.astype(dtype)
    a, t = engine(monkeypatch, NLM, dtype), engine(monkeypatch, NLM, dtype)
    for e in (a, t):
        e.set_state(X, P)
    a.augment_device(sim.device_ptrs()["ZN"], mn, R)
    t.augment(ZN, R)
    assert a.n == t.n == 3 + 2 * (N0 + mn)
    assert bits_equal(a.get_state(), t.get_state())
    a.close()
    t.close()
    sim.close()


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_eight_steps_of_associate_update_augment(gpu_required, monkeypatch, dtype):
    steps, X_end, P_end = get_loop(dtype)
    gates = GATES[0]
    X0, P0 = initial_state(dtype)
    a, t = engine(monkeypatch, NF_END, dtype), engine(monkeypatch, NF_END, dtype)
    R, Q = R_OBS.astype(dtype), CTRL["Q"].astype(dtype)
    for e in (a, t):
        e.set_state(X0, P0)
    for n, s in enumerate(steps):
        for e in (a, t):
            e.predict(CTRL["v"], s["swa"], Q, CTRL["wb"], CTRL["dt"])
            assert e.n == s["n"]
        idf, kind, counts = a.associate_update_augment(s["Z"], R, *gates)
        idf_t, kind_t, counts_t = t.associate_update_counted(s["Z"], R, *gates)
        t.augment(np.asfortranarray(s["Z"][:, kind_t == 2]), R)
        assert np.array_equal(idf, s["idf"]) and np.array_equal(kind, s["kind"]), (n, idf, s["idf"], kind, s["kind"])
        assert np.array_equal(idf_t, s["idf"]) and np.array_equal(kind_t, s["kind"]), n
        assert list(counts) == list(counts_t) == [int((s["kind"] == k).sum()) for k in (1, 2, 0)]
    assert a.factor_status() == 0 and t.factor_status() == 0
    assert a.n == t.n == 3 + 2 * NF_END == 3 + 2 * (NF0 + sum(N_NEW))
    assert a.augment_launches() == len(steps) and t.augment_launches() == sum(N_NEW)
    (Xa, Pa), (Xt, Pt) = a.get_state(), t.get_state()
    assert np.array_equal(Xa, Xt) and np.array_equal(Pa, Pt), (
        f"max |dX| {float(np.abs(Xa - Xt).max()):.3e}, max |dP| {float(np.abs(Pa - Pt).max()):.3e}")
    # 8 x (predict + update + augment) against the oracle loop: the per-call tolerance once per call of a step
    dt = np.dtype(dtype)
    assert_close("X", Xa, X_end, 3 * len(steps) * X_RTOL[dt])
    assert_close("P", Pa, P_end, 3 * len(steps) * P_RTOL[dt])
    a.close()
    t.close()


def test_ref_exact_augments_nothing(gpu_required, monkeypatch):
    """EKF.cpp:307: under REF_EXACT the reference's dataAssociate returns an empty ZN, and so does this loop"""
    steps, _, _ = get_loop(F32)
    X0, P0 = initial_state(F32)
    e = engine(monkeypatch, NF_END, F32, quirks=REF_EXACT)
    e.set_state(X0, P0)
    _, kind, counts = e.associate_update_augment(steps[0]["Z"], R_OBS.astype(F32), *GATES[0])
    assert counts[1] == int((kind == 2).sum()) > 0
    assert e.n == 3 + 2 * NF0 and e.augment_launches() == 0
    e.close()
