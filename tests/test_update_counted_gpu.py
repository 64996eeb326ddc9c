"""cslam_ekf_update_counted (ekf_counted_kernels.hpp): the batch update whose observation count c = clamp(*d_count, 0,
m_cap) is read on the device by every kernel of the chain, while the host plans for m_cap.

References: the CPU oracle's update with the first c observations (helpers.OracleState, SURVEY 8d tolerances as written
in helpers.assert_close, with the x4 fairness rule against the f64 oracle) and a twin handle driven with update_device.
Every case runs at N = 70 landmarks (n = 143: two 128-row tiles; landmark 63 straddles them).
  1  against the oracle at the boundaries of every factor kernel class, smallest and largest count inside each
  2  under pending columns: in-gather correction, its wide form, and the Y = H Wp path with the MFMA correction
  3  c = 0 is exactly nothing
  4  entries c .. m_cap-1 of dZ / d_idf are never used
  5  a count outside 0..m_cap is clamped and flagged
  6  the count is read in stream order, not in call order
  7  a queued look-ahead update is drained as a window of one; the counted update adds none
  8  errors change nothing
(zero_column_argument in test_update_counted_cpu.py is the oracle-side statement behind the inert columns.)"""
import ctypes as C

import numpy as np
import pytest

from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs, make_scenario
from pyoracle import REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu

N = 70
R22 = np.diag([0.08, 0.0024])
Q_CTRL = np.diag([0.18, 6e-4])
F32, F64 = np.float32, np.float64

SHAPES_BOTH = {2: (0, 1, 2), 8: (0, 1, 3, 8), 9: (0, 1, 8, 9), 17: (0, 1, 8, 16, 17), 32: (0, 1, 31, 32)}
SHAPES_F32 = {33: (1, 32, 33), 64: (0, 1, 33, 64)}


def _shape_cases():
    out = [pytest.param(dt, mc, c, id=f"{np.dtype(dt).name}-{mc}:{c}")
           for dt in (F32, F64) for mc, cs in SHAPES_BOTH.items() for c in cs]
    return out + [pytest.param(F32, mc, c, id=f"float32-{mc}:{c}") for mc, cs in SHAPES_F32.items() for c in cs]


def pick(m, seed):
    """m distinct 1-based landmarks, the tile-straddling one (63) and the last one among them"""
    rng = np.random.default_rng(seed)
    special = [63, N][:m]
    rest = [int(f) for f in rng.permutation(N) + 1 if f not in special]
    idf = np.array(special + rest[: m - len(special)], dtype=np.int32)
    return idf[rng.permutation(m)]


_INPUTS = {}


def inputs(dtype, m_cap, quirks=TEXTBOOK, seed=0):
    """(X0, P0, idf[m_cap], Z[2, m_cap], R) of one shape: built once and never written to"""
    key = (np.dtype(dtype).name, m_cap, quirks, seed)
    if key not in _INPUTS:
        X, P = make_scenario(N, dtype, seed=100 + m_cap + seed, corr=0.1 if quirks == REF_EXACT else 0.5)
        idf = pick(m_cap, 7 * m_cap + seed)
        _INPUTS[key] = (X, P, idf, make_obs(X, idf, dtype, seed=m_cap + seed), R22.astype(dtype))
        for a in _INPUTS[key]:
            a.setflags(write=False)
    return _INPUTS[key]


def engine(monkeypatch, dtype, quirks=TEXTBOOK, deferred=0, env=None, sync=False):
    from conan_slam_amd import EKF

    env = {"CSLAM_LOOKAHEAD": "0", **(env or {})}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = EKF(N, dtype=dtype, quirks=quirks, sync_mode=sync)
    for k in env:
        monkeypatch.delenv(k)
    e.set_deferred(deferred)
    return e


class Dev:
    """Z, idf and the count in device memory (kept alive by the object)"""

    def __init__(self, Z, idf, count):
        import torch

        self.Z = torch.from_numpy(np.array(np.asarray(Z).reshape(-1, order="F"))).cuda()  # (column-major, a copy)
        self.idf = torch.from_numpy(np.array(idf, dtype=np.int32)).cuda()
        self.count = torch.tensor([count], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def counted(self, e, m_cap, R):
        e.update_counted(self.Z.data_ptr(), m_cap, R, self.idf.data_ptr(), self.count.data_ptr())

    def plain(self, e, m, R):
        e.update_device(self.Z.data_ptr(), m, R, self.idf.data_ptr(), batch=True)


def oracle_pair(X, P, dtype, quirks):
    return (OracleState(X, P, dtype, quirks),
            OracleState(X.astype(F64), np.asfortranarray(P.astype(F64)), F64, quirks))


def oracle_update(orc, hi, Z, R, idf, c):
    if c:
        assert orc.update(np.asfortranarray(Z[:, :c]), R, idf[:c], True) == 0
        hi.update(np.asfortranarray(Z[:, :c].astype(F64)), R.astype(F64), idf[:c], True)


def check_state(e, orc, hi, dtype):
    Xg, Pg = e.get_state()
    dt = np.dtype(dtype)
    assert_close("X", Xg, orc.x(), X_RTOL[dt], hi.x())
    assert_close("P", Pg, orc.p(), P_RTOL[dt], hi.p())
    return Xg, Pg


def bits_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("dtype,m_cap,c", _shape_cases())
def test_counted_update_matches_the_oracle_update_of_c(gpu_required, monkeypatch, dtype, m_cap, c):
    X, P, idf, Z, R = inputs(dtype, m_cap)
    e = engine(monkeypatch, dtype)
    e.set_state(X, P)
    d = Dev(Z, idf, c)
    d.counted(e, m_cap, R)
    assert e.factor_status() == 0
    orc, hi = oracle_pair(X, P, dtype, TEXTBOOK)
    oracle_update(orc, hi, Z, R, idf, c)
    got = check_state(e, orc, hi, dtype)
    if c == m_cap:  # the same kernels' bodies with the same k: the twin's update_device, bit for bit
        t = engine(monkeypatch, dtype)
        t.set_state(X, P)
        d.plain(t, c, R)
        assert bits_equal(got, t.get_state())
        t.close()
    e.close()


def test_counted_update_ref_exact(gpu_required, monkeypatch):
    X, P, idf, Z, R = inputs(F32, 17, REF_EXACT)
    e = engine(monkeypatch, F32, REF_EXACT)
    e.set_state(X, P)
    d = Dev(Z, idf, 8)
    d.counted(e, 17, R)
    assert e.factor_status() == 0
    orc, hi = oracle_pair(X, P, F32, REF_EXACT)
    oracle_update(orc, hi, Z, R, idf, 8)
    check_state(e, orc, hi, F32)
    e.close()


# ------------------------------------------------------------------------------------------------ 2
HEADINGS = (0.31, 0.29, 0.305)


def put_pending(target, kind, dtype, X):
    """the pending columns of one variant on an engine or an oracle pair (same calls on both)"""
    objs = target if isinstance(target, tuple) else (target,)
    if kind in ("heading", "both"):
        for phi in HEADINGS:
            for o in objs:
                o.observe_heading(phi, True)
    if kind in ("update", "both"):
        idf = pick(32, 991)
        R = R22.astype(dtype)
        for o in objs:
            Zo = make_obs(X, idf, dtype, seed=55)
            if isinstance(o, OracleState):
                assert o.update(np.asfortranarray(Zo.astype(o.X.dtype)), R.astype(o.X.dtype), idf, True) == 0
            else:
                o.update(Zo, R, idf, batch=True)


@pytest.mark.parametrize("kind", ["heading", "update", "both"])
@pytest.mark.parametrize("m_cap,c", [(9, 1), (9, 8), (32, 1), (32, 31)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_counted_update_under_pending_columns(gpu_required, monkeypatch, dtype, m_cap, c, kind):
    """3 heading columns (corrected inside the gather kernel), a pending 32-observation update (64 columns: the wide
    gather form), both (67 columns: Y = H Wp and the MFMA correction; with m_cap = 32 the window of 128 has no room for
    64 more columns, so the pending ones are applied first, as update_device would)."""
    X, P, idf, Z, R = inputs(dtype, m_cap, seed=3)
    e = engine(monkeypatch, dtype, deferred=128)
    e.set_state(X, P)
    put_pending(e, kind, dtype, X)
    d = Dev(Z, idf, c)
    d.counted(e, m_cap, R)
    assert e.factor_status() == 0
    orc, hi = oracle_pair(X, P, dtype, TEXTBOOK)
    put_pending((orc, hi), kind, dtype, X)
    oracle_update(orc, hi, Z, R, idf, c)
    check_state(e, orc, hi, dtype)
    e.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("pending", [False, True], ids=["clean", "pending"])
@pytest.mark.parametrize("dtype,m_cap", [(F32, 2), (F32, 17), (F32, 64), (F64, 2), (F64, 17)])
def test_count_zero_is_exactly_nothing(gpu_required, monkeypatch, dtype, m_cap, pending):
    X, P, idf, Z, R = inputs(dtype, m_cap)
    states = []
    for counted in (True, False):
        e = engine(monkeypatch, dtype, deferred=128 if pending else 0)
        e.set_state(X, P)
        if pending:
            put_pending(e, "heading", dtype, X)
        e.predict(83.33, 0.02, Q_CTRL.astype(dtype), 73.0, 0.01)
        if counted:
            d = Dev(Z, idf, 0)
            d.counted(e, m_cap, R)
            assert e.factor_status() == 0
        states.append(e.get_state())
        e.close()
    assert not np.array_equal(states[1][0][:3], X[:3])  # (the predicted state is there)
    assert bits_equal(*states)


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("m_cap,c", [(17, 8), (32, 1)])
def test_the_tail_is_never_used(gpu_required, monkeypatch, m_cap, c):
    from conan_slam_amd._capi import FACTOR_BAD_IDF

    X, P, idf, Z, R = inputs(F32, m_cap)
    Zp, ip = Z.copy(), idf.copy()
    Zp[:, c:] = np.nan
    ip[c:] = np.resize(np.array([0, -5, N + 7, idf[0]], dtype=np.int32), m_cap - c)
    states = []
    for Zc, ic in ((Z, idf), (Zp, ip)):
        e = engine(monkeypatch, F32)
        e.set_state(X, P)
        d = Dev(Zc, ic, c)
        d.counted(e, m_cap, R)
        assert e.factor_status() == 0
        states.append(e.get_state())
        e.close()
    assert bits_equal(*states)
    assert np.all(np.isfinite(states[1][0])) and np.all(np.isfinite(states[1][1]))
    ib = idf.copy()
    ib[c - 1] = N + 7  # inside the first c entries: clamped by the kernels and reported
    e = engine(monkeypatch, F32)
    e.set_state(X, P)
    d = Dev(Z, ib, c)
    d.counted(e, m_cap, R)
    assert e.factor_status() & FACTOR_BAD_IDF
    e.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_count_outside_the_range_is_clamped_and_flagged(gpu_required, monkeypatch, dtype):
    from conan_slam_amd._capi import FACTOR_COUNT_CLAMPED

    m_cap = 9
    X, P, idf, Z, R = inputs(dtype, m_cap)

    def run(count):
        e = engine(monkeypatch, dtype)
        e.set_state(X, P)
        d = Dev(Z, idf, count)
        d.counted(e, m_cap, R)
        flags, st = e.factor_status(), e.get_state()
        e.close()
        return flags, st

    full, none, mid = run(m_cap), run(0), run(4)
    over, under = run(m_cap + 5), run(-1)
    assert full[0] == none[0] == mid[0] == 0
    assert over[0] == FACTOR_COUNT_CLAMPED and under[0] == FACTOR_COUNT_CLAMPED
    assert bits_equal(over[1], full[1]) and bits_equal(under[1], none[1])
    assert not bits_equal(full[1], none[1]) and not bits_equal(mid[1], full[1])


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("dtype", [F32, F64], ids=["float32", "float64"])
def test_count_is_read_in_stream_order(gpu_required, monkeypatch, dtype):
    """One count buffer, rewritten by copies enqueued on the handle's chain stream: before the first counted update (the
    buffer holds another value when the call is made) and between the two.  The host never waits in between."""
    import torch

    m_cap, c1, c2 = 17, 5, 12
    X, P, idf, Z, R = inputs(dtype, m_cap)
    idf2 = pick(m_cap, 4242)
    Z2 = make_obs(X, idf2, dtype, seed=77)
    e, t = engine(monkeypatch, dtype), engine(monkeypatch, dtype)
    for h in (e, t):
        h.set_state(X, P)
    a, b = Dev(Z, idf, m_cap), Dev(Z2, idf2, 0)
    # (device-to-device copies: a pinned host source would make the allocator record an event on the handle's stream when
    # the source is freed, which may be after the handle -- and its stream -- are gone)
    src = torch.tensor([c1, c2], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    chain = torch.cuda.ExternalStream(e.streams()[0])
    with torch.cuda.stream(chain):
        a.count.copy_(src[0:1], non_blocking=True)
    e.update_counted(a.Z.data_ptr(), m_cap, R, a.idf.data_ptr(), a.count.data_ptr())
    with torch.cuda.stream(chain):
        a.count.copy_(src[1:2], non_blocking=True)
    e.update_counted(b.Z.data_ptr(), m_cap, R, b.idf.data_ptr(), a.count.data_ptr())
    del chain
    a.plain(t, c1, R)
    b.plain(t, c2, R)
    assert e.factor_status() == 0 and t.factor_status() == 0
    (Xe, Pe), (Xt, Pt) = e.get_state(), t.get_state()
    dt = np.dtype(dtype)
    assert_close("X", Xe, Xt, X_RTOL[dt])
    assert_close("P", Pe, Pt, P_RTOL[dt])
    orc, hi = oracle_pair(X, P, dtype, TEXTBOOK)
    oracle_update(orc, hi, Z, R, idf, c1)
    oracle_update(orc, hi, Z2, R, idf2, c2)
    check_state(e, orc, hi, dtype)
    e.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 7
def test_queued_lookahead_update_is_drained_as_a_window_of_one(gpu_required, monkeypatch):
    X, P, idf, Z, R = inputs(F32, 17)
    idf2 = pick(17, 4243)
    Z2 = make_obs(X, idf2, F32, seed=78)
    e = engine(monkeypatch, F32, deferred=128, env={"CSLAM_LOOKAHEAD": "1"})
    e.set_state(X, P)
    a, b = Dev(Z, idf, 17), Dev(Z2, idf2, 9)
    a.plain(e, 17, R)
    assert e.lookahead_windows() == 0  # (queued: a window needs a second update or a drain)
    b.counted(e, 17, R)
    assert e.lookahead_windows() == 1
    assert e.factor_status() == 0
    orc, hi = oracle_pair(X, P, F32, TEXTBOOK)
    oracle_update(orc, hi, Z, R, idf, 17)
    oracle_update(orc, hi, Z2, R, idf2, 9)
    check_state(e, orc, hi, F32)
    assert e.lookahead_windows() == 1
    e.close()


# ------------------------------------------------------------------------------------------------ 8
def test_errors_change_nothing(gpu_required, monkeypatch):
    from conan_slam_amd._capi import ERR_BAD_ARG, CslamError

    def call(e, d, m_cap, R, batch=1, dZ=True, dI=True, dC=True, r=True):
        vp = C.c_void_p
        return e._L.cslam_ekf_update_counted(e._h, vp(d.Z.data_ptr()) if dZ else None, C.c_int(m_cap),
                                             R.ctypes.data_as(vp) if r else None, vp(d.idf.data_ptr()) if dI else None,
                                             vp(d.count.data_ptr()) if dC else None, C.c_int(batch))

    for dtype, too_many in ((F32, 65), (F64, 33)):
        X, P, idf, Z, R = inputs(dtype, 17)
        R = np.asfortranarray(R)
        e = engine(monkeypatch, dtype)
        e.set_state(X, P)
        before = e.get_state()
        Zbig, ibig = np.zeros((2, 80), dtype=dtype, order="F"), np.ones(80, dtype=np.int32)
        Zbig[:, :17], ibig[:17] = Z, idf
        d = Dev(Zbig, ibig, 5)
        assert call(e, d, too_many, R) == ERR_BAD_ARG
        assert call(e, d, -1, R) == ERR_BAD_ARG
        assert call(e, d, 17, R, batch=0) == ERR_BAD_ARG
        for missing in ("dZ", "dI", "dC", "r"):
            assert call(e, d, 17, R, **{missing: False}) == ERR_BAD_ARG, missing
        assert e._L.cslam_ekf_update_counted(None, None, C.c_int(1), None, None, None, C.c_int(1)) == ERR_BAD_ARG
        assert call(e, d, 0, R) == 0  # m_cap = 0: accepted, nothing happens
        assert e.factor_status() == 0
        assert bits_equal(e.get_state(), before)
        e.set_sync_mode(True)
        assert call(e, d, 17, R) == ERR_BAD_ARG
        assert bits_equal(e.get_state(), before)
        e.set_sync_mode(False)
        assert call(e, d, 17, R) == 0  # (the same call is accepted once nothing is wrong with it)
        assert not bits_equal(e.get_state(), before)
        with pytest.raises(CslamError) as err:  # documented: k of a counted update is known on the device only
            e.debug_last_update()
        assert err.value.code == ERR_BAD_ARG
        e.close()
    X, P, idf, Z, R = inputs(F32, 17)
    p = engine(monkeypatch, F32, env={"CSLAM_PIPELINE": "1"})
    p.set_state(X, P)
    before = p.get_state()
    d = Dev(Z, idf, 5)
    assert call(p, d, 17, np.asfortranarray(R)) == ERR_BAD_ARG
    assert bits_equal(p.get_state(), before)
    p.close()
