"""cslam_ekf_associate_deferred (ekf_assoc_pair_kernel + ekf_assoc_resolve_kernel): the association of the single handle
read from the deferred covariance P = Ps - Wp diag(s) Wp^T without applying it.

Integers are compared only where the reference is decisive (assoc_builders.py, assoc_deferred_ref.py: every comparison
that fixes a decision has a margin of at least 64 x the C oracle's own error).
  1  nothing pending: every case of assoc_builders.CASE_KEYS, both quirks, both gate pairs
  2  columns pending (two modes of the engine, a negative heading column): the answer is the decisive reference on a
     twin's flushed state, and the flip observations show that a read ignoring the panels would answer otherwise
  3  the map grows while columns are pending
  4  the call flushes nothing and perturbs nothing: the run ends bit for bit where it ends without the calls
  5  the split left on the device feeds update_device
  6  errors change nothing
  7  two-stream mode"""
import ctypes as C

import numpy as np
import pytest

from assoc_builders import CASE_KEYS, GATES, case_id, get_case, predicted
from assoc_deferred_ref import NEG_N, SPLIT_NF, check_pending, get_pending, split_scan
from helpers import make_obs, make_scenario
from pyoracle import REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu

QUIRKS = [REF_EXACT, TEXTBOOK]
DTYPES = [np.float32, np.float64]
Q_CTRL = np.diag([0.18, 6e-4])
WB, DT = 73.0, 0.01


def _new(monkeypatch, nmax, dtype, quirks=TEXTBOOK, env=None, sync=True):
    from conan_slam_amd import EKF

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    e = EKF(nmax, dtype=dtype, quirks=quirks, sync_mode=sync)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return e


def _bits_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("quirks", QUIRKS, ids=["ref_exact", "textbook"])
@pytest.mark.parametrize("key", CASE_KEYS, ids=case_id)
def test_deferred_returns_the_decisive_reference(gpu_required, monkeypatch, key, quirks):
    case = get_case(key)
    eng = _new(monkeypatch, case.nf, case.dtype.type, quirks)
    eng.set_state(case.X, case.P)
    for gates in case.gates:
        idf_r, kind_r, _ = case.decisions(gates)
        idf, kind, counts = eng.associate_deferred(case.Z, case.R, *gates, with_counts=True)
        assert np.array_equal(kind, kind_r), (case, gates, kind, kind_r)
        assert np.array_equal(idf, idf_r), (case, gates, idf, idf_r)
        assert list(counts) == [int((kind_r == k).sum()) for k in (1, 2, 0)], (case, gates, counts)
        ZF, ZN, idff = eng.data_associate_deferred(case.Z, case.R, *gates)
        assert np.array_equal(ZF, case.Z[:, kind_r == 1]) and np.array_equal(idff, idf_r[kind_r == 1]), (case, gates)
        if quirks == REF_EXACT:
            assert ZN.shape == (0, 0)
        else:
            assert np.array_equal(ZN, case.Z[:, kind_r == 2]), (case, gates)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2, 7
MODES = {"la0": ({"CSLAM_LOOKAHEAD": "0"}, "pos"), "la1": ({"CSLAM_LOOKAHEAD": "1"}, "la"),
         "pipeline": ({"CSLAM_PIPELINE": "1"}, "pos"), "neg": ({"CSLAM_LOOKAHEAD": "0"}, "neg")}


def _pending_case(monkeypatch, nf, dtype, mode):
    """The builder's steps on a handle and on a twin; the twin is read with get_state (which applies what is pending), the
    builder's promises are checked on THAT state, and the handle must return its decisions with everything still pending."""
    env, variant = MODES[mode]
    p = get_pending(nf, dtype, variant)
    a = _new(monkeypatch, nf, dtype, env=env, sync=False)
    t = _new(monkeypatch, nf, dtype, env=env, sync=False)
    for e in (a, t):
        e.set_state(p.X0, p.P0)
        e.set_deferred(128)
        p.apply(e)
    windows = a.lookahead_windows()
    Xt, Pt = t.get_state()
    case = check_pending(p, Xt, Pt)           # margins >= tau for EVERY observation; the flips flip under the stale blocks
    for gates in p.gates:
        idf_r, kind_r, _ = case.decisions(gates)
        idf, kind = a.associate_deferred(p.Z, p.R, *gates)
        assert np.array_equal(kind, kind_r), (mode, gates, kind, kind_r)
        assert np.array_equal(idf, idf_r), (mode, gates, idf, idf_r)
    if mode == "la1":
        # two updates ran as one window, the third was queued and the call launched it as a window of one
        assert (windows, a.lookahead_windows()) == (1, 2)
    # the call applied nothing: the handle's state, read now, is the twin's bit for bit
    assert _bits_equal(a.get_state(), (Xt, Pt))
    a.close()
    t.close()


@pytest.mark.parametrize("mode", ["la0", "la1"])
@pytest.mark.parametrize("nf", [65, 257])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_deferred_under_pending_columns(gpu_required, monkeypatch, dtype, nf, mode):
    _pending_case(monkeypatch, nf, dtype, mode)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_deferred_under_a_negative_heading_column(gpu_required, monkeypatch, dtype):
    _pending_case(monkeypatch, NEG_N, dtype, "neg")


def test_deferred_in_pipeline_mode(gpu_required, monkeypatch):
    _pending_case(monkeypatch, 257, np.float32, "pipeline")


# ------------------------------------------------------------------------------------------------ 3
def _own_obs(case, feats, dr=0.05):
    return np.asfortranarray(np.stack([predicted(case.X, f - 1, case.dtype) + [dr, 0.001] for f in feats], axis=1).astype(case.dtype))


@pytest.mark.parametrize("nf", [65, 257])
def test_deferred_after_the_map_grew(gpu_required, monkeypatch, nf):
    """nf - 1 features, two updates pending, then augment one landmark (64 -> 65, 256 -> 257: a second wave, a second
    workgroup) while the columns are pending -- the new feature has zero rows in the panels.  The answer equals a fresh
    handle's associate on the twin's state."""
    case = get_case(("A", nf, "float32"))
    n0 = case.n - 2
    a = _new(monkeypatch, nf, np.float32, env={"CSLAM_LOOKAHEAD": "0"}, sync=False)
    t = _new(monkeypatch, nf, np.float32, env={"CSLAM_LOOKAHEAD": "0"}, sync=False)
    z_new = np.asfortranarray(case.Z[:, case.m - 1:case.m])
    gates = case.gates[0]
    for e in (a, t):
        e.set_state(case.X[:n0], np.asfortranarray(case.P[:n0, :n0]))
        e.set_deferred(128)
        for feats in (np.arange(1, 9), np.arange(9, 17)):
            e.update(_own_obs(case, feats), case.R, feats.astype(np.int32), batch=True)
    idf0, kind0 = a.associate_deferred(case.Z, case.R, *gates)    # (the buffers are sized for one workgroup here)
    assert idf0.max() <= nf - 1
    for e in (a, t):
        e.augment(z_new, case.R)
    assert a.n == case.n
    idf1, kind1 = a.associate_deferred(case.Z, case.R, *gates)
    Xt, Pt = t.get_state()
    fresh = _new(monkeypatch, nf, np.float32)
    fresh.set_state(Xt, Pt)
    idf_f, kind_f = fresh.associate(case.Z, case.R, *gates)
    assert np.array_equal(idf1, idf_f) and np.array_equal(kind1, kind_f), (idf1, idf_f, kind1, kind_f)
    assert np.all(kind1 == 1) and idf1[case.m - 1] in (nf, idf0[case.m - 1])
    assert _bits_equal(a.get_state(), (Xt, Pt))
    for e in (a, t, fresh):
        e.close()


# ------------------------------------------------------------------------------------------------ 4
R_DIAG = np.diag([0.08, 0.0024])
K_STEPS, M_STEP, N_RUN = 6, 16, 300


def _run(monkeypatch, dtype, env, deferred, between, profile=False):
    """K_STEPS steps of predict, `between(engine, Z)`, update with a FIXED idf -> (state, downdate launches, tables)"""
    X, P = make_scenario(N_RUN, np.dtype(dtype), seed=3, corr=0.1)
    e = _new(monkeypatch, N_RUN, dtype, env=env, sync=False)
    e.set_state(X, P)
    if deferred:
        e.set_deferred(deferred)
    if profile:
        e.set_profiling(2)
    rng = np.random.default_rng(21)
    tables = []
    for t in range(K_STEPS):
        idf = (rng.permutation(N_RUN)[:M_STEP] + 1).astype(np.int32)
        Z = make_obs(X, idf, np.dtype(dtype), seed=40 + t)
        e.predict(83.33, 0.01 * t, Q_CTRL.astype(dtype), WB, DT)
        if between is not None:
            tables.append(between(e, Z))
        e.update(Z, R_DIAG.astype(dtype), idf, True)
    launches = e.stage_times()["downdate"][1] if profile else None
    state = e.get_state()
    e.close()
    return state, launches, tables


def _deferred_call(e, Z):
    return tuple(np.copy(v) for v in e.associate_deferred(Z, R_DIAG, *GATES[0]))


def _flushing_call(e, Z):
    return tuple(np.copy(v) for v in e.associate(Z, R_DIAG, *GATES[0]))


def _landmark_read(e, Z):
    return e.landmarks(1, 1)


@pytest.mark.parametrize("mode", ["immediate", "deferred"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_deferred_call_flushes_nothing_and_perturbs_nothing(gpu_required, monkeypatch, dtype, mode):
    env, deferred = {"CSLAM_LOOKAHEAD": "0"}, (128 if mode == "deferred" else 0)
    plain = _run(monkeypatch, dtype, env, deferred, None)
    with_calls = _run(monkeypatch, dtype, env, deferred, _deferred_call)
    assert _bits_equal(plain[0], with_calls[0]), "the run with associate_deferred calls ends elsewhere"
    again = _run(monkeypatch, dtype, env, deferred, _deferred_call)
    assert all(_bits_equal(u, v) for u, v in zip(with_calls[2], again[2])) and len(again[2]) == K_STEPS
    assert any((tb[1] == 1).any() for tb in with_calls[2])      # (the calls did associate something)
    # the downdate launches of the run are those of the run without the calls; `associate` in their place adds some
    base = _run(monkeypatch, dtype, env, deferred, None, profile=True)[1]
    assert _run(monkeypatch, dtype, env, deferred, _deferred_call, profile=True)[1] == base
    if mode == "deferred":
        assert _run(monkeypatch, dtype, env, deferred, _flushing_call, profile=True)[1] > base


def test_deferred_call_with_lookahead_drains_as_the_landmark_read(gpu_required, monkeypatch):
    """Look-ahead windows on: the call launches a queued update as a window of one, exactly as get_landmarks does, so the
    run is bit-identical to the one that reads a landmark at the same places."""
    env = {"CSLAM_LOOKAHEAD": "1"}
    ref = _run(monkeypatch, np.float32, env, 128, _landmark_read)
    got = _run(monkeypatch, np.float32, env, 128, _deferred_call)
    assert _bits_equal(ref[0], got[0])


# ------------------------------------------------------------------------------------------------ 5
def _d2h(ptr, count, dtype):
    from conan_slam_amd import _capi

    hip = C.CDLL(_capi.hip_runtime_path or "libamdhip64.so.7")
    out = np.zeros(max(count, 1), dtype=dtype)
    rc = hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(count * out.itemsize), C.c_int(2))
    assert rc == 0
    return out[:count]


def test_split_on_the_device_feeds_update_device(gpu_required, monkeypatch):
    """m = 1, 40, 3 in that order on one handle (the buffers grow), then m = 0: the device lists, given to
    update_device, leave the state bitwise where update with the host lists leaves a twin."""
    case = split_scan()
    gates = GATES[0]
    idf_r, kind_r, _ = case.decisions(gates)
    a = _new(monkeypatch, SPLIT_NF, np.float32)
    t = _new(monkeypatch, SPLIT_NF, np.float32)
    for e in (a, t):
        e.set_state(case.X, case.P)
    known = np.nonzero(kind_r == 1)[0]
    scans = [known[:1], np.arange(40), np.array([known[1], np.nonzero(kind_r == 2)[0][0], known[2]])]
    for cols in scans:
        Z = np.asfortranarray(case.Z[:, cols])
        idf, kind, counts = a.associate_deferred(Z, case.R, *gates, with_counts=True)
        if len(cols) < 40:   # (after the first update the state has moved: the full scan is checked against the builder)
            assert np.all(kind[np.isin(cols, known)] == 1)
        else:
            assert np.array_equal(idf, idf_r) and np.array_equal(kind, kind_r)
            assert list(counts) == [30, 5, 5]
        mf, mn = int(counts[0]), int(counts[1])
        assert (mf, mn, int(counts[2])) == tuple(int((kind == k).sum()) for k in (1, 2, 0))
        dZF, d_idf, dZN, d_counts = a.association_device_ptrs()
        assert np.array_equal(_d2h(d_counts, 3, np.int32), counts)
        assert np.array_equal(_d2h(dZF, 2 * mf, np.float32).reshape(2, mf, order="F"), Z[:, kind == 1])
        assert np.array_equal(_d2h(dZN, 2 * mn, np.float32).reshape(2, mn, order="F"), Z[:, kind == 2])
        assert np.array_equal(_d2h(d_idf, mf, np.int32), idf[kind == 1])
        a.update_device(dZF, mf, case.R, d_idf, batch=True)
        t.update(np.asfortranarray(Z[:, kind == 1]), case.R, idf[kind == 1], batch=True)
        assert _bits_equal(a.get_state(), t.get_state()), len(cols)
    before = a.get_state()
    idf, kind, counts = a.associate_deferred(np.zeros((2, 0), np.float32), case.R, *gates, with_counts=True)
    assert idf.shape == (0,) and kind.shape == (0,) and list(counts) == [0, 0, 0]
    assert _bits_equal(a.get_state(), before)
    a.close()
    t.close()


def test_empty_map_and_all_dropped_scan(gpu_required, monkeypatch):
    case = split_scan()
    empty = _new(monkeypatch, 8, np.float32)
    idf, kind, counts = empty.associate_deferred(case.Z[:, :5], case.R, *GATES[0], with_counts=True)
    assert np.all(idf == 0) and np.all(kind == 2) and list(counts) == [0, 5, 0]
    dZN = empty.association_device_ptrs()[2]
    assert np.array_equal(_d2h(dZN, 10, np.float32).reshape(2, 5, order="F"), case.Z[:, :5])
    empty.close()
    eng = _new(monkeypatch, SPLIT_NF, np.float32)
    eng.set_state(case.X, case.P)
    dropped = np.nonzero(case.decisions(GATES[0])[1] == 0)[0]
    idf, kind, counts = eng.associate_deferred(case.Z[:, dropped], case.R, *GATES[0], with_counts=True)
    assert np.all(idf == 0) and np.all(kind == 0) and list(counts) == [0, 0, len(dropped)]
    eng.close()


# ------------------------------------------------------------------------------------------------ 6
def test_errors_change_nothing(gpu_required, monkeypatch):
    from conan_slam_amd._capi import ERR_BAD_ARG, CslamError

    p = get_pending(65, np.float32, "pos")
    env = {"CSLAM_LOOKAHEAD": "0"}
    a = _new(monkeypatch, 65, np.float32, env=env, sync=False)
    t = _new(monkeypatch, 65, np.float32, env=env, sync=False)
    for e in (a, t):
        e.set_state(p.X0, p.P0)
        e.set_deferred(128)
        e.set_profiling(2)
        p.apply(e)
    with pytest.raises(CslamError) as err:
        a.association_device_ptrs()
    assert err.value.code == ERR_BAD_ARG
    L, h = a._L, a._h
    Z = np.ascontiguousarray(p.Z.reshape(-1, order="F"))
    R = np.asfortranarray(p.R.astype(np.float32))
    out = np.zeros(64, np.int32)
    ip = out.ctypes.data_as(C.POINTER(C.c_int))
    vp = lambda x: x.ctypes.data_as(C.c_void_p)    # noqa: E731
    g = (C.c_double(4.0), C.c_double(25.0))
    assert L.cslam_ekf_associate_deferred(h, vp(Z), C.c_int(-1), vp(R), *g, ip, ip, ip) == ERR_BAD_ARG
    assert L.cslam_ekf_associate_deferred(h, vp(Z), C.c_int(3), None, *g, ip, ip, ip) == ERR_BAD_ARG
    assert L.cslam_ekf_associate_deferred(h, None, C.c_int(3), vp(R), *g, ip, ip, ip) == ERR_BAD_ARG
    assert L.cslam_ekf_associate_deferred(None, vp(Z), C.c_int(3), vp(R), *g, ip, ip, ip) == ERR_BAD_ARG
    with pytest.raises(CslamError):
        a.association_device_ptrs()
    # every output may be NULL
    assert L.cslam_ekf_associate_deferred(h, vp(Z), C.c_int(3), vp(R), *g, None, None, None) == 0
    # nothing was applied: no downdate launch so far on either handle, and the states agree bit for bit
    assert a.stage_times()["downdate"][1] == t.stage_times()["downdate"][1] == 0
    assert _bits_equal(a.get_state(), t.get_state())
    a.close()
    t.close()
