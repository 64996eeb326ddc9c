"""cslam_ekf_associate_deferred_async / cslam_ekf_association_wait, and the loop they exist for: association and counted
update on the handle's stream with no host round trip in between (EKF.associate_update_counted).

  9   async + wait return the integers of associate_deferred on a twin (decisive cases of assoc_builders); a wait with
      nothing outstanding is an error; a second asynchronous call replaces the first
  10  twelve steps of predict + association + update on split_scan()'s map (assoc_counted_loop.py; every observation of
      every step is decisive, proven on the oracle alone by test_assoc_counted_cpu.py):
      (i)  every observation associates: bitwise the twin driven with associate_deferred + update_device(mf)
      (ii) counts (30, 5, 5): the same integers, the state within the per-call tolerances of the twin's.  In f64 a
           counted update takes at most 32 observations, so the f64 run uses the 32-column scan with counts (24, 4, 4)
           and the 40-column one must be refused."""
import numpy as np
import pytest

from assoc_builders import GATES, get_case
from assoc_counted_loop import CTRL, get_loop
from assoc_deferred_ref import SPLIT_NF, split_scan
from helpers import P_RTOL, X_RTOL, assert_close
from pyoracle import TEXTBOOK

pytestmark = pytest.mark.gpu

KEYS = [("A", 65, "float32"), ("C", 0, "float32")]


def _new(monkeypatch, nmax, dtype):
    from conan_slam_amd import EKF

    monkeypatch.setenv("CSLAM_LOOKAHEAD", "0")
    e = EKF(nmax, dtype=dtype, quirks=TEXTBOOK, sync_mode=False)
    monkeypatch.delenv("CSLAM_LOOKAHEAD")
    return e


def _bits_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("which", ["split"] + [f"{k[0]}-{k[1]}" for k in KEYS])
def test_async_and_wait_return_what_the_synchronous_call_returns(gpu_required, monkeypatch, which):
    from conan_slam_amd._capi import ERR_BAD_ARG, CslamError

    case = split_scan() if which == "split" else get_case([k for k in KEYS if f"{k[0]}-{k[1]}" == which][0])
    a, t = _new(monkeypatch, case.nf, case.dtype.type), _new(monkeypatch, case.nf, case.dtype.type)
    for e in (a, t):
        e.set_state(case.X, case.P)
    with pytest.raises(CslamError) as err:
        a.association_wait()
    assert err.value.code == ERR_BAD_ARG
    for gates in case.gates:
        idf_r, kind_r, _ = case.decisions(gates)
        want = t.associate_deferred(case.Z, case.R, *gates, with_counts=True)
        assert np.array_equal(want[0], idf_r) and np.array_equal(want[1], kind_r)
        # a first call on other observations, never waited for: the second call replaces it
        a.associate_deferred_async(np.asfortranarray(case.Z[:, ::-1][:, : max(case.m // 2, 1)]), case.R, *gates)
        a.associate_deferred_async(case.Z, case.R, *gates)
        got = a.association_wait(with_counts=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (case, gates, got, want)
        with pytest.raises(CslamError) as err:   # handed out once
            a.association_wait()
        assert err.value.code == ERR_BAD_ARG
        # a synchronous call discards an outstanding asynchronous one
        a.associate_deferred_async(case.Z, case.R, *gates)
        assert _bits_equal(a.associate_deferred(case.Z, case.R, *gates, with_counts=True), want)
        with pytest.raises(CslamError):
            a.association_wait()
    # m = 0 launches nothing and its wait returns counts 0
    a.associate_deferred_async(np.zeros((2, 0), case.dtype), case.R, *case.gates[0])
    idf, kind, counts = a.association_wait(with_counts=True)
    assert idf.shape == (0,) and kind.shape == (0,) and list(counts) == [0, 0, 0]
    assert _bits_equal(a.get_state(), t.get_state())
    a.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("shape,dtype", [("all", np.float32), ("all", np.float64), ("split", np.float32),
                                         ("split32", np.float64)],
                         ids=["all-float32", "all-float64", "split-float32", "split32-float64"])
def test_twelve_steps_of_associate_and_counted_update(gpu_required, monkeypatch, shape, dtype):
    base = split_scan()
    steps = get_loop(shape, dtype)
    gates = GATES[0]
    a, t = _new(monkeypatch, SPLIT_NF, dtype), _new(monkeypatch, SPLIT_NF, dtype)
    R = base.R.astype(dtype)
    Q = CTRL["Q"].astype(dtype)
    for e in (a, t):
        e.set_state(base.X.astype(dtype), np.asfortranarray(base.P.astype(dtype)))
    dt = np.dtype(dtype)
    if dt == np.float64:   # beyond the f64 range of the counted update: refused, nothing changes
        from conan_slam_amd._capi import ERR_BAD_ARG, CslamError

        with pytest.raises(CslamError) as err:
            a.associate_update_counted(get_loop("split", dtype)[0]["Z"], R, *gates)
        assert err.value.code == ERR_BAD_ARG
    for n, s in enumerate(steps):
        for e in (a, t):
            e.predict(CTRL["v"], s["swa"], Q, CTRL["wb"], CTRL["dt"])
        idf, kind, counts = a.associate_update_counted(s["Z"], R, *gates)
        idf_t, kind_t, counts_t = t.associate_deferred(s["Z"], R, *gates, with_counts=True)
        dZF, d_idf, _, _ = t.association_device_ptrs()
        t.update_device(dZF, int(counts_t[0]), R, d_idf, batch=True)
        assert np.array_equal(idf, s["idf"]) and np.array_equal(kind, s["kind"]), (n, idf, s["idf"])
        assert np.array_equal(idf_t, s["idf"]) and np.array_equal(kind_t, s["kind"]), n
        assert list(counts) == list(counts_t) == [int((s["kind"] == k).sum()) for k in (1, 2, 0)]
    assert a.factor_status() == 0 and t.factor_status() == 0
    (Xa, Pa), (Xt, Pt) = a.get_state(), t.get_state()
    assert not np.array_equal(Xt, base.X.astype(dtype))
    if shape == "all":   # the count equals the capacity: the same kernels' statements with the same k
        assert np.array_equal(Xa, Xt) and np.array_equal(Pa, Pt), (
            f"max |dX| {float(np.abs(Xa - Xt).max()):.3e}, max |dP| {float(np.abs(Pa - Pt).max()):.3e}")
    else:
        assert_close("X", Xa, Xt, X_RTOL[dt])
        assert_close("P", Pa, Pt, P_RTOL[dt])
    a.close()
    t.close()
