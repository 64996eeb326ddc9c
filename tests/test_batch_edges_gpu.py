"""The batched Monte-Carlo engine's windows at the edges of their kernel dispatch (cslam_ekf_batch.hip).  Inputs, the f64
reference drive and the check come from batch_edges_builders.py; test_batch_edges_cpu.py proves on the oracle alone that
the inputs are healthy and that the check rejects a dropped heading column, a dropped observation, a stale column where
the zero-fill should be, a misplaced held predict and exchanged gain rows.

The three dispatch sites, both sides of every boundary, and the test that runs them:
  chain kernel  ekf_la_chain_batch<16 | 32 | 64> by max(ka, kb):
      m = 8 | 9 and 16 | 17 through update(): test_chain_and_wide_dispatch (held predict inside the window or not);
      m = 9, 17 through run(): test_run_windows_equal_solo_lookahead_runs.
  wide kernel   ekf_la_wide_batch | ekf_la_wide_batch_k64 at m = 31 | 32 (k = 62: two padded factor columns):
      test_chain_and_wide_dispatch, test_run_windows_equal_solo_lookahead_runs (m = 31; m = 32 at n = 129),
      test_instance_count (m = 31); the A/B forms CSLAM_LA_K64=0 (general kernel at m = 32) and
      CSLAM_BATCH_WIDE_PAIRS=1 (ekf_la_wide_batch1): test_ab_forms.
  P-GEMM class  <0,2,32> | <0,4,24> | <0,4,32> by k8 = round_up(kp, 8), with the zero-fill of columns kp .. cover - 1:
      kp = 64 | 65, 96 | 97, 127 | 128, the forced flush on the 129th column (then kp = 1), kp = 2, 3, 37, 72 (a
      zero-filled column below k8): test_pgemm_class_and_zero_fill; kp = 68 and 100 through run() at m = 17 and 25:
      test_run_windows_equal_solo_lookahead_runs; the final get_state of every segment flushes kp = 2 m = 16 .. 64.
  n = 127, 129, 255, 257 (the last row at and just past a 128-row tile edge): test_tile_boundaries.
Every observed set holds landmark 63 (rows 127 | 128 of P: two tiles) and the last landmark, when the map has them.

update() windows are checked per segment against the f32 oracle with the f64 oracle as the fairness reference, both
restarted from the state the batch itself returned at the start of the segment, at X_RTOL / P_RTOL and fair = 4 (SURVEY
8d) -- not the 4 x / fair = 8 of test_batch_loop_gpu.py.  run() windows must be bitwise the solo handle's.
"""
import numpy as np
import pytest

from batch_edges_builders import (AB, CHAIN, COUNT, DT, PGEMM, PRELUDE_M, PRELUDE_STEPS, Q, R, RUN_CASES, TILES, V, WB,
                                  _swa, assert_symmetric, check_segment, drive, errors, prelude, run_case_id, run_loads,
                                  run_oracle, seg_id, seg_states)
from helpers import assert_close
from pyoracle import TEXTBOOK
from test_batch_gpu import _batch, _inputs, _solo

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1: run() windows
@pytest.mark.parametrize("case", RUN_CASES, ids=run_case_id)
def test_run_windows_equal_solo_lookahead_runs(gpu_required, monkeypatch, case):
    """test_batch_gpu.py's method at the sizes it leaves out: every instance bitwise the solo handle running look-ahead
    windows of the same pairs of updates; instance 0 against the oracle at 1e-5 / 1e-4, fair = 4."""
    monkeypatch.setenv("CSLAM_LOOKAHEAD", "1")
    loads, ctrl = run_loads(case)
    inputs = _inputs(loads, case.steps)
    states, traces, flags, nwin = _batch(loads, case.quirks, ctrl, inputs, case.steps, (case.steps,))
    assert flags == [0] * len(loads), flags
    assert nwin == (case.steps + 1) // 2
    for i, w in enumerate(loads):
        Xs, Ps, trs, fls = _solo(w, case.quirks, ctrl, inputs[i][0], inputs[i][1], case.steps)
        assert fls == 0
        assert np.array_equal(states[i][0], Xs), f"instance {i}: state differs from the solo run"
        assert np.array_equal(states[i][1], Ps), f"instance {i}: covariance differs from the solo run"
        assert traces[i] == trs
    assert not np.array_equal(states[0][0], states[1][0])
    ref = {}
    for dt in (np.float32, np.float64):
        X, P, codes = run_oracle(loads[0], ctrl, inputs[0][2], case.quirks, dt)
        assert codes == [0] * case.steps, codes
        ref[dt] = (X, P)
    for name, k in (("X", 0), ("P", 1)):
        hi = np.asarray(ref[np.float64][k])
        print(f"{run_case_id(case)} {name}: device error against f64 {float(np.abs(states[0][k] - hi).max()):.3e}, "
              f"CPU f32 {float(np.abs(ref[np.float32][k] - hi).max()):.3e}")
    assert_close("batch X", states[0][0], ref[np.float32][0], 1e-5, ref[np.float64][0])
    assert_close("batch P", states[0][1], ref[np.float32][1], 1e-4, ref[np.float64][1])


# ------------------------------------------------------------------------------------------------ 2: update() windows
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _segment_on_device(seg, monkeypatch):
    """prelude + one segment on a fresh batch -> the device's states after the segment; all of the segment's assertions"""
    import torch

    from conan_slam_amd import EKFBatch

    for key, val in seg.env:
        monkeypatch.setenv(key, val)  # (the options are read when the handle is created)
    states = seg_states(seg)
    pre = prelude(states)
    I, N = seg.I, seg.N
    b = EKFBatch(I, N, quirks=TEXTBOOK)
    try:
        for i, (X, P) in enumerate(states):
            b.set_state(i, X, P)
        # the prelude: two windows of 128 columns, both pending regions hold data afterwards
        pz = [_dev(np.concatenate([pre.obs[t][i][0].reshape(-1, order="F") for t in range(PRELUDE_STEPS)])) for i in range(I)]
        pi = [_dev(np.concatenate([pre.obs[t][i][1] for t in range(PRELUDE_STEPS)]).astype(np.int32)) for i in range(I)]
        torch.cuda.synchronize()
        b.run(PRELUDE_STEPS, [c[0] for c in pre.ctrl], [c[1] for c in pre.ctrl], Q, WB, DT, [t.data_ptr() for t in pz],
              [t.data_ptr() for t in pi], PRELUDE_M, R)
        # 1. the state the references start from is the batch's own
        starts = [b.get_state(i) for i in range(I)]
        assert b.factor_status() == [0] * I
        w0 = b.windows()
        assert w0 == PRELUDE_STEPS // 2
        hi = drive(seg, starts, np.float64)
        lo = drive(seg, starts, np.float32, hi.inputs)
        assert hi.codes == [0] * (2 * I) and lo.codes == [0] * (2 * I)
        inp = hi.inputs
        dz = {k: [_dev(Z.reshape(-1, order="F")) for Z, _ in inp[k]] for k in ("obs1", "obs2")}
        di = {k: [_dev(np.asarray(idf, np.int32)) for _, idf in inp[k]] for k in ("obs1", "obs2")}
        torch.cuda.synchronize()
        # 2. .. 5.
        b.update_device([t.data_ptr() for t in dz["obs1"]], [t.data_ptr() for t in di["obs1"]], seg.m_prev, R)
        for t in range(seg.h):
            b.predict(V, _swa(t), Q, WB, DT)
            b.observe_heading(inp["phi"][t], True)
        if seg.hold:
            b.predict(V, _swa(seg.h), Q, WB, DT)
        b.update_device([t.data_ptr() for t in dz["obs2"]], [t.data_ptr() for t in di["obs2"]], seg.m, R)
        # 6.
        got = [b.get_state(i) for i in range(I)]
        flags = b.factor_status()
        nwin = b.windows() - w0
        split = b.pgemm_split()
        n = b.n
    finally:
        b.close()
    eg, el = errors(got, hi.states), errors(lo.states, hi.states)
    print(f"{seg_id(seg)}: error against f64, device X {eg[0]:.3e} P {eg[1]:.3e}; CPU f32 X {el[0]:.3e} P {el[1]:.3e}")
    assert flags == [0] * I, flags
    assert nwin == 2
    T = (n + 127) // 128
    assert n == 3 + 2 * N and split == (I * T * (T + 1) // 2, 0), (n, split)  # (so few tiles: all whole, none as strips)
    for X, P in got:
        assert_symmetric(P)
    check_segment(seg_id(seg), got, lo.states, hi.states)
    return got


@pytest.mark.parametrize("seg", PGEMM, ids=seg_id)
def test_pgemm_class_and_zero_fill(gpu_required, monkeypatch, seg):
    _segment_on_device(seg, monkeypatch)


@pytest.mark.parametrize("seg", CHAIN, ids=seg_id)
def test_chain_and_wide_dispatch(gpu_required, monkeypatch, seg):
    _segment_on_device(seg, monkeypatch)


@pytest.mark.parametrize("seg", TILES, ids=seg_id)
def test_tile_boundaries(gpu_required, monkeypatch, seg):
    _segment_on_device(seg, monkeypatch)


def test_instance_count(gpu_required, monkeypatch):
    """(32, 33; 31) with 1, 2 and 3 instances: each against its references, and instance 0 -- fed identical inputs --
    bitwise the same in all three."""
    got = [_segment_on_device(seg, monkeypatch) for seg in COUNT]
    assert [len(g) for g in got] == [1, 2, 3]
    for g in got[1:]:
        assert np.array_equal(g[0][0], got[0][0][0]) and np.array_equal(g[0][1], got[0][0][1])
    assert not np.array_equal(got[2][0][0], got[2][1][0]) and not np.array_equal(got[2][1][0], got[2][2][0])


@pytest.mark.parametrize("seg", AB, ids=seg_id)
def test_ab_forms(gpu_required, monkeypatch, seg):
    _segment_on_device(seg, monkeypatch)
