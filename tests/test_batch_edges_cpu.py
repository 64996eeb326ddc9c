"""The input conditions of test_batch_edges_gpu.py, proved on the CPU oracle alone (no GPU), for every segment:
  * the oracle's return codes are all 0 in f32 and f64 (prelude included), under the quirk set used;
  * every heading step has S = P22 + R > 0 in every instance and both precisions (the 65-heading segment included);
  * the check can tell: each negative control -- the f64 drive re-run with ONE fault -- is rejected by the segment check
    in every family that claims it, and what the fault changes exceeds what the check lets pass (fair x the f32 oracle's
    own error against f64 + rtol x scale) in EVERY instance.  The smallest such ratio per family and control is printed
    and asserted to be above 1.
The faults: the last pending heading column is not applied to the map block; the last observation of the second update
is dropped; a stale column where the zero-fill should be (w w^T of the prelude's panel column added to the downdate);
the held predict applied after the update instead of inside it; the two rows of landmark 63 exchanged in the gain.
"""
import numpy as np
import pytest

from batch_edges_builders import (CONTROLS, FAIR, FAMILIES, R, RUN_CASES, SEGMENTS, applicable, check_segment,
                                  control_margin, drive, errors, np_update, pending_columns, pick_landmarks, prelude,
                                  run_case_id, run_loads, run_oracle, seg_id, seg_states, stale_columns,
                                  straddling_landmark)
from helpers import OracleState

_cache = {}


def _segment(seg):
    """(prelude, f64 drive, f32 drive) of a segment, computed once"""
    if seg not in _cache:
        pre = prelude(seg_states(seg))
        hi = drive(seg, pre.ends, np.float64)
        lo = drive(seg, pre.ends, np.float32, hi.inputs)
        _cache[seg] = (pre, hi, lo)
    return _cache[seg]


@pytest.mark.parametrize("seg", SEGMENTS, ids=seg_id)
def test_segment_inputs_are_healthy(seg):
    pre, hi, lo = _segment(seg)
    assert pre.codes == [0] * len(pre.codes), pre.codes
    assert hi.codes == [0] * (2 * seg.I) and lo.codes == [0] * (2 * seg.I), (hi.codes, lo.codes)
    if seg.h:
        assert len(hi.inputs["phi"]) == seg.h
        assert hi.s_min > 0 and lo.s_min > 0, (hi.s_min, lo.s_min)
    for key, m in (("obs1", seg.m_prev), ("obs2", seg.m)):
        for _, idf in hi.inputs[key]:
            assert len(set(idf.tolist())) == m == len(idf)
            assert straddling_landmark(seg.N) in idf
            assert m == 1 or seg.N in idf
    if seg.I > 1:  # different states and different observations
        assert not np.array_equal(pre.ends[0][0], pre.ends[1][0])
        assert not np.array_equal(hi.inputs["obs2"][0][1], hi.inputs["obs2"][1][1])
    for X, P in lo.states + hi.states:
        assert np.all(np.isfinite(X)) and np.all(np.isfinite(P))
    check_segment("f32 oracle", lo.states, lo.states, hi.states)  # (holds trivially: the check is well formed)
    ex, ep = errors(lo.states, hi.states)
    kp, cover = pending_columns(seg)
    print(f"{seg_id(seg)}: kp {kp} (class {cover}), min S {min(hi.s_min, lo.s_min):.3e}, "
          f"CPU f32 error against f64: X {ex:.3e}, P {ep:.3e}")


def test_numpy_update_is_the_oracles():
    """the restated textbook update behind the gain-row control agrees with the f64 oracle to rounding"""
    seg = SEGMENTS[0]
    pre, hi, _ = _segment(seg)
    X, P = pre.ends[0]
    a = OracleState(X.astype(np.float64), P.astype(np.float64), np.float64, 0)
    b = OracleState(X.astype(np.float64), P.astype(np.float64), np.float64, 0)
    Z, idf = hi.inputs["obs1"][0]
    assert a.update(Z.astype(np.float64), R.astype(np.float64), idf, True) == 0
    np_update(b, Z.astype(np.float64), idf)
    assert np.abs(a.x() - b.x()).max() <= 1e-10 * np.abs(a.x()).max()
    assert np.abs(a.p() - b.p()).max() <= 1e-10 * np.abs(a.p()).max()


@pytest.mark.parametrize("control", CONTROLS)
@pytest.mark.parametrize("family", FAMILIES)
def test_negative_control_is_rejected(family, control):
    segs = [s for s in SEGMENTS if s.family == family and applicable(s, control)]
    if not segs:
        assert control == "predict_after_update" and family != "chain"  # (only the chain family holds a predict)
        return
    worst = None
    for seg in segs:
        pre, hi, lo = _segment(seg)
        stale = stale_columns(seg, pre) if control == "stale_column" else None
        bad = drive(seg, pre.ends, np.float64, hi.inputs, fault=control, stale=stale)
        with pytest.raises(AssertionError):
            check_segment(control, bad.states, lo.states, hi.states)
        margin = control_margin(bad.states, lo.states, hi.states)
        assert margin > 1.0, (seg_id(seg), control, margin)
        if worst is None or margin < worst[0]:
            worst = (margin, seg_id(seg))
    ex, ep = (max(v) for v in zip(*(errors(_segment(s)[2].states, _segment(s)[1].states) for s in segs)))
    print(f"{family} / {control}: smallest change / (fair {FAIR:g} x e_ref + rtol x scale) = {worst[0]:.3g} at {worst[1]} "
          f"over {len(segs)} segments; CPU f32 error X {ex:.3e}, P {ep:.3e}")


def test_every_family_claims_every_control_it_can():
    for family in FAMILIES:
        claimed = {c for c in CONTROLS for s in SEGMENTS if s.family == family and applicable(s, c)}
        expected = set(CONTROLS) - (set() if family == "chain" else {"predict_after_update"})
        assert claimed == expected, (family, claimed)


@pytest.mark.parametrize("case", RUN_CASES, ids=run_case_id)
def test_run_window_inputs_are_healthy(case):
    """the run() cases: oracle codes 0 in f32 and f64, landmark 63 and the last one in every observed set"""
    loads, ctrl = run_loads(case)
    for w in loads:
        obs = []
        for t in range(case.steps):
            w.controls(t)
            obs.append(w.observations(t))
        for Z, idf in obs:
            assert len(set(idf.tolist())) == case.m
            assert straddling_landmark(case.N) in idf and case.N in idf
            if case.same:
                assert set(idf.tolist()) == set(obs[0][1].tolist())
        for dt in (np.float32, np.float64):
            X, P, codes = run_oracle(w, ctrl, obs, case.quirks, dt)
            assert codes == [0] * case.steps, (dt, codes)
            assert np.all(np.isfinite(X)) and np.all(np.isfinite(P))
    assert not np.array_equal(loads[0].X0, loads[1].X0)


def test_pick_landmarks_puts_the_straddling_and_last_landmarks_first():
    for N in (62, 63, 70, 126, 127):
        for m in (1, 8, 9, 32):
            idf = pick_landmarks(N, m, seed=N + m)
            assert len(set(idf.tolist())) == m and idf.min() >= 1 and idf.max() <= N
            assert straddling_landmark(N) in idf
