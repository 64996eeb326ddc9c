"""CPU checks of tests/pose_queue_ref.py: the reference against the oracle's dense Joseph form, the constant c of the
check (measured from the CPU oracle of each dtype), and the negative controls -- a heading column that never reaches
the map block and swapped controls must be rejected by the very check the GPU tests rely on (DESIGN.md 3 "Pose queue at
its limits").  Run with -s to see the measured figures."""
import numpy as np
import pytest

import pose_queue_ref as pq
from helpers import P_RTOL, X_RTOL, OracleState, assert_close
from pyoracle import REF_EXACT, Oracle

F32, F64 = pq.F32, pq.F64
MIN_REJECT = 4.0


def _hi_work(dtype):
    return np.float64 if np.dtype(dtype) == F32 else np.longdouble


def _single_runs():
    """(name, dtype, X0, P0, script, quirks) of every run that a GPU test checks with `check`"""
    for case in pq.SINGLE_CASES:
        for dt in case.dtypes:
            X0, P0, steps = case.make(dt)
            yield case.name, dt, X0, P0, steps, case.quirks
    for name, N, count in pq.BATCH_CASES:
        states, steps = pq.batch_common_script(name, N, count)
        for i, (X0, P0) in enumerate(states):
            yield f"{name}[{i}]", F32, X0, P0, steps, REF_EXACT
    name, N, count = pq.BATCH_RING
    states, scripts = pq.batch_each_scripts(name, N, count)
    for i, (X0, P0) in enumerate(states):
        yield f"{name}[{i}]", F32, X0, P0, scripts[i], REF_EXACT


@pytest.fixture(scope="module")
def runs():
    return list(_single_runs())


@pytest.fixture(scope="module")
def between():
    """the control-step runs between the updates, started from the state the CPU oracle of the dtype holds there (it
    stands in for the handle): (name, dtype, Xa, Pa, run, panels pending under set_deferred)"""
    out = []
    for dt in (F32, F64):
        plan = pq.between_plan(dt)
        o = OracleState(plan["X0"], plan["P0"], dt, pq.BETWEEN_QUIRKS)
        for u in range(2):
            assert o.update(plan["Z"][u], pq.BETWEEN_R.astype(dt), pq.BETWEEN_IDF, True) == 0
            out.append((f"between-run{pq.BETWEEN_RUNS[u]}", dt, o.x(), o.p(), plan["runs"][u], plan["pending"][u]))
            X, P = pq.oracle_run(o.x(), o.p(), plan["runs"][u], dt, pq.BETWEEN_QUIRKS)
            o.X[:], o.P[:, :] = X, P
    return out


def test_scripts_reach_the_limits(runs):
    """the cases are the ones the branches need: queue depth, region capacity, ring slots, step kinds"""
    by = {name: pq.replay(X0, P0, steps, pq.heading_R(dt), q) for name, dt, X0, P0, steps, q in runs if dt == F32}
    assert [by[f"run{L}-N62"]["steps"] for L in pq.RUN_LENGTHS] == list(pq.RUN_LENGTHS)
    assert by["run9-N62"]["steps"] == pq.POSE_SEQ_MAX + 1 and by["run131-N62"]["headings"] == pq.WCAP + 3
    assert by["kinds-ref_exact"]["steps"] == 20 and by["kinds-ref_exact"]["headings"] == 15
    assert by["empty-N0"]["steps"] == 20
    assert -(-pq.BATCH_RING[2] // pq.POSE_SEQ_MAX) > pq.CTL_SLOTS + 1  # the control ring wraps
    ref = pq.replay(*pq.SECOND_CROSSING.make(F64)[:2], pq.SECOND_CROSSING.make(F64)[2], pq.heading_R(F64))
    assert ref["headings"] > 2 * pq.WCAP
    for N in (62, 63, 64, 126, 127, 190):
        rows = pq.spike_rows(3 + 2 * N)
        assert rows[0] == 3 and rows[-1] == 2 + 2 * N
        assert all(e - 1 in rows and e in rows for e in range(128, 3 + 2 * N, 128))


def test_every_column_carries_weight(runs, between):
    """P22 < R / 100 and S > 0 throughout, and no map row is uncorrelated with the heading at the start: every heading
    column is about as heavy as the first, on every row"""
    for name, dt, X0, P0, steps, q in runs + [b[:5] + (pq.BETWEEN_QUIRKS,) for b in between]:
        R = pq.heading_R(dt)
        ref = pq.replay(X0, P0, steps, R, q)
        assert max(ref["P22"]) < R / 100, (name, max(ref["P22"]), R)
        assert min(ref["S"]) > 0, name
        if X0.shape[0] > 3 and not name.startswith("between"):
            assert np.abs(np.asarray(P0, np.float64)[3:, 2]).min() > 0, name
        if ref["headings"] > pq.WCAP and dt == F32:
            # every map row is moved by columns on both sides of the region switch
            cut = [k for k, s in enumerate(steps) if s[0] == "heading"][pq.WCAP - 1] + 1
            first = pq.replay(X0, P0, steps[:cut], R, q)
            d0, d1, d2 = (np.diag(np.asarray(M, np.float64))[3:] for M in (P0, first["P"], ref["P"]))
            assert first["headings"] == pq.WCAP and np.all(d1 < d0) and np.all(d2 < d1), name


def test_replay_matches_the_dense_joseph_form():
    """20 mixed steps at N = 5: the rank-1 replay against the oracle's n^3 Joseph form (structured=False), f64"""
    for quirks in (REF_EXACT, pq.TEXTBOOK):
        X0, P0 = pq.scenario(5, F64, 7)
        steps = pq.step_kinds_script(X0, P0, F64, quirks)
        ref = pq.replay(X0, P0, steps, pq.heading_R(F64), quirks)
        assert ref["steps"] == 20
        o = Oracle(np.float64, quirks)
        X, P = X0.copy(), P0.copy(order="F")
        for s in steps:
            if s[0] == "predict":
                o.predict(X, P, X.shape[0], s[1], s[2], np.asfortranarray(s[3]), s[4], s[5])
            elif s[0] == "heading":
                o.observe_heading(X, P, X.shape[0], s[1], True, structured=False)
        assert_close("X", ref["X"], X, X_RTOL[F64])
        assert_close("P", ref["P"], P, P_RTOL[F64])
        # ... and element-wise: the Joseph form passes the check as an f64 engine would have to
        pq.check(X, P, ref, F64, "dense Joseph")


def test_long_double_replay_is_the_same_recursion():
    """the numpy predict of the long-double replay against the f64 oracle's (which the f64 replay calls)"""
    X0, P0 = pq.scenario(64, F64, 9)
    for quirks in (REF_EXACT, pq.TEXTBOOK):
        steps = pq.step_kinds_script(X0, P0, F64, quirks)
        a = pq.replay(X0, P0, steps, pq.heading_R(F64), quirks)
        b = pq.replay(X0, P0, steps, pq.heading_R(F64), quirks, work=np.longdouble)
        rx, rp = pq.ratios(a["X"], a["P"], b, F64, c=0.0)
        assert rx <= 1.0 and rp <= 1.0, (rx, rp)


def test_oracle_passes_and_c_has_its_margin(runs, between):
    """The CPU oracle of each dtype (heading in its rank-structured form) passes `check` on every GPU case, and C_MARGIN
    is 4 x the worst constant it needs against the reference of the next precision up -- no less, and not idly more."""
    worst = {F32: 0.0, F64: 0.0}
    for name, dt, X0, P0, steps, q in runs:
        ref = pq.replay(X0, P0, steps, pq.heading_R(dt), q, work=_hi_work(dt))
        X, P = pq.oracle_run(X0, P0, steps, dt, q)
        c = pq.needed_c(X, P, ref, dt)
        rx, rp = pq.check(X, P, ref, dt, name)
        print(f"{name:24s} {dt.name} steps {ref['steps']:3d}: oracle needs c = {c:5.2f}, error / bound X {rx:.3f} P {rp:.3f}")
        worst[dt] = max(worst[dt], c)
    for name, dt, Xa, Pa, run, d in between:
        for dd in (None, d):
            ref = pq.between_ref(Xa, Pa, run, dt, dd)
            if dt == F64:  # (the long-double replay, with the bookkeeping of between_ref)
                hi = pq.replay(Xa, Pa, run, pq.heading_R(dt), pq.BETWEEN_QUIRKS, work=np.longdouble)
                ref["X"], ref["P"] = hi["X"], hi["P"]
            X, P = pq.oracle_run(Xa, Pa, run, dt, pq.BETWEEN_QUIRKS)
            c = pq.needed_c(X, P, ref, dt)
            pq.check(X, P, ref, dt, name)
            print(f"{name:24s} {dt.name} steps {ref['steps']:3d}: oracle needs c = {c:5.2f}")
            worst[dt] = max(worst[dt], c)
    # the augment behind the empty-map run
    for dt in (F32, F64):
        X0, P0, steps = pq.EMPTY_CASE.make(dt)
        mid = pq.replay(X0, P0, steps, pq.heading_R(dt))
        tail = pq.empty_map_tail(mid["X"], mid["P"], dt)
        ref = pq.replay(X0, P0, steps + tail, pq.heading_R(dt))
        X, P = pq.oracle_run(X0, P0, steps + tail, dt)
        assert X.shape[0] == 5
        c = pq.needed_c(X, P, ref, dt)
        pq.check(X, P, ref, dt, "empty map + augment")
        print(f"empty map + augment      {dt.name} steps {ref['steps']:3d}: oracle needs c = {c:5.2f}")
        worst[dt] = max(worst[dt], c)
    for dt in (F32, F64):
        print(f"{dt.name}: worst c the oracle needs {worst[dt]:.3f}, C_MARGIN {pq.C_MARGIN[dt]}")
        assert 4.0 * worst[dt] <= pq.C_MARGIN[dt] <= 4.0 * worst[dt] + 1.0, (dt, worst[dt])


def _reject(name, dt, make_ref, columns=None):
    ref = make_ref(None)
    low = np.inf
    for j in pq.drop_columns(ref["headings"]) if columns is None else columns:
        bad = make_ref(j)
        rp = pq.ratios(bad["X"], bad["P"], ref, dt)[1]
        with pytest.raises(AssertionError):
            pq.check(bad["X"], bad["P"], ref, dt, name)
        assert rp >= MIN_REJECT, f"{name}: losing heading column {j} moves P by {rp:.2f} x the bound only"
        low = min(low, rp)
    return low


def test_a_lost_heading_column_is_rejected(runs, between):
    """For every GPU case and every heading column next to a launch or region boundary: the f64 replay without that
    column's downdate of the map block misses the check by a factor >= 4, at the tolerance of the dtype the case runs
    in (f32 wherever it runs in f32).  The empty-map run itself has no map block to lose a column from; the heading
    column behind its augment has, and is judged here like the others."""
    lowest = np.inf
    for name, dt, X0, P0, steps, q in runs:
        if X0.shape[0] == 3 or (dt == F64 and name != pq.SECOND_CROSSING.name):
            continue  # (no map block: see below; f64: the looser f32 bound has been shown to reject)
        low = _reject(name, dt, lambda j: pq.replay(X0, P0, steps, pq.heading_R(dt), q, drop=j))
        print(f"{name:24s} {dt.name}: smallest error / bound of a lost column {low:.1f}")
        lowest = min(lowest, low)
    for name, dt, Xa, Pa, run, d in between:
        if dt == F64:
            continue
        for dd in (None, d):
            low = _reject(name, dt, lambda j: pq.between_ref(Xa, Pa, run, dt, dd, drop=j))
            print(f"{name:24s} {dt.name} {'deferred' if dd is not None else 'immediate'}: smallest {low:.1f}")
            lowest = min(lowest, low)
    X0, P0, steps = pq.EMPTY_CASE.make(F32)
    mid = pq.replay(X0, P0, steps, pq.heading_R(F32))
    steps = steps + pq.empty_map_tail(mid["X"], mid["P"], F32)
    low = _reject("empty map + augment", F32, lambda j: pq.replay(X0, P0, steps, pq.heading_R(F32), drop=j),
                  columns=[mid["headings"]])  # (the one heading column that meets a map block)
    print(f"empty map + augment      float32: error / bound of the lost column {low:.1f}")
    lowest = min(lowest, low)
    print(f"smallest reject ratio: {lowest:.1f}")
    assert lowest >= MIN_REJECT


def test_swapped_controls_are_rejected():
    """predict_each: the replay with two steps' controls exchanged (neighbours; the same slot position one launch and one
    whole ring later), or with the other instance's controls at one step, misses the check on X by a factor >= 4"""
    name, N, count = pq.BATCH_RING
    states, scripts = pq.batch_each_scripts(name, N, count)
    R = pq.heading_R(F32)
    pred = [[k for k, s in enumerate(sc) if s[0] == "predict"] for sc in scripts]
    for k in range(count):  # v differs by >= 1 % between instances and between steps
        v = [scripts[i][pred[i][k]][1] for i in range(pq.BATCH_I)]
        assert abs(v[0] - v[1]) >= 0.01 * max(v)
        for i in range(pq.BATCH_I):
            others = [scripts[i][pred[i][l]][1] for l in range(count) if l != k]
            assert min(abs(v[i] - o) for o in others) >= 0.01 * max(v[i], max(others))
    lowest = np.inf
    for i, (X0, P0) in enumerate(states):
        ref = pq.replay(X0, P0, scripts[i], R)
        ring = pq.POSE_SEQ_MAX * pq.CTL_SLOTS
        for a, b in ((3, 4), (7, 8), (2, 2 + pq.POSE_SEQ_MAX), (5, 5 + ring), (count - 1, count - 1 - ring)):
            bad = list(scripts[i])
            bad[pred[i][a]], bad[pred[i][b]] = bad[pred[i][b]], bad[pred[i][a]]
            got = pq.replay(X0, P0, bad, R)
            rx = pq.ratios(got["X"], got["P"], ref, F32)[0]
            assert rx >= MIN_REJECT, (i, a, b, rx)
            lowest = min(lowest, rx)
        for k in (0, 8, count - 1):  # the other instance's controls
            bad = list(scripts[i])
            bad[pred[i][k]] = scripts[1 - i][pred[1 - i][k]]
            got = pq.replay(X0, P0, bad, R)
            rx = pq.ratios(got["X"], got["P"], ref, F32)[0]
            assert rx >= MIN_REJECT, (i, k, rx)
            lowest = min(lowest, rx)
    print(f"smallest error / bound on X of exchanged controls: {lowest:.1f}")
