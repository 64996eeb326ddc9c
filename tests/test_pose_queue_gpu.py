"""Long runs of control steps through the pose queue of both engines, to the limits only such a run reaches: the queue
depth kPoseSeqMax, the pending-column capacity of a region (wcap / kWcols = 128) with the region switch behind it, the
batched engine's control ring, and the workgroup that rewrites the pose (DESIGN.md 3 "Pose queue at its limits").

Every case is one handle, one short script and one comparison with the float64 replay of tests/pose_queue_ref.py through
its element-wise `check`; test_pose_queue_cpu.py shows on the CPU that this check rejects a single lost heading column
and exchanged controls in every one of these cases.  Run with -s to see error / bound of each case.
"""
import numpy as np
import pytest

import pose_queue_ref as pq
from helpers import P_RTOL, X_RTOL, OracleState, assert_close
from pyoracle import REF_EXACT

pytestmark = pytest.mark.gpu

F32, F64 = pq.F32, pq.F64
DTYPES = [F32, F64]


def _play(eng, steps):
    for s in steps:
        if s[0] == "predict":
            eng.predict(s[1], s[2], s[3], s[4], s[5])
        elif s[0] == "heading":
            eng.observe_heading(s[1], True)
        elif s[0] == "heading_off":
            eng.observe_heading(s[1], False)
        else:
            eng.augment(np.reshape(s[1], (2, 1)), s[2])


def _handle(X0, P0, dtype, quirks=REF_EXACT, capacity=None, deferred=0):
    from conan_slam_amd import EKF

    eng = EKF(max((X0.shape[0] - 3) // 2 if capacity is None else capacity, 1), dtype=dtype, quirks=quirks)
    eng.set_state(X0, P0)
    if deferred:
        eng.set_deferred(deferred)
    return eng


def _run(X0, P0, steps, dtype, quirks=REF_EXACT, capacity=None):
    eng = _handle(X0, P0, dtype, quirks, capacity)
    _play(eng, steps)
    X, P = eng.get_state()
    status = eng.factor_status()
    eng.close()
    assert status == 0, status
    return X, P


def _report(name, dtype, r):
    print(f"{name:24s} {np.dtype(dtype).name}: error / bound X {r[0]:.3f} P {r[1]:.3f}")


def _case(case, dtype):
    X0, P0, steps = case.make(dtype)
    ref = pq.replay(X0, P0, steps, pq.heading_R(dtype), case.quirks)
    X, P = _run(X0, P0, steps, dtype, case.quirks)
    _report(case.name, dtype, pq.check(X, P, ref, dtype, case.name))
    return X, P, ref


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("case", pq.RUN_CASES, ids=repr)
def test_run_lengths(gpu_required, case, dtype):
    """N = 62 (one workgroup): runs of predict + heading of 1, 7, 8 (one full queue), 9 and 17 (one and two launches in the
    middle of the run), 16, and 131: the 129th heading column flushes 128 heading columns alone and lands, with two more,
    in the other region."""
    _case(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("case", pq.EDGE_CASES, ids=repr)
def test_state_edges(gpu_required, case, dtype):
    """Run length 17 at n = 129, 131 (rows [n, 256) of a heading column are zeros), 255, 257 (one workgroup, then two: the
    last to take a ticket rewrites the pose the others read at their start), 383 (a half-occupied second workgroup), and
    131 steps at n = 257: two workgroups take tickets over 17 launches and one region switch."""
    _case(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("case", pq.KIND_CASES, ids=repr)
def test_step_kinds(gpu_required, case, dtype):
    """One run of 20 steps at N = 64 with predict-only steps (predicts in a row), heading-only steps, an unused heading
    between a predict and its heading (the predict stays held) and a predict left held at the end, which get_state
    resolves; REF_EXACT (predict width n - 4) and TEXTBOOK."""
    _case(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.name)
def test_empty_map(gpu_required, dtype):
    """n = 3: 20 steps through the scratch column.  None of them may count as a pending column: a feature augmented
    behind them, and one more control step, agree with the replay.  The feature is 300 m away with a tiny R, so that the
    one heading column behind the augment moves the new block by 600 x the f32 bound (test_pose_queue_cpu.py)."""
    case = pq.EMPTY_CASE
    _case(case, dtype)
    X0, P0, steps = case.make(dtype)
    mid = pq.replay(X0, P0, steps, pq.heading_R(dtype))
    tail = pq.empty_map_tail(mid["X"], mid["P"], dtype)
    ref = pq.replay(X0, P0, steps + tail, pq.heading_R(dtype))
    X, P = _run(X0, P0, steps + tail, dtype, capacity=1)
    assert X.shape[0] == 5
    _report("empty map + augment", dtype, pq.check(X, P, ref, dtype, "empty map + augment"))


def test_second_crossing(gpu_required):
    """260 control steps at N = 62 in f64: both regions are used a second time, with the sign words and the heading-column
    count of a region that held heading columns a flush ago."""
    _case(pq.SECOND_CROSSING, F64)


@pytest.mark.parametrize("deferred", [0, 64, 128], ids=["immediate", "deferred64", "deferred128"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.name)
def test_between_updates(gpu_required, dtype, deferred):
    """N = 127, m = 9 (k = 18, landmarks 63 and 127 among them): update, 12 control steps, update, 131 control steps,
    update.  Immediate: the second run flushes 128 heading columns alone, and the last update's panel is appended behind
    the 3 heading columns in the other region, its gather corrected with them.  set_deferred: both earlier panels and the
    first run's columns are still pending when the second run starts, 80 heading columns fill the region and 51 land in
    the other one; a window of 64 applies those ahead of the last update, a window of 128 appends its panel behind that
    odd number of heading columns.  Each control-step run is checked by `check` on a twin handle that stops behind it,
    against the replay from the state a twin read back behind the update in front; the end against the CPU oracle with
    the project's fairness rule."""
    plan = pq.between_plan(dtype)
    R = pq.BETWEEN_R.astype(dtype)

    def twin(updates, runs):
        eng = _handle(plan["X0"], plan["P0"], dtype, pq.BETWEEN_QUIRKS, deferred=deferred)
        for u in range(updates):
            eng.update(plan["Z"][u], R, pq.BETWEEN_IDF, True)
            if u < runs:
                _play(eng, plan["runs"][u])
        X, P = eng.get_state()
        status = eng.factor_status()
        eng.close()
        assert status == 0, status
        return X, P

    for u in range(2):
        Xa, Pa = twin(u + 1, u)
        Xb, Pb = twin(u + 1, u + 1)
        # One `pending` list serves both windows: it rests on queue_step() flushing heading columns at wcap only, never
        # at the deferral window, so that neither window applies a panel between the start of the script and the end of
        # run u.  Were queue_step() to flush at the window, fewer panels would be pending than the list says and the bound
        # would be wider than it needs to be, not wrong: the cases would then want a list per window.
        ref = pq.between_ref(Xa, Pa, plan["runs"][u], dtype, plan["pending"][u] if deferred else None)
        name = f"between-run{pq.BETWEEN_RUNS[u]}"
        _report(name, dtype, pq.check(Xb, Pb, ref, dtype, name))
    X, P = twin(3, 2)
    cpu = OracleState(plan["X0"], plan["P0"], dtype, pq.BETWEEN_QUIRKS)
    for u in range(3):
        assert cpu.update(plan["Z"][u], R, pq.BETWEEN_IDF, True) == 0
        if u < 2:
            Xc, Pc = pq.oracle_run(cpu.x(), cpu.p(), plan["runs"][u], dtype, pq.BETWEEN_QUIRKS)
            cpu.X[:], cpu.P[:, :] = Xc, Pc
    hi = plan["hi"]
    assert_close("X", X, cpu.x(), X_RTOL[dtype], hi=hi.x() if dtype == F32 else None)
    assert_close("P", P, cpu.p(), P_RTOL[dtype], hi=hi.p() if dtype == F32 else None)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.name)
def test_launch_grouping(gpu_required, dtype, monkeypatch):
    """The 131 steps at N = 127 with CSLAM_FUSE_PREDICT=0: every predict and every heading is a launch of its own.  The
    arithmetic of a step is the same code and the flushes fall on the same columns, so X and P are bitwise those of the
    queued run."""
    case = pq.EDGE_CASES[-1]
    assert case.name == "run131-N127"
    Xq, Pq, ref = _case(case, dtype)
    X0, P0, steps = case.make(dtype)
    monkeypatch.setenv("CSLAM_FUSE_PREDICT", "0")
    X1, P1 = _run(X0, P0, steps, dtype, case.quirks)
    monkeypatch.delenv("CSLAM_FUSE_PREDICT")
    _report("one launch per call", dtype, pq.check(X1, P1, ref, dtype, "one launch per call"))
    assert np.array_equal(Xq, X1) and np.array_equal(Pq, P1)


# ---------------------------------------------------------------------------------------------------- the batched engine
def _batch_run(states, scripts, each):
    from conan_slam_amd import EKFBatch

    N = (states[0][0].shape[0] - 3) // 2
    b = EKFBatch(len(states), N)
    for i, (X0, P0) in enumerate(states):
        b.set_state(i, X0, P0)
    for k, s in enumerate(scripts[0]):
        if s[0] == "predict":
            if each:
                b.predict_each([sc[k][1] for sc in scripts], [sc[k][2] for sc in scripts], s[3].astype(np.float32), s[4],
                               s[5])
            else:
                b.predict(s[1], s[2], s[3].astype(np.float32), s[4], s[5])
        else:
            assert all(sc[k] == s for sc in scripts)  # (the heading observation is common to the instances)
            b.observe_heading(s[1], True)
    out = [b.get_state(i) for i in range(len(states))]
    status = b.factor_status()
    b.close()
    assert status == [0] * len(states), status
    return out


@pytest.mark.parametrize("spec", pq.BATCH_CASES, ids=lambda s: s[0])
def test_batch_run_lengths(gpu_required, spec):
    """EKFBatch, I = 2 instances with their own maps: runs of 9 (kPoseSeqMax) and 131 (kWcols, region switch) at N = 62,
    and 17 at N = 127 (grid (2, I)); every instance against its own replay."""
    name, N, count = spec
    states, steps = pq.batch_common_script(name, N, count)
    got = _batch_run(states, [steps] * len(states), each=False)
    for i, ((X0, P0), (X, P)) in enumerate(zip(states, got)):
        ref = pq.replay(X0, P0, steps, pq.heading_R(F32))
        _report(f"{name}[{i}]", F32, pq.check(X, P, ref, F32, f"{name}[{i}]"))


def test_batch_control_ring(gpu_required):
    """predict_each over 41 steps with controls that differ per instance and per step: six queue launches, so the ring of
    four control slots wraps and a slot is reused behind its event.  Every instance against the replay with ITS
    controls (test_pose_queue_cpu.py: a control from another step, slot or instance misses the check on X)."""
    name, N, count = pq.BATCH_RING
    states, scripts = pq.batch_each_scripts(name, N, count)
    got = _batch_run(states, scripts, each=True)
    for i, ((X0, P0), (X, P)) in enumerate(zip(states, got)):
        ref = pq.replay(X0, P0, scripts[i], pq.heading_R(F32))
        _report(f"{name}[{i}]", F32, pq.check(X, P, ref, F32, f"{name}[{i}]"))
