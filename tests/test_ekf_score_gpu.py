"""The score and the trajectory log of the single EKF handle on the device (cslam_ekf_score*, cslam_ekf_get_pose;
EKF.score / scores / pose), f32 and f64.

The method of tests/test_score_gpu.py: after every score call the test reads pose() and landmarks() of the same handle --
the reads a host scorer makes, which leave the run alone -- and feeds them to the f64 restatement
(tests/ekf_score_ref.py over tests/score_ref.py).  Device and restatement start from the same bits and work in f64:
  - the counts (valid, bad, inside the gate) are EXACT;
  - every sum and series value lies within score_ref's rounding bounds, and those bounds reject a relative 1e-6;
  - the track's pose is bitwise pose()'s x, its n exact, its trace within 2 (n - 1) u sum |d| of the f64 sum of the pose
    diagonal and the landmarks() diagonals (u = 2^-53), a bound that rejects a relative 1e-9.
Scoring never perturbs the run (bitwise against the same run unscored, same P-GEMM launches and look-ahead windows) and
is reproducible bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import score_ref as sr
from ekf_score_ref import SingleRef, trace_ref, trace_terms
from helpers import make_obs, make_scenario
from pyoracle import TEXTBOOK

pytestmark = pytest.mark.gpu

Q = np.diag([0.18, 6e-4])
R = np.diag([0.08, 0.0024])
WB, DT = 73.0, 0.01
DTYPES = [np.float32, np.float64]
XV = (1.05, -2.1, 0.31)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ids(N, m, rng, must=()):
    ids = list(must) + [int(f) for f in rng.permutation(N) + 1 if int(f) not in must]
    return np.array(ids[:m], dtype=np.int32)


def _engine(monkeypatch, cap, dtype, env=None, deferred=0, sync=False):
    from conan_slam_amd import EKF

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    e = EKF(cap, dtype=dtype, quirks=TEXTBOOK, sync_mode=sync)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if deferred:
        e.set_deferred(deferred)
    return e


class Scored:
    """An EKF handle with N landmarks (room for `extra` more), a truth near the estimate, and the restatement fed from
    pose() / landmarks() after every score call."""

    def __init__(self, monkeypatch, N, dtype, env=None, deferred=128, sync=False, extra=2, seed=0, capacity=16, state=None,
                 truth_count=None, reset=True):
        self.N, self.dtype = N, np.dtype(dtype)
        self.X0, P = state if state is not None else make_scenario(N, self.dtype, seed=seed, corr=0.1)
        self.e = _engine(monkeypatch, N + extra, dtype, env, 0, sync)
        self.e.set_state(self.X0, P)
        if deferred:
            self.e.set_deferred(deferred)
        self.rng = np.random.default_rng(1000 + seed)
        # the true map: the initial estimate displaced by about one standard deviation; the new features' truth is anywhere
        self.truth = np.concatenate([self.X0[3:].astype(np.float64).reshape(N, 2) + self.rng.normal(size=(N, 2)),
                                     self.rng.uniform(-300, 300, size=(extra, 2))])
        if truth_count is not None:
            self.truth = self.truth[:truth_count]
        if reset:
            self.e.score_reset(capacity)
        self.e.score_set_truth(self.truth)
        self.ref = SingleRef(capacity if reset else 0)
        self.k = 0

    def score(self, xv_true=XV, with_map=True):
        self.e.score(xv_true, with_map)
        return self.ref.add(self.e, self.truth, xv_true, with_map)

    def predict(self, swa=0.01):
        self.e.predict(83.33, swa, Q.astype(self.dtype), WB, DT)

    def steps(self, count):
        """control steps with a heading observation each: in deferred mode every one leaves a rank-1 column pending"""
        for _ in range(count):
            self.predict(0.01 * (self.k % 3 - 1))
            self.e.observe_heading(float(self.X0[2]) + 1e-3 * (self.k + 1), True)
            self.k += 1

    def update(self, m, must=()):
        """m of the first N features (the initial ones: their observations come from the initial estimate)"""
        idf = _ids(self.N, m, self.rng, must=must)
        self.k += 1
        self.e.update(make_obs(self.X0, idf, self.dtype, seed=self.k), R.astype(self.dtype), idf, True)

    def augment(self):
        self.e.augment(np.asfortranarray(np.array([[300.0, 410.0], [0.2, -0.4]], self.dtype)), R.astype(self.dtype))

    def finish(self, tag):
        out = self.e.scores()
        self.ref.check(out, tag)
        self.e.close()
        return out


# ------------------------------------------------------------------------------------------------ 1. values

VALUES = [(N, dt, "lower") for N in (1, 255, 256, 257) for dt in DTYPES] + [(257, dt, "full") for dt in DTYPES]


@pytest.mark.parametrize("N,dtype,storage", VALUES, ids=[f"N{N}-{np.dtype(d).name}-{s}" for N, d, s in VALUES])
def test_values(gpu_required, monkeypatch, N, dtype, storage):
    """Landmark counts at the workgroup edges (256 lanes), feature 63 with fx = 127 across two row tiles; scored with
    nothing pending, with update panels pending, with heading columns pending as well, after a flush, and right after an
    augment of 2 (the new rows have nothing pending)."""
    s = Scored(monkeypatch, N, dtype, env={"CSLAM_LOOKAHEAD": "0", "CSLAM_STORAGE": storage}, seed=10 * N)
    must = tuple(dict.fromkeys(f for f in (1, 63, N) if f <= N))
    s.score()                                   # kp = 0
    s.predict()
    s.update(min(5, N), must=must[: min(5, N)])
    s.score()                                   # the update's panel pending
    s.steps(3)
    s.score()                                   # ... and heading columns
    s.e.flush()
    _, pvv, _, pll = s.score()                  # kp = 0 after a flush
    flushed = s.e.scores()[2][3, 3]
    d = trace_terms(pvv, pll)
    assert abs(flushed - s.e.trace()) <= trace_ref(d)[1], "the track's trace after a flush is not EKF.trace()'s sum"
    s.predict()
    s.update(min(7, N), must=must[: min(7, N)])
    s.augment()
    assert s.e.n == 3 + 2 * (N + 2)
    s.score()                                   # right after an augment, a panel pending below
    totals, series, track, calls = s.finish(f"N={N} {np.dtype(dtype).name} {storage}")
    assert calls == 5 and series.shape == (5, 4) and track.shape == (5, 5)
    assert totals[sr.POSE_N] == 5 and totals[sr.LM_BAD] == 0 and totals[sr.LM_N] + totals[sr.LM_BAD] == 4 * N + N + 2
    assert track[:, 4].tolist() == [3 + 2 * N] * 4 + [3 + 2 * (N + 2)]


# ------------------------------------------------------------------------------------------------ 2. partial truth, with_map = 0


def test_partial_truth_and_without_the_map(gpu_required, monkeypatch):
    """N = 257 with 200 truth rows: 200 landmarks scored per call, the trace still covers all 257.  with_map = 0 leaves the
    landmark totals alone, series fields 2 and 3 NaN and the track's trace NaN."""
    N = 257
    s = Scored(monkeypatch, N, np.float32, env={"CSLAM_LOOKAHEAD": "0"}, seed=3, truth_count=200)
    s.predict()
    s.update(5, must=(1, 63, N))
    s.score()
    before = s.e.scores()
    assert before[0][sr.LM_N] + before[0][sr.LM_BAD] == 200
    _, pvv, _, pll = s.score(with_map=False)
    after = s.e.scores()
    assert _bits_equal(before[0][sr.LM_N:], after[0][sr.LM_N:]), "with_map = 0 touched the landmark totals"
    assert after[0][sr.POSE_N] == 2 and np.isnan(after[1][1, 2:]).all() and np.isfinite(after[1][1, :2]).all()
    assert np.isnan(after[2][1, 3]) and after[2][1, 4] == 3 + 2 * N
    # the first record's trace is the sum over all 257 landmarks (nothing has moved between the two calls)
    full, b = trace_ref(trace_terms(pvv, pll))
    assert pll.shape[0] == N and abs(after[2][0, 3] - full) <= b
    s.score()
    totals = s.finish("partial truth")[0]
    assert totals[sr.LM_N] + totals[sr.LM_BAD] == 400


# ------------------------------------------------------------------------------------------------ 3. negative heading column


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_negative_heading_column(gpu_required, monkeypatch, dtype):
    """set_state with P22 + R < 0: the heading column is stored with S < 0 (sign word set) and enters P with the opposite
    sign.  The sign words must reach the score kernel: the blocks it scores are the ones landmarks() returns."""
    N = 40
    X, P = make_scenario(N, np.dtype(dtype), seed=9, corr=0.1)
    P = P.astype(np.float64)
    P[2, 2] = -0.5
    P = np.asfortranarray(P.astype(dtype))
    s = Scored(monkeypatch, N, dtype, state=(X, P), env={"CSLAM_LOOKAHEAD": "0"}, extra=0, seed=9)
    s.e.observe_heading(float(X[2]) + 1e-3, True)
    _, _, _, pll = s.score()
    fx = 3 + 2 * np.arange(N)
    # the column really is there, with the positive sign: the blocks lie above the stored Ps
    assert np.all(pll[:, 0, 0] >= P[fx, fx] - 1e-3 * np.abs(P[fx, fx])) and np.any(pll[:, 0, 0] > P[fx, fx])
    totals = s.finish("negative heading column")[0]
    assert totals[sr.LM_N] + totals[sr.LM_BAD] == N


# ------------------------------------------------------------------------------------------------ 4. heading wrap


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_heading_wrap_on_the_device(gpu_required, monkeypatch, dtype):
    """True phi = pi - 0.01, estimate -pi + 0.01 (through set_state): the heading error is 0.02, not 2 pi - 0.02."""
    N = 3
    X, P = make_scenario(N, np.dtype(dtype), seed=5, corr=0.1)
    X[2] = -np.pi + 0.01
    s = Scored(monkeypatch, N, dtype, state=(X, P), env={"CSLAM_LOOKAHEAD": "0"}, extra=0, seed=5, capacity=2)
    s.score((1.0, -2.0, np.pi - 0.01))
    s.score((1.0, -2.0, -np.pi + 0.02))
    totals = s.finish("wrap")[0]
    # first call: error 0.02 across the cut; second: -0.01 without wrapping (f32 angles: 1e-6 of slack)
    assert totals[sr.POSE_N] == 2 and abs(totals[sr.POSE_EPHI2] - (0.02 ** 2 + 0.01 ** 2)) < 1e-6


# ------------------------------------------------------------------------------------------------ 5. bad blocks


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bad_blocks(gpu_required, monkeypatch, dtype):
    """P = 0: the pose is BAD, every landmark BAD, nothing enters the sums, the series holds NaN and the totals none.  A
    NaN truth row and one indefinite 2 x 2 block count in LM_BAD only."""
    e = _engine(monkeypatch, 64, dtype)                     # a fresh handle: n = 3, X = 0, P = 0
    e.score_reset(1)
    e.score((0.0, 0.0, 0.0))
    totals, series, track, calls = e.scores()
    assert calls == 1 and totals[sr.POSE_BAD] == 1 and not np.any(np.delete(totals, sr.POSE_BAD))
    assert np.isnan(series).all() and track[0].tolist() == [0.0, 0.0, 0.0, 0.0, 3.0]
    N = 5
    X, _ = make_scenario(N, np.dtype(dtype), seed=2, corr=0.1)
    e.set_state(X, np.zeros((3 + 2 * N, 3 + 2 * N), dtype))  # (set_state leaves the score state alone)
    e.score_set_truth(np.zeros((N, 2)))
    e.score((0.0, 0.0, 0.0))
    totals, series, track, calls = e.scores()
    assert calls == 2 and totals[sr.POSE_BAD] == 2 and totals[sr.LM_BAD] == N and totals[sr.LM_N] == 0
    assert not np.any(np.delete(totals, [sr.POSE_BAD, sr.LM_BAD])) and np.isfinite(totals).all() and series.shape == (1, 4)
    e.close()

    N = 10
    X, P = make_scenario(N, np.dtype(dtype), seed=40, corr=0.1)
    P[9:11, 9:11] = np.array([[1.0, 2.0], [2.0, 1.0]], dtype)   # feature 4: det < 0
    s = Scored(monkeypatch, N, dtype, state=(X, P), env={"CSLAM_LOOKAHEAD": "0"}, extra=0, seed=40, capacity=1)
    s.truth[6] = np.nan                                       # feature 7: no truth
    s.e.score_set_truth(s.truth)
    s.score()
    totals = s.finish("indefinite block and NaN truth")[0]
    assert totals[sr.LM_BAD] == 2 and totals[sr.LM_N] == N - 2 and totals[sr.POSE_N] == 1 and totals[sr.POSE_BAD] == 0


# ------------------------------------------------------------------------------------------------ 6. no perturbation, determinism


def _cadence(e, N, dtype, score):
    """The cadence of test_landmarks_gpu._single_script: 6 steps of predict + heading + update with growing m, one
    augment; score(k) after every update and the augment."""
    rng = np.random.default_rng(3)
    Xs = e.get_x()
    k = 0
    for t in range(6):
        e.predict(83.33, 0.02 * np.sin(t), Q.astype(dtype), WB, DT)
        e.observe_heading(float(Xs[2]) + 1e-3 * t, True)
        idf = _ids(N, 12 + 4 * t, rng, must=(1, 63, N))
        e.update(make_obs(Xs, idf, dtype, seed=t), R.astype(dtype), idf, True)
        if score:
            score(k)
            k += 1
        if t == 3:
            e.augment(np.asfortranarray(np.array([[300.0, 410.0], [0.2, -0.4]], dtype)), R.astype(dtype))
            if score:
                score(k)
                k += 1


def _cadence_run(monkeypatch, dtype, mode, scored):
    N = 130
    X, P = make_scenario(N, np.dtype(dtype), seed=21, corr=0.1)
    e = _engine(monkeypatch, N + 2, dtype, {"CSLAM_LOOKAHEAD": "0"}, sync=(mode == "immediate"))
    e.set_state(X, P)
    if mode == "deferred":
        e.set_deferred(128)
    e.set_profiling(2)
    mid = []

    def score(k):
        e.score((1.0 + 0.01 * k, -2.0, 0.3))
        if k == 3:
            mid.append(e.scores())  # (the one synchronising call, in the middle of the run)

    if scored:
        e.score_reset(8)
        e.score_set_truth(np.concatenate([X[3:].astype(np.float64).reshape(N, 2) + 0.5, np.full((2, 2), 100.0)]))
    _cadence(e, N, dtype, score if scored else None)
    launches = e.stage_times()["downdate"][1]
    sc = e.scores() if scored else None
    assert e.stage_times()["downdate"][1] == launches, "reading the scores launched a P-GEMM"
    out = (e.get_state(), launches, sc, mid)
    e.close()
    return out


@pytest.mark.parametrize("mode", ["immediate", "deferred"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_scoring_does_not_perturb_and_is_deterministic(gpu_required, monkeypatch, dtype, mode):
    """A run scored after every update and augment, with one scores() call mid-run, ends bitwise where the unscored run
    ends, with the same P-GEMM launch count; the scored run twice gives bitwise equal totals, series and track."""
    a = _cadence_run(monkeypatch, dtype, mode, True)
    plain = _cadence_run(monkeypatch, dtype, mode, False)
    c = _cadence_run(monkeypatch, dtype, mode, True)
    (Xa, Pa), (Xb, Pb) = a[0], plain[0]
    assert np.array_equal(Xa, Xb) and np.array_equal(Pa, Pb), "scoring perturbed the run"
    assert a[1] == plain[1] == c[1]
    (ta, sa, ka, ca), (tc, sc, kc, cc) = a[2], c[2]
    assert ca == cc == 7 and sa.shape == (7, 4) and ka.shape == (7, 5)
    assert _bits_equal(ta, tc) and _bits_equal(sa, sc) and _bits_equal(ka, kc)
    assert ta[sr.POSE_N] == 7 and ta[sr.LM_N] + ta[sr.LM_BAD] == 4 * 130 + 3 * 132
    assert a[3][0][3] == 4 and _bits_equal(a[3][0][1], sa[:4]) and _bits_equal(a[3][0][2], ka[:4])


# ------------------------------------------------------------------------------------------------ 7. look-ahead forced


def _lookahead_run(monkeypatch, after):
    """Five predict + update(16) steps with look-ahead windows forced; after(e, t) runs after update t."""
    N = 300
    X, P = make_scenario(N, np.dtype(np.float32), seed=5, corr=0.1)
    e = _engine(monkeypatch, N, np.float32, {"CSLAM_LOOKAHEAD": "1"})
    e.set_state(X, P)
    e.set_deferred(128)
    e.score_set_truth(X[3:].astype(np.float64).reshape(N, 2) + 0.5)
    rng = np.random.default_rng(5)
    for t in range(5):
        e.predict(83.33, 0.01 * t, Q.astype(np.float32), WB, DT)
        idf = _ids(N, 16, rng, must=(1, 63, N))
        e.update(make_obs(X, idf, np.float32, seed=10 + t), R.astype(np.float32), idf, True)
        if after:
            after(e, t)
    state = e.get_state()
    out = (state, e.lookahead_windows(), e.scores())
    e.close()
    return out


def test_lookahead_windows(gpu_required, monkeypatch):
    """CSLAM_LOOKAHEAD=1.  Scoring after EVERY update launches the queued update as a window of one, exactly as a
    landmarks() read at the same points does: bitwise the same end state and window count.  Scoring after every SECOND
    update -- at the window boundaries -- splits no window: bitwise the unscored run, same window count."""
    every = _lookahead_run(monkeypatch, lambda e, t: e.score(XV))
    reads = _lookahead_run(monkeypatch, lambda e, t: e.landmarks())
    assert np.array_equal(every[0][0], reads[0][0]) and np.array_equal(every[0][1], reads[0][1])
    assert every[1] == reads[1] and every[2][3] == 5 and every[2][0][sr.LM_N] + every[2][0][sr.LM_BAD] == 5 * 300
    second = _lookahead_run(monkeypatch, lambda e, t: e.score(XV) if t % 2 == 1 else None)
    plain = _lookahead_run(monkeypatch, None)
    assert np.array_equal(second[0][0], plain[0][0]) and np.array_equal(second[0][1], plain[0][1])
    assert second[1] == plain[1] and second[2][3] == 2 and plain[2][3] == 0
    assert plain[1] < every[1], "the every-update run must have split the windows"


# ------------------------------------------------------------------------------------------------ 8. pipeline mode


def test_pipeline_mode(gpu_required, monkeypatch):
    """Two-stream mode (CSLAM_PIPELINE=1): the score kernels wait for the P-GEMM in flight on stream B."""
    N = 400
    s = Scored(monkeypatch, N, np.float32, env={"CSLAM_PIPELINE": "1", "CSLAM_LOOKAHEAD": "0"}, deferred=0, extra=0, seed=31)
    for t in range(3):
        s.predict()
        s.update(32, must=(1, 63, N))
        s.score()
    totals = s.finish("pipelined")[0]
    assert totals[sr.POSE_N] == 3 and totals[sr.LM_N] + totals[sr.LM_BAD] == 3 * N


# ------------------------------------------------------------------------------------------------ 9. pose()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_pose_read(gpu_required, monkeypatch, dtype):
    """Deferred mode with panels and a heading column pending: x and pvv are bitwise the twin's get_state() X[:3] and
    P[:3, :3]; the read launches no P-GEMM; a NULL output is refused."""
    from conan_slam_amd._capi import ERR_BAD_ARG

    N = 70
    X, P = make_scenario(N, np.dtype(dtype), seed=17, corr=0.1)
    pair = []
    for _ in range(2):
        e = _engine(monkeypatch, N, dtype, {"CSLAM_LOOKAHEAD": "0"})
        e.set_state(X, P)
        e.set_deferred(128)
        e.set_profiling(2)
        rng = np.random.default_rng(17)
        e.predict(83.33, 0.02, Q.astype(dtype), WB, DT)
        idf = _ids(N, 9, rng, must=(1, 63, N))
        e.update(make_obs(X, idf, dtype, seed=1), R.astype(dtype), idf, True)
        e.predict(83.33, -0.01, Q.astype(dtype), WB, DT)
        e.observe_heading(float(X[2]) + 1e-3, True)
        pair.append(e)
    a, t = pair
    before = a.stage_times()["downdate"][1]
    x, pvv = a.pose()
    assert a.stage_times()["downdate"][1] == before, "pose() launched a P-GEMM"
    Xt, Pt = t.get_state()
    assert x.dtype == np.dtype(dtype) and pvv.dtype == np.dtype(dtype)
    assert x.tobytes() == Xt[:3].tobytes() and np.array_equal(pvv, Pt[:3, :3])
    buf = np.full(9, 7.0, dtype)
    p = buf.ctypes.data_as(C.c_void_p)
    assert a._L.cslam_ekf_get_pose(a._h, None, p) == ERR_BAD_ARG
    assert a._L.cslam_ekf_get_pose(a._h, p, None) == ERR_BAD_ARG
    assert np.all(buf == 7.0)
    Xa, Pa = a.get_state()  # (the read did not perturb: the two handles end alike)
    assert np.array_equal(Xa, Xt) and np.array_equal(Pa, Pt)
    a.close()
    t.close()


# ------------------------------------------------------------------------------------------------ 10. series capacity and reset


def test_series_capacity_and_reset(gpu_required, monkeypatch):
    """Capacity 2 and three calls: two records, three calls, all three in the totals; a reset zeroes totals, series, track
    and calls and keeps the truth; a handle scored without a reset keeps totals only."""
    s = Scored(monkeypatch, 5, np.float32, env={"CSLAM_LOOKAHEAD": "0"}, capacity=2)
    for k in range(3):
        s.score((1.0 + 0.1 * k, -2.0, 0.3))
    out = s.e.scores()
    s.ref.check(out, "capacity 2")
    totals, series, track, calls = out
    assert series.shape == (2, 4) and track.shape == (2, 5) and calls == 3 and totals[sr.POSE_N] == 3
    s.e.score_reset(2)
    totals, series, track, calls = s.e.scores()
    assert calls == 0 and series.shape[0] == 0 and track.shape[0] == 0 and not np.any(totals)
    # the log itself was zeroed, not only the record count: read both records raw
    L, h = s.e._L, s.e._h
    raw_s, raw_t, rec = np.ones((2, 4), np.float32), np.ones((2, 5), np.float64), C.c_int(-1)
    s.e.score((1.0, -2.0, 0.3))  # (the truth rows survive a reset)
    assert L.cslam_ekf_get_scores(h, None, raw_s.ctypes.data_as(C.c_void_p), raw_t.ctypes.data_as(C.c_void_p), 2,
                                  C.byref(rec), None) == 0
    assert rec.value == 1 and np.all(raw_s[1] == 1) and np.all(raw_t[1] == 1), "only the records held are copied"
    s.e.score_reset(0)
    s.e.score((1.0, -2.0, 0.3))
    totals, series, track, calls = s.e.scores()
    assert calls == 1 and series.shape[0] == 0 and track.shape[0] == 0 and totals[sr.LM_N] == 5 and totals[sr.POSE_N] == 1
    s.e.close()

    s = Scored(monkeypatch, 4, np.float64, env={"CSLAM_LOOKAHEAD": "0"}, reset=False, extra=0)
    s.score()
    totals, series, track, calls = s.finish("never reset")
    assert calls == 1 and series.shape[0] == 0 and track.shape[0] == 0 and totals[sr.POSE_N] == 1 and totals[sr.LM_N] == 4

    e = _engine(monkeypatch, 4, np.float32)
    totals, series, track, calls = e.scores()  # (never scored: zeros, and nothing allocated for it)
    assert calls == 0 and not np.any(totals) and series.shape[0] == 0
    e.close()


# ------------------------------------------------------------------------------------------------ 11. errors change nothing


def test_errors_change_nothing(gpu_required, monkeypatch):
    from conan_slam_amd._capi import ERR_BAD_ARG

    s = Scored(monkeypatch, 5, np.float32, env={"CSLAM_LOOKAHEAD": "0"}, extra=1, capacity=4)
    s.predict()
    s.update(3, must=(1,))
    s.score()
    before = s.e.scores()
    L, h = s.e._L, s.e._h
    rows = np.zeros((8, 2), np.float64)
    p = rows.ctypes.data_as(C.c_void_p)
    assert L.cslam_ekf_score_reset(h, -1, 0.0, 0.0) == ERR_BAD_ARG
    assert L.cslam_ekf_score_set_truth(h, p, 7) == ERR_BAD_ARG  # max_landmarks = 6
    assert L.cslam_ekf_score_set_truth(h, p, -1) == ERR_BAD_ARG
    assert L.cslam_ekf_score_set_truth(h, None, 2) == ERR_BAD_ARG
    assert L.cslam_ekf_score(h, None, 1) == ERR_BAD_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(3):
            xv = np.array(XV, np.float64)
            xv[i] = bad
            assert L.cslam_ekf_score(h, xv.ctypes.data_as(C.c_void_p), 1) == ERR_BAD_ARG, (bad, i)
    assert L.cslam_ekf_get_scores(h, None, None, None, -1, None, None) == ERR_BAD_ARG
    assert L.cslam_ekf_score(None, p, 1) == ERR_BAD_ARG and L.cslam_ekf_get_pose(None, p, p) == ERR_BAD_ARG
    after = s.e.scores()
    assert all(_bits_equal(x, y) for x, y in zip(before[:3], after[:3])) and before[3] == after[3] == 1
    s.score()  # (the truth rows, the gates and the capacity are the ones set before the refused calls)
    s.finish("after the refused calls")
