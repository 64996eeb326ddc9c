"""The score of a Monte-Carlo study on the device (cslam_ekf_batch_score_*, EKFBatch.score / score_scan / scores).

After every score call the test also reads poses() and landmarks() -- the reads a host scorer makes, which leave the run
alone -- and feeds them to the numpy f64 restatement (tests/score_ref.py).  Device and restatement start from the same f32
numbers and work in f64, so they differ by rounding only:
  - the counts (valid, bad, inside the gate) must be EXACT;
  - every sum must lie within the restatement's bound (derived in score_ref's docstring): per landmark
    16 u (Nabs / det + |q| Dabs / det + |q|) with u = 2^-53 -- the f64 rounding of the closed form, growing with the
    cancellation Dabs / det in the block's determinant as computed on the host; per pose 64 u cond_2(Pvv) q plus the
    heading wrap's rounding; (n - 1) u sum |t| for a sum of n terms and one rounding per call for the running totals,
    both sides counted;
  - every series value within the same bound plus half an f32 ulp of the value;
  - a negative control shows these bounds reject a relative error of 1e-6 in every sum and series value.
Scoring never perturbs the run (bitwise against the same run unscored, same windows and P-GEMM launches), is reproducible
bit for bit, and in generator form equals scoring against a truth table built on the host.
"""
import json
import os

import numpy as np
import pytest

import score_ref as sr
from helpers import make_obs, make_scenario
from pyoracle import TEXTBOOK

pytestmark = pytest.mark.gpu

F32 = np.dtype(np.float32)
Q = np.diag([0.18, 6e-4]).astype(np.float32)
R = np.diag([0.08, 0.0024]).astype(np.float32)
WB, DT = 73.0, 0.01
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check(acc, totals, series, calls, tag):
    """Counts exact, sums and series within the bounds -- and the bounds reject a relative error of 1e-6."""
    acc.check(totals, series, calls, tag)
    for f in (sr.POSE_ERR2, sr.POSE_EPHI2, sr.POSE_NEES, sr.LM_ERR2, sr.LM_NEES):
        if not np.any(totals[:, f] != 0):
            continue
        bad = totals.copy()
        bad[:, f] *= 1 + 1e-6
        with pytest.raises(AssertionError):
            acc.check(bad, series, calls, tag)
    if series.size and np.any(np.isfinite(series) & (series != 0)):
        with pytest.raises(AssertionError):
            acc.check(totals, (series.astype(np.float64) * (1 + 1e-6)).astype(np.float32), calls, tag)


class Scored:
    """An EKFBatch of I instances with N landmarks each (room for `extra` more), a truth near the estimate, and the
    restatement fed from poses() / landmarks() after every score call."""

    def __init__(self, I, N, extra=2, seed=0, capacity=16):
        from conan_slam_amd import EKFBatch

        self.I, self.N = I, N
        self.states = [make_scenario(N, F32, seed=seed + i, corr=0.1) for i in range(I)]
        self.b = EKFBatch(I, n_landmarks=N, max_landmarks=N + extra, quirks=TEXTBOOK)
        for i, (X, P) in enumerate(self.states):
            self.b.set_state(i, X, P)
        rng = np.random.default_rng(1000 + seed)
        # the true map: instance 0's initial estimate displaced by about one standard deviation; the new features' truth
        # is anywhere (their blocks are wide)
        self.truth = np.concatenate([self.states[0][0][3:].astype(np.float64).reshape(N, 2) + rng.normal(size=(N, 2)),
                                     rng.uniform(-300, 300, size=(extra, 2))]).astype(np.float32)
        self.b.score_reset(capacity)
        self.b.score_set_truth(self.truth)
        self.acc = sr.Accumulator(I, capacity)
        self.rng, self.keep, self.k = rng, [], 0

    def score(self, xv_true=None):
        xv = np.array([1.05, -2.1, 0.31], np.float32) if xv_true is None else np.asarray(xv_true, np.float32)
        self.b.score(xv)
        x, pvv = self.b.poses()
        xl, pll, _ = self.b.landmarks() if self.b.n_landmarks else (np.zeros((self.I, 0, 2), np.float32),
                                                                    np.zeros((self.I, 0, 2, 2), np.float32), None)
        self.acc.add(x, pvv, xl, pll, self.truth, xv)

    def steps(self, count=2):
        for t in range(count):
            self.b.predict_each([83.0 + 0.2 * i for i in range(self.I)], [0.01 * (t - i) for i in range(self.I)], Q, WB, DT)
            self.b.observe_heading(0.3 + 0.001 * (self.k + t), True)
        self.k += count

    def update(self, m, must=()):
        """m of the first N features (the initial ones: their observations come from the initial estimate)"""
        dz, di = [], []
        for i in range(self.I):
            ids = list(must) + [int(f) for f in self.rng.permutation(self.N) + 1 if int(f) not in must]
            idf = np.array(ids[:m], np.int32)
            dz.append(_dev(make_obs(self.states[i][0], idf, np.float32, seed=self.k + 7 * i).reshape(-1, order="F")))
            di.append(_dev(idf))
        self.keep += dz + di
        self.b.update_device([t.data_ptr() for t in dz], [t.data_ptr() for t in di], m, R)

    def augment(self, q=1):
        dz = [_dev(np.array([[250.0 + 10 * i + 15 * j, 0.5 + 0.1 * i - 0.3 * j] for j in range(q)], np.float32).reshape(-1))
              for i in range(self.I)]
        self.keep += dz
        self.b.augment_device([t.data_ptr() for t in dz], q, R)

    def finish(self, tag):
        totals, series, calls = self.b.scores()
        _check(self.acc, totals, series, calls, tag)
        self.b.close()
        return totals, series


@pytest.mark.parametrize("I,N", [(3, 1), (3, 255), (3, 256), (3, 257), (1, 257)])
def test_values(gpu_required, I, N):
    """Feature counts at the workgroup edges (256 lanes), feature 63 with fx = 127 across two row tiles, one and three
    instances; scored with nothing pending (fresh state, after a flush), with window panels and heading columns pending,
    and right after an augment (the new rows have nothing pending)."""
    s = Scored(I, N, seed=10 * N)
    must = tuple(dict.fromkeys(f for f in (1, 63, N) if f <= N))
    s.score()                                   # kp = 0
    s.steps(2)
    s.update(min(5, N), must=must[: min(5, N)])
    s.score()                                   # the window's panels pending
    s.steps(3)
    s.score()                                   # ... and heading columns
    s.b.flush()
    s.score()                                   # kp = 0 after a flush
    s.steps(1)
    s.update(min(7, N), must=must[: min(7, N)])
    s.augment(2)
    assert s.b.n_landmarks == N + 2
    s.score()                                   # right after an augment, panels pending below
    totals, series = s.finish(f"I={I} N={N}")
    assert np.all(totals[:, sr.POSE_N] == 5) and np.all(totals[:, sr.LM_N] + totals[:, sr.LM_BAD] == 4 * N + N + 2)
    assert series.shape == (5, I, 4)


def test_heading_wrap_on_the_device(gpu_required):
    """True phi = pi - 0.01, estimate -pi + 0.01 (through set_state): the heading error is 0.02, not 2 pi - 0.02."""
    from conan_slam_amd import EKFBatch

    I, N = 2, 3
    b = EKFBatch(I, n_landmarks=N, quirks=TEXTBOOK)
    acc = sr.Accumulator(I, 2)
    for i in range(I):
        X, P = make_scenario(N, F32, seed=5 + i, corr=0.1)
        X[2] = np.float32(-np.pi + 0.01)
        b.set_state(i, X, P)
    truth = np.zeros((N, 2), np.float32)
    b.score_reset(2)
    b.score_set_truth(truth)
    for xv in ([1.0, -2.0, np.pi - 0.01], [1.0, -2.0, -np.pi + 0.02]):
        xv = np.array(xv, np.float32)
        b.score(xv)
        x, pvv = b.poses()
        xl, pll, _ = b.landmarks()
        acc.add(x, pvv, xl, pll, truth, xv)
    totals, series, calls = b.scores()
    _check(acc, totals, series, calls, "wrap")
    # first call: error 0.02 across the cut; second: -0.01 without wrapping (f32 angles: 1e-6 of slack)
    assert np.all(np.abs(totals[:, sr.POSE_EPHI2] - (0.02 ** 2 + 0.01 ** 2)) < 1e-6)
    b.close()


def test_bad_blocks(gpu_required):
    """P = 0 (a fresh handle): the pose is BAD, nothing enters the sums, the series holds NaN and the totals none.  An
    indefinite landmark block in one instance counts in LM_BAD of that instance only."""
    from conan_slam_amd import EKFBatch

    b = EKFBatch(3, n_landmarks=0, max_landmarks=64, quirks=TEXTBOOK)
    b.score_reset(1)
    b.score([0.0, 0.0, 0.0])
    totals, series, calls = b.scores()
    assert calls == 1 and series.shape == (1, 3, 4)
    assert np.all(totals[:, sr.POSE_BAD] == 1) and np.all(totals[:, sr.POSE_N] == 0)
    assert np.all(np.isnan(series)) and np.all(np.isfinite(totals))
    assert np.all(np.delete(totals, sr.POSE_BAD, axis=1) == 0)
    b.close()

    I, N = 3, 10
    b = EKFBatch(I, n_landmarks=N, quirks=TEXTBOOK)
    acc = sr.Accumulator(I, 1)
    for i in range(I):
        X, P = make_scenario(N, F32, seed=40 + i, corr=0.1)
        if i == 1:  # feature 4: det < 0; feature 7: p00 < 0
            P[9:11, 9:11] = np.array([[1.0, 2.0], [2.0, 1.0]], np.float32)
            P[15, 15] = -1.0
        b.set_state(i, X, P)
    truth = np.zeros((N, 2), np.float32)
    b.score_reset(1)
    b.score_set_truth(truth)
    xv = np.array([1.0, -2.0, 0.3], np.float32)
    b.score(xv)
    x, pvv = b.poses()
    xl, pll, _ = b.landmarks()
    acc.add(x, pvv, xl, pll, truth, xv)
    totals, series, calls = b.scores()
    _check(acc, totals, series, calls, "indefinite block")
    assert totals[:, sr.LM_BAD].tolist() == [0, 2, 0] and totals[:, sr.LM_N].tolist() == [N, N - 2, N]
    b.close()


def _cadence(b, dz, di, score):
    """Six observation cycles of the demo cadence (as test_landmarks_gpu._batch_script): predict_each + heading per step,
    update (m = 5) + augment (q = 1); score(b) after every update and every augment."""
    I = b.instances
    zo = io = 0
    for c in range(6):
        for t in range(3):
            b.predict_each([83.0 + 0.2 * i for i in range(I)], [0.01 * (t - i) for i in range(I)], Q, WB, DT)
            b.observe_heading(0.02 * (3 * c + t), True)
        b.update_device([z.data_ptr() + 4 * zo for z in dz], [d.data_ptr() + 4 * io for d in di], 5, R)
        zo, io = zo + 10, io + 5
        if score:
            score(b, 3 * c)
        b.augment_device([z.data_ptr() + 4 * zo for z in dz], 1, R)
        zo += 2
        if score:
            score(b, 3 * c + 1)


def _scored_run(scored, capacity=12):
    from conan_slam_amd import EKFBatch
    from test_landmarks_gpu import _batch_inputs

    I, N = 3, 120
    states, dz, di = _batch_inputs(I, N, seed=80)
    b = EKFBatch(I, n_landmarks=N, max_landmarks=N + 6, quirks=TEXTBOOK)
    for i, (X, P) in enumerate(states):
        b.set_state(i, X, P)
    b.set_profiling(1)
    if scored:
        b.score_reset(capacity)
        b.score_set_truth(np.concatenate([states[0][0][3:].reshape(N, 2) + 0.5, np.full((6, 2), 100.0, np.float32)]))
    _cadence(b, dz, di, (lambda b, k: b.score([1.0 + 0.01 * k, -2.0, 0.3])) if scored else None)
    launches, wins = b.pgemm_time()[1], b.windows()
    sc = b.scores() if scored else None
    assert b.pgemm_time()[1] == launches and b.windows() == wins, "reading the scores launched a P-GEMM or a window"
    out = ([b.get_state(i) for i in range(I)], launches, wins, sc)
    b.close()
    return out


def test_scoring_does_not_perturb_and_is_deterministic(gpu_required):
    """The demo cadence scored after every update and every augment ends bitwise where the unscored run ends, with the
    same windows() and P-GEMM launch count; the same scored run twice gives bitwise equal totals and series."""
    a, plain, c = _scored_run(True), _scored_run(False), _scored_run(True)
    for i in range(3):
        (Xa, Pa), (Xb, Pb) = a[0][i], plain[0][i]
        assert np.array_equal(Xa, Xb) and np.array_equal(Pa, Pb), i
    assert a[1:3] == plain[1:3]
    (ta, sa, ca), (tc, sc, cc) = a[3], c[3]
    assert ca == cc == 12 and sa.shape == (12, 3, 4)
    assert _bits_equal(ta, tc) and _bits_equal(sa, sc)
    assert np.all(ta[:, sr.POSE_N] == 12) and np.all(ta[:, sr.LM_N] + ta[:, sr.LM_BAD] == sum(120 + c for c in range(6)) +
                                                     sum(121 + c for c in range(6)))


def test_series_capacity_and_reset(gpu_required):
    """Capacity 2 and three calls: two records, three calls, all three in the totals; reset zeroes everything; a handle
    scored without a reset keeps totals only."""
    s = Scored(2, 5, capacity=2)
    for k in range(3):
        s.score([1.0 + 0.1 * k, -2.0, 0.3])
    totals, series, calls = s.b.scores()
    _check(s.acc, totals, series, calls, "capacity 2")
    assert series.shape == (2, 2, 4) and calls == 3 and np.all(totals[:, sr.POSE_N] == 3)
    s.b.score_reset(0)
    totals, series, calls = s.b.scores()
    assert calls == 0 and series.shape[0] == 0 and not np.any(totals)
    s.b.score([1.0, -2.0, 0.3])  # (the truth rows survive a reset)
    totals, series, calls = s.b.scores()
    assert calls == 1 and series.shape[0] == 0 and np.all(totals[:, sr.LM_N] == 5)
    s.b.close()

    from conan_slam_amd import EKFBatch

    b = EKFBatch(2, n_landmarks=4, quirks=TEXTBOOK)
    for i in range(2):
        b.set_state(i, *make_scenario(4, F32, seed=i, corr=0.1))
    t0, s0, c0 = b.scores()  # (never scored: zeros)
    assert c0 == 0 and not np.any(t0)
    b.score([1.0, -2.0, 0.3])
    totals, series, calls = b.scores()
    assert calls == 1 and series.shape[0] == 0 and np.all(totals[:, sr.POSE_N] == 1) and np.all(totals[:, sr.LM_N] == 0)
    b.close()


def _generator_run(mode, early, n_control=72):
    """A few observation steps of the demo on the demo map from the device generator.  mode "scan": score_scan; "table":
    score after score_set_truth built on the host from the generator's table."""
    from conan_slam_amd import BatchSimulator, EKFBatch
    from conan_slam_amd.synth import control_noise, noise_matrices
    from test_sim_batch_gpu import _demo_truth

    d = json.load(open(os.path.join(ROOT, "tests", "golden", "demo_map.json")))
    LM = np.asfortranarray(np.array([d["landmarks_x"], d["landmarks_y"]], dtype=np.float32))
    WP = np.asfortranarray(np.array([d["waypoints_x"], d["waypoints_y"]], dtype=np.float32))
    I, seeds = 3, [1000, 1001, 1002]
    cfg, script = _demo_truth(LM, WP, n_control)
    Qn, Rn, QE, RE = noise_matrices(np.float32)
    vn, swan = control_noise(seeds, np.arange(1, len(script) + 1), cfg.velocity, np.array([s[1] for s in script], np.float32), Qn)
    vn, swan = vn.astype(np.float64), swan.astype(np.float64)
    gen = BatchSimulator(LM, I, seeds)
    b = EKFBatch(I, n_landmarks=0, max_landmarks=64, quirks=TEXTBOOK)
    b.score_reset(32)
    wb, dt, rmax = float(cfg.wheel_base), float(np.float32(cfg.dt_controls)), float(cfg.max_range)
    obs = [k for k, s in enumerate(script) if s[2]]
    nxt = dict(zip(obs, obs[1:]))
    made, scored = None, 0
    LMf = np.asarray(LM, np.float32)
    for k, (xv, swa, observe) in enumerate(script):
        b.predict_each(vn[k], swan[k], QE, wb, dt)
        b.observe_heading(float(xv[2]), True)
        if not observe:
            continue
        if made is None:
            gen.scan(xv, rmax, Rn, k + 1)
        made = None
        b.update_scan(gen, RE)
        b.augment_scan(gen, RE)
        if early and k in nxt:
            made = gen.scan(script[nxt[k]][0], rmax, Rn, nxt[k] + 1)  # (the table now runs a scan ahead of the batch)
        if mode == "scan":
            b.score_scan(gen, xv)
        else:
            tab = gen.table
            rows = np.full((max(int(tab.max()), 1), 2), np.nan, np.float32)
            for t in np.nonzero(tab)[0]:
                rows[tab[t] - 1] = LMf[:, t]
            b.score_set_truth(rows[: b.max_landmarks])
            b.score(xv)
        scored += 1
    out = b.scores() + (b.n_landmarks, scored)
    b.close()
    gen.close()
    return out


def test_generator_form(gpu_required):
    """score_scan equals, bitwise, score against a truth table built on the host from get_table() -- also with the next
    scan made early, when the table is ahead of the batch's feature count."""
    ref = _generator_run("table", early=False)
    assert ref[4] >= 4 and ref[3] >= 2, "the run must observe and grow a map"
    assert np.all(ref[0][:, sr.LM_BAD] == 0) and np.all(ref[0][:, sr.LM_N] > 0) and np.all(ref[0][:, sr.POSE_N] == ref[4])
    for mode, early in (("scan", False), ("scan", True), ("table", True)):
        got = _generator_run(mode, early)
        assert got[2:] == ref[2:], (mode, early)
        assert _bits_equal(got[0], ref[0]) and _bits_equal(got[1], ref[1]), (mode, early)


def test_errors_change_nothing(gpu_required):
    import ctypes as C

    from conan_slam_amd import BatchSimulator, _capi

    s = Scored(2, 5, extra=1, capacity=4)
    s.score()
    before = s.b.scores()
    L, h = s.b._L, s.b._h
    rows = np.zeros((8, 2), np.float32)
    p = rows.ctypes.data_as(C.c_void_p)
    assert L.cslam_ekf_batch_score_set_truth(h, p, 7) == _capi.ERR_BAD_ARG  # max_landmarks = 6
    assert L.cslam_ekf_batch_score_set_truth(h, p, -1) == _capi.ERR_BAD_ARG
    assert L.cslam_ekf_batch_score_set_truth(h, None, 2) == _capi.ERR_BAD_ARG
    assert L.cslam_ekf_batch_score(h, None) == _capi.ERR_BAD_ARG
    assert L.cslam_ekf_batch_score_reset(h, -1, 0.0, 0.0) == _capi.ERR_BAD_ARG
    gen = BatchSimulator(np.array([[10.0, 20.0, 30.0], [5.0, -5.0, 0.0]], np.float32), 3, [1, 2, 3])  # 3 instances, not 2
    xv = np.array([1.0, -2.0, 0.3], np.float32)
    xp = xv.ctypes.data_as(C.c_void_p)
    assert L.cslam_ekf_batch_score_scan(h, gen._h, xp) == _capi.ERR_BAD_ARG  # no scan yet
    gen.scan(xv, 100.0, None, 1)
    assert L.cslam_ekf_batch_score_scan(h, gen._h, xp) == _capi.ERR_BAD_ARG  # instance counts differ
    assert L.cslam_ekf_batch_score_scan(h, None, xp) == _capi.ERR_BAD_ARG
    after = s.b.scores()
    assert _bits_equal(before[0], after[0]) and _bits_equal(before[1], after[1]) and before[2] == after[2] == 1
    s.score()  # (the truth rows are the ones set before the refused calls)
    gen.close()
    s.finish("after the refused calls")
