"""The reference's filter loop through the batched Monte-Carlo engine (test/main.cpp:132-200 x I): predict +
observeHeading on every control step, update + augment on every observation step, one call per reference call for all
instances (cslam_ekf_batch_predict / observe_heading / update / augment).

Every instance is checked against its own CPU oracle (OracleState, f32) with the f64 oracle as the fairness reference,
at the tolerances of test_ekf_gpu.py::test_reference_loop_cadence.  PARITY UNPINNED.
"""
import numpy as np
import pytest

from helpers import OracleState, P_RTOL, X_RTOL, assert_close, make_obs, make_scenario
from pyoracle import REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu

F32 = np.dtype(np.float32)
Q = np.diag([0.18, 6e-4]).astype(np.float32)
R = np.diag([0.08, 0.0024]).astype(np.float32)
WB, DT = 73.0, 0.01


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Loop:
    """One batch and, per instance, an f32 and an f64 oracle driven through the same calls."""

    def __init__(self, states, quirks, extra, oracle=True):
        from conan_slam_amd import EKFBatch

        N = (states[0][0].shape[0] - 3) // 2
        self.I = len(states)
        self.b = EKFBatch(self.I, n_landmarks=N, max_landmarks=N + extra, quirks=quirks)
        for i, (X, P) in enumerate(states):
            self.b.set_state(i, X, P)
        self.oracle = oracle
        self.orc = [OracleState(X, P, np.float32, quirks, extra) for X, P in states] if oracle else []
        self.hi = [OracleState(X.astype(np.float64), P.astype(np.float64), np.float64, quirks, extra)
                   for X, P in states] if oracle else []
        self.keep = []  # device inputs stay alive (and unchanged) until the work has run

    def _all(self):
        return self.orc + self.hi

    def predict(self, v, swa):
        self.b.predict(v, swa, Q, WB, DT)
        for s in self._all():
            s.predict(v, swa, Q, WB, DT)

    def heading(self, phi):
        self.b.observe_heading(phi, True)
        for s in self._all():
            s.observe_heading(phi, True)

    def update(self, obs):
        """obs[i] = (Z 2 x m, idf) of instance i"""
        m = len(obs[0][1])
        dz = [_dev(Z.reshape(-1, order="F")) for Z, _ in obs]
        di = [_dev(np.asarray(idf, dtype=np.int32)) for _, idf in obs]
        self.keep += dz + di
        self.b.update_device([t.data_ptr() for t in dz], [t.data_ptr() for t in di], m, R)
        for i in range(len(self.orc)):
            Z, idf = obs[i]
            self.orc[i].update(Z, R, idf, True)
            self.hi[i].update(Z.astype(np.float64), R.astype(np.float64), idf, True)

    def augment(self, Zns):
        q = Zns[0].shape[1]
        dz = [_dev(Zn.reshape(-1, order="F")) for Zn in Zns]
        self.keep += dz
        self.b.augment_device([t.data_ptr() for t in dz], q, R)
        for i in range(len(self.orc)):
            self.orc[i].augment(Zns[i], R)
            self.hi[i].augment(Zns[i].astype(np.float64), R.astype(np.float64))

    def run(self, ctrls, obs_steps):
        """b.run(len(ctrls)) -- obs_steps[t][i] = (Z, idf) -- against predict + update per step on the oracles"""
        steps, m = len(ctrls), len(obs_steps[0][0][1])
        dz = [_dev(np.concatenate([obs_steps[t][i][0].reshape(-1, order="F") for t in range(steps)]))
              for i in range(self.I)]
        di = [_dev(np.concatenate([np.asarray(obs_steps[t][i][1], np.int32) for t in range(steps)])) for i in range(self.I)]
        self.keep += dz + di
        v = np.array([c[0] for c in ctrls], np.float64)
        s = np.array([c[1] for c in ctrls], np.float64)
        self.b.run(steps, v, s, Q, WB, DT, [t.data_ptr() for t in dz], [t.data_ptr() for t in di], m, R)
        for t in range(steps):
            for o in self._all():
                o.predict(ctrls[t][0], ctrls[t][1], Q, WB, DT)
            for i in range(len(self.orc)):
                Z, idf = obs_steps[t][i]
                self.orc[i].update(Z, R, idf, True)
                self.hi[i].update(Z.astype(np.float64), R.astype(np.float64), idf, True)

    def obs(self, m, rng, seed, ids=None):
        out = []
        for i in range(self.I):
            nf = (self.orc[i].n - 3) // 2
            idf = ids if ids is not None else (rng.permutation(nf)[:m] + 1).astype(np.int32)
            out.append((make_obs(self.orc[i].x(), idf, np.float32, seed=seed + 97 * i), idf))
        return out

    def check(self, tag, instances=None):
        for i in (range(self.I) if instances is None else instances):
            X, P = self.b.get_state(i)
            assert self.b.n == self.orc[i].n, tag
            assert_close(f"{tag} X[{i}]", X, self.orc[i].x(), 4 * X_RTOL[F32], self.hi[i].x(), fair=8.0)
            assert_close(f"{tag} P[{i}]", P, self.orc[i].p(), 4 * P_RTOL[F32], self.hi[i].p(), fair=8.0)

    def close(self):
        self.b.close()


def _states(I, N, seed, corr=0.1):
    return [make_scenario(N, np.float32, seed=seed + i, corr=corr) for i in range(I)]


def _new_features(I, q, cycle):
    return [np.asfortranarray(np.array([[250.0 + 40 * cycle + 10 * i + 15 * j for j in range(q)],
                                        [0.5 - 0.4 * cycle + 0.1 * i - 0.3 * j for j in range(q)]], np.float32))
            for i in range(I)]


def _phi(lp, rng):
    return float(lp.hi[0].x()[2]) + 1e-4 * rng.normal()


@pytest.mark.parametrize("quirks", [TEXTBOOK, REF_EXACT], ids=["textbook", "ref_exact"])
def test_reference_cadence(gpu_required, quirks):
    """3 instances x N = 300, three cycles of 6 x (predict + heading) + update (m = 16, 32) + augment (q = 1, 2)."""
    lp = Loop(_states(3, 300, seed=40), quirks, extra=4)
    rng = np.random.default_rng(5)
    t = 0
    for cycle, (m, q) in enumerate([(16, 1), (32, 2), (32, 1)]):
        for _ in range(6):
            lp.predict(83.33, 0.04 * np.sin(0.3 * t))
            lp.heading(_phi(lp, rng))
            t += 1
        lp.update(lp.obs(m, rng, seed=cycle))
        lp.augment(_new_features(3, q, cycle))
        assert lp.b.n == lp.orc[0].n
    lp.check("cadence")
    assert lp.b.factor_status() == [0, 0, 0]
    lp.close()


def _isolation_script(lp, obs_of, rng_seed):
    rng = np.random.default_rng(rng_seed)
    t = 0
    for cycle, (m, q) in enumerate([(16, 1), (32, 0)]):
        for _ in range(6):
            lp.predict(83.33, 0.04 * np.sin(0.3 * t))
            lp.heading(0.3 + 1e-3 * rng.normal())
            t += 1
        lp.update(obs_of(cycle, m))
        if q:
            lp.augment(obs_of(cycle, -q))


def test_instance_isolation(gpu_required):
    """Instance 0 of a 3-instance batch is bitwise a 1-instance batch fed its inputs; instances 1 and 2, fed identical
    inputs, end bitwise equal."""
    N = 200
    s0, s1 = _states(2, N, seed=70)
    rng = np.random.default_rng(9)
    table = {}
    for cycle, m in enumerate([16, 32]):
        idf = [(rng.permutation(N)[:m] + 1).astype(np.int32) for _ in range(2)]
        table[(cycle, m)] = [(make_obs(s[0], idf[k], np.float32, seed=cycle + 13 * k), idf[k]) for k, s in enumerate((s0, s1))]
        table[(cycle, -1)] = _new_features(2, 1, cycle)

    def obs3(cycle, m):
        o = table[(cycle, m)]
        return [o[0], o[1], o[1]]

    def obs1(cycle, m):
        return [table[(cycle, m)][0]]

    big = Loop([s0, s1, s1], REF_EXACT, extra=1, oracle=False)
    one = Loop([s0], REF_EXACT, extra=1, oracle=False)
    _isolation_script(big, obs3, 3)
    _isolation_script(one, obs1, 3)
    X0, P0 = big.b.get_state(0)
    X1, P1 = big.b.get_state(1)
    X2, P2 = big.b.get_state(2)
    Xs, Ps = one.b.get_state(0)
    assert big.b.n == one.b.n == 3 + 2 * (N + 1)
    assert np.array_equal(X0, Xs) and np.array_equal(P0, Ps)
    assert np.array_equal(X1, X2) and np.array_equal(P1, P2)
    assert not np.array_equal(X0, X1)
    big.close()
    one.close()


def test_predict_update_calls_match_run(gpu_required):
    """predict + update_device (no heading) is bitwise run(steps=1) per step; then a mixed sequence -- run(4), heading
    steps and augment, run(4) -- against the oracle."""
    N, m, I = 300, 24, 2
    states = _states(I, N, seed=90)
    rng = np.random.default_rng(4)
    calls = Loop(states, TEXTBOOK, extra=2)
    runs = Loop(states, TEXTBOOK, extra=2, oracle=False)
    for t in range(3):
        ctrl = (83.33, 0.02 * t)
        obs = calls.obs(m, rng, seed=t)
        calls.predict(*ctrl)
        calls.update(obs)
        runs.run([ctrl], [obs])
    for i in range(I):
        Xa, Pa = calls.b.get_state(i)
        Xb, Pb = runs.b.get_state(i)
        assert np.array_equal(Xa, Xb) and np.array_equal(Pa, Pb), i
    runs.close()
    # mixed: run(4), heading steps and an augment, run(4)
    calls.run([(83.33, 0.01 * t) for t in range(4)], [calls.obs(m, rng, seed=10 + t) for t in range(4)])
    for t in range(3):
        calls.predict(83.33, -0.01 * t)
        calls.heading(_phi(calls, rng))
    calls.augment(_new_features(I, 2, 0))
    calls.run([(83.33, 0.01 * t) for t in range(4)], [calls.obs(m, rng, seed=20 + t) for t in range(4)])
    calls.check("mixed")
    assert calls.b.factor_status() == [0] * I
    calls.close()


def test_growth_across_a_row_tile(gpu_required):
    """N = 62 (n = 127) grows to n = 131 across the 128-row boundary of the P-GEMM tile list; an update then observes
    the new landmarks.  Beyond max_landmarks augment fails with CSLAM_ERR_CAPACITY and changes nothing."""
    from conan_slam_amd import CslamError
    from conan_slam_amd._capi import ERR_CAPACITY

    lp = Loop(_states(2, 62, seed=120), REF_EXACT, extra=2)
    rng = np.random.default_rng(8)
    for t in range(3):
        lp.predict(83.33, 0.03 * t)
        lp.heading(_phi(lp, rng))
    lp.update(lp.obs(16, rng, seed=1))
    assert lp.b.n == 127
    lp.augment(_new_features(2, 2, 1))
    assert lp.b.n == 131
    lp.predict(83.33, 0.01)
    lp.heading(_phi(lp, rng))
    ids = np.concatenate([[63, 64], rng.permutation(62)[:14] + 1]).astype(np.int32)
    lp.update(lp.obs(16, rng, seed=2, ids=ids))
    lp.check("grown")
    before = [lp.b.get_state(i) for i in range(2)]
    with pytest.raises(CslamError) as e:
        lp.augment(_new_features(2, 1, 2))
    assert e.value.code == ERR_CAPACITY
    assert lp.b.n == 131
    for i in range(2):
        X, P = lp.b.get_state(i)
        assert np.array_equal(X, before[i][0]) and np.array_equal(P, before[i][1])
    assert lp.b.factor_status() == [0, 0]
    lp.close()


def test_pose_queue_and_pending_region_limits(gpu_required):
    """10 heading steps between two updates (two pose-queue launches); a run() of two m = 32 updates (128 pending
    columns) followed by a heading step, which must apply the pending panels first."""
    lp = Loop(_states(2, 300, seed=150), TEXTBOOK, extra=0)
    rng = np.random.default_rng(11)
    lp.update(lp.obs(16, rng, seed=1))
    for t in range(10):
        lp.predict(83.33, 0.02 * t)
        lp.heading(_phi(lp, rng))
    lp.update(lp.obs(16, rng, seed=2))
    lp.check("ten headings")
    lp.run([(83.33, 0.01), (83.33, 0.02)], [lp.obs(32, rng, seed=3), lp.obs(32, rng, seed=4)])
    lp.predict(83.33, 0.03)
    lp.heading(_phi(lp, rng))
    lp.update(lp.obs(32, rng, seed=5))
    lp.check("full region")
    assert lp.b.factor_status() == [0, 0]
    lp.close()


def test_heading_skipped_on_indefinite_pose_block(gpu_required):
    """An instance with P22 + R < 0 skips the heading step (bitwise unchanged state, CSLAM_FACTOR_HEADING_SKIPPED);
    the others apply it."""
    from conan_slam_amd._capi import FACTOR_HEADING_SKIPPED

    states = _states(3, 100, seed=180)
    Xb, Pb = states[1]
    Pb = Pb.copy(order="F")
    Pb[2, 2] = -1.0
    states[1] = (Xb, Pb)
    lp = Loop(states, TEXTBOOK, extra=0)
    before = lp.b.get_state(1)
    lp.b.observe_heading(0.31, True)
    for k in (0, 2):
        lp.orc[k].observe_heading(0.31, True)
        lp.hi[k].observe_heading(0.31, True)
    flags = lp.b.factor_status()
    assert flags[1] & FACTOR_HEADING_SKIPPED
    assert flags[0] == 0 and flags[2] == 0
    X, P = lp.b.get_state(1)
    assert np.array_equal(X, before[0]) and np.array_equal(P, before[1])
    lp.check("heading", instances=(0, 2))
    lp.close()


def test_mid_run_state_applies_the_queue(gpu_required):
    """get_state / trace in the middle of a cycle launch the queued pose steps and apply the pending columns."""
    lp = Loop(_states(2, 300, seed=210), REF_EXACT, extra=1)
    rng = np.random.default_rng(12)
    for t in range(6):
        lp.predict(83.33, 0.02 * t)
        lp.heading(_phi(lp, rng))
    lp.update(lp.obs(32, rng, seed=1))
    for t in range(3):
        lp.predict(83.33, -0.02 * t)
        lp.heading(_phi(lp, rng))
    lp.predict(83.33, 0.05)  # held
    tr = lp.b.trace()
    for i in range(2):
        ref = float(np.trace(lp.orc[i].p().astype(np.float64)))
        assert abs(tr[i] - ref) <= 4 * P_RTOL[F32] * max(1.0, abs(ref)), (tr[i], ref)
    lp.check("mid-run")
    lp.augment(_new_features(2, 1, 0))
    lp.update(lp.obs(32, rng, seed=2))
    lp.check("after")
    assert lp.b.factor_status() == [0, 0]
    lp.close()
