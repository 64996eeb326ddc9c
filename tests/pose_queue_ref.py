"""Long runs of control steps through the pose queue: float64 reference, scenario, scripts and the element-wise check
(DESIGN.md 3 "Pose queue at its limits").  CPU only; shared by test_pose_queue_cpu.py and test_pose_queue_gpu.py.

A step is ("predict", v, swa, Q, wb, dt) or ("heading", phi).  The reference replays them on a dense P:
predict as Oracle(np.float64).predict, heading in the rank-1 form P - p p^T / S that the head of ekf_pose_kernels.hpp
derives, which is what the engine evaluates (one pending column w = p / sqrt(S) per heading step).
"""
import numpy as np

from pyoracle import REF_EXACT, Q_PREDICT_NM4, Oracle

FLT_MIN = float(np.finfo(np.float32).tiny)
P22_0 = 1e-10                      # << R = 3.05e-8: S ~ R, so every heading column keeps the weight of the first one
Q_SMALL = np.diag([1e-6, 1e-9])    # keeps P22 below R / 100 (test_pose_queue_cpu.py asserts it)
V0, SWA0, WB, DT = 83.33, 0.05, 73.0, 0.01
INNOVATION = 1e-3
AUGMENT_STEPS = 6  # an augment in the bound: 3-term dot products of products (gamma_5) and one sin / cos evaluation


def unit_roundoff(dtype):
    return float(np.finfo(np.dtype(dtype)).eps) / 2


def heading_R(dtype):
    """sigmaPhi^2 as the engine and the oracle form it: float sigmaPhi = 0.01F * pi / 180 narrowed to the dtype"""
    t = np.dtype(dtype).type
    sigma = t((float(np.float32(0.01)) * np.pi) / 180.0)
    return float(t(sigma * sigma))


def quantise(steps, dtype):
    """The script with every number rounded to the engine's dtype: what its kernels are handed."""
    t = np.dtype(dtype).type
    out = []
    for s in steps:
        if s[0] == "predict":
            _, v, swa, Q, wb, dt = s
            out.append(("predict", float(t(v)), float(t(swa)), np.asarray(Q, dtype=dtype).astype(np.float64),
                        float(t(wb)), float(t(dt))))
        elif s[0] == "augment":
            out.append(("augment", np.asarray(s[1], dtype=dtype).astype(np.float64),
                        np.asarray(s[2], dtype=dtype).astype(np.float64)))
        else:
            out.append((s[0], float(t(s[1]))))
    return out


def _pi2pi(a, work):
    two_pi = work(2) * work(np.pi)
    a = np.fmod(a, two_pi)
    if a > work(np.pi):
        a = a - two_pi
    if a < -work(np.pi):
        a = a + two_pi
    return a


class Replay:
    """The running reference.  work = np.float64 (predict by the f64 oracle itself) or np.longdouble (the same
    formulas in numpy; test_pose_queue_cpu.py holds the two together).  Next to X and P it carries the operand
    magnitudes the check is built from: MP >= |P_ij| + sum |w_ki w_kj| and MX >= |X_i| + sum |W_i| (|phi| + |X_2|)
    (v = phi - X_2 by its operands), propagated through predict with |Gv|, |Gu|.  MX is a deliberate departure from the
    form |X_i| + sum |W_i v| the check was first specified with: about 300 x larger per heading term (see heading()).
    With it X does not detect a lost heading gain -- only P does -- and X is what catches a wrong control."""

    def __init__(self, X0, P0, R, quirks=REF_EXACT, work=np.float64, drop=None):
        self.work = work
        self.X = np.array(X0, dtype=work)
        self.P = np.array(P0, dtype=work, order="F")
        self.n = self.X.shape[0]
        self.R = work(R)
        self.quirks = quirks
        self.drop = drop
        self.MX = np.abs(self.X).astype(np.float64)
        self.MP = np.abs(self.P).astype(np.float64)
        self.headings = 0
        self.queued = 0      # control steps as the pose queue counts them: a predict joins the heading behind it
        self.held = False
        self.S, self.P22 = [], []
        self._orc = Oracle(np.float64, quirks) if work == np.float64 else None

    # -- predict (EKF.cpp:406-455)
    def _jacobians(self, v, swa, wb, dt):
        w = self.work
        phi = self.X[2]
        s, c = np.sin(w(swa) + phi), np.cos(w(swa) + phi)
        Gv = np.array([[1, 0, -w(v) * w(dt) * s], [0, 1, w(v) * w(dt) * c], [0, 0, 1]], dtype=w)
        Gu = np.array([[w(dt) * c, -w(v) * w(dt) * s], [w(dt) * s, w(v) * w(dt) * c],
                       [w(dt) * np.sin(w(swa)) / w(wb), w(v) * w(dt) * np.cos(w(swa)) / w(wb)]], dtype=w)
        return Gv, Gu

    def predict(self, v, swa, Q, wb, dt):
        n, w = self.n, self.work
        Gv, Gu = self._jacobians(v, swa, wb, dt)
        width = 0 if n <= 3 else ((n - 4) if (self.quirks & Q_PREDICT_NM4) else (n - 3))
        aGv, aGu = np.abs(Gv).astype(np.float64), np.abs(Gu).astype(np.float64)
        self.MP[:3, :3] = aGv @ self.MP[:3, :3] @ aGv.T + aGu @ np.abs(np.asarray(Q, np.float64)) @ aGu.T
        if width:
            self.MP[:3, 3:3 + width] = aGv @ self.MP[:3, 3:3 + width]
            self.MP[3:3 + width, :3] = self.MP[:3, 3:3 + width].T
        self.MX[0] += abs(v * dt)
        self.MX[1] += abs(v * dt)
        self.MX[2] += abs(v * dt * np.sin(swa) / wb)
        if self._orc is not None:
            self._orc.predict(self.X, self.P, n, v, swa, np.asfortranarray(Q, dtype=np.float64), wb, dt)
        else:
            Qw = np.asarray(Q, dtype=w)
            phi = self.X[2]
            self.P[:3, :3] = Gv @ self.P[:3, :3] @ Gv.T + Gu @ Qw @ Gu.T
            if width:
                self.P[:3, 3:3 + width] = Gv @ self.P[:3, 3:3 + width]
                self.P[3:3 + width, :3] = self.P[:3, 3:3 + width].T
            self.X[0] = self.X[0] + w(v) * w(dt) * np.cos(w(swa) + phi)
            self.X[1] = self.X[1] + w(v) * w(dt) * np.sin(w(swa) + phi)
            self.X[2] = _pi2pi(phi + w(v) * w(dt) * np.sin(w(swa)) / w(wb), w)
        self.queued += 1 if self.held else 0  # (two predicts in a row: the first is a step of its own)
        self.held = True

    # -- heading (EKF.cpp:328-352 with slam.h:700-725, in the rank-1 form)
    def heading(self, phi):
        w = self.work
        p = self.P[:, 2].copy()
        S = p[2] + self.R
        self.S.append(float(S))
        self.P22.append(float(p[2]))
        vin = _pi2pi(w(phi) - self.X[2], w)
        W = p / S
        self.X = self.X + W * vin
        # the innovation is itself a difference: its operands are phi and X[2] (INNOVATION / |X[2]| ~ 1 / 300 here, so
        # one rounding of X[2] is 300 roundings of v), and X[2] carries the error of the steps before
        self.MX += (np.abs(W) * (abs(float(phi)) + self.MX[2])).astype(np.float64)
        down = np.outer(p, p) / S
        self.MP += np.abs(down).astype(np.float64)
        if self.drop is not None and self.headings == self.drop:
            down[3:, 3:] = 0  # the negative control: this column never reaches the map block
        self.P = np.asfortranarray(self.P - down)
        self.P[[0, 1, 2], [0, 1, 2]] += w(FLT_MIN)
        self.headings += 1
        self.queued += 1
        self.held = False

    # -- one new feature (EKF.cpp:28-91), by the f64 oracle; counted as AUGMENT_STEPS steps of the bound
    def augment(self, z, Rz):
        assert self._orc is not None, "augment: float64 only"
        n = self.n
        r, b = float(z[0]), float(z[1])
        X = np.zeros(n + 2)
        P = np.zeros((n + 2, n + 2), order="F")
        X[:n], P[:n, :n] = self.X, self.P
        assert self._orc.augment(X, P, n, np.array([[r], [b]]), np.asfortranarray(Rz, dtype=np.float64)) == n + 2
        # magnitudes: rows Gv P[0:3, :] with Gv = [I | r (-sin, cos)^T], block Gv Pvv Gv^T + Gz R Gz^T.  sin / cos of
        # an angle rounded to the dtype are off by u |angle| <= u pi, times r: |r| stands for |r sin|, |r cos|
        aGv = np.array([[1.0, 0.0, abs(r)], [0.0, 1.0, abs(r)]])
        aGz = np.array([[1.0, abs(r)], [1.0, abs(r)]])
        MP = np.zeros((n + 2, n + 2))
        MP[:n, :n] = self.MP
        MP[n:, :n] = aGv @ self.MP[:3, :]
        MP[:n, n:] = MP[n:, :n].T
        MP[n:, n:] = aGv @ self.MP[:3, :3] @ aGv.T + aGz @ np.abs(np.asarray(Rz, np.float64)) @ aGz.T
        self.MX = np.concatenate([self.MX, [self.MX[0] + abs(r), self.MX[1] + abs(r)]])
        self.X, self.P, self.MP, self.n = X, P, MP, n + 2
        self.queued += AUGMENT_STEPS + (1 if self.held else 0)
        self.held = False

    def step(self, s):
        if s[0] == "predict":
            self.predict(*s[1:])
        elif s[0] == "heading":
            self.heading(s[1])
        elif s[0] == "augment":
            self.augment(s[1], s[2])
        else:
            assert s[0] == "heading_off"  # observeHeading(phi, false): EKF.cpp:332-335 returns at once

    def result(self):
        return {"X": self.X.copy(), "P": self.P.copy(), "MX": self.MX.copy(), "MP": self.MP.copy(),
                "steps": self.queued + (1 if self.held else 0), "headings": self.headings, "S": list(self.S),
                "P22": list(self.P22)}


def replay(X0, P0, steps, R=None, quirks=REF_EXACT, work=np.float64, drop=None):
    """float64 (or long double) X, P and operand magnitudes after `steps`.  R: heading_R of the engine's dtype."""
    r = Replay(X0, P0, heading_R(np.float64) if R is None else R, quirks, work, drop)
    for s in steps:
        r.step(s)
    return r.result()


def spike_rows(n):
    """map rows (state indices) whose whitened pose correlation is non-zero: the first map row, both sides of every
    128-row tile edge below n, and the last row"""
    rows = {3, n - 1}
    for edge in range(128, n, 128):
        rows.update((edge - 1, edge))
    return sorted(r for r in rows if 3 <= r < n)


def scenario(N, dtype, seed=0):
    """X0, P0 in `dtype`: pose block diag(1e-4, 1e-4, 1e-10), map block I + U U^T, cross block L C D with L the map
    block's Cholesky factor, D = sqrt of the pose block and C whitened correlations of norm (0.3, 0.3, 0.4) carried by
    spike_rows(n): L spreads them over every later row, so no map row is uncorrelated with the heading."""
    rng = np.random.default_rng(seed)
    n = 3 + 2 * N
    pose = np.array([1e-4, 1e-4, P22_0])
    P = np.zeros((n, n))
    P[:3, :3] = np.diag(pose)
    if N:
        U = rng.normal(size=(n - 3, 4)) * 0.3
        M = np.eye(n - 3) + U @ U.T
        L = np.linalg.cholesky(M)
        rows = np.array(spike_rows(n)) - 3
        C = np.zeros((n - 3, 3))
        for c, norm in enumerate((0.3, 0.3, 0.4)):
            sign = np.array([(-1.0) ** ((i >> c) & 1) for i in range(len(rows))])
            C[rows, c] = sign * norm / np.sqrt(len(rows))
        cross = L @ C * np.sqrt(pose)[None, :]
        P[3:, 3:] = M
        P[3:, :3] = cross
        P[:3, 3:] = cross.T
    X = np.concatenate([[1.0, -2.0, 0.3], rng.uniform(-500, 500, size=2 * N)])
    X, P = np.array(X, dtype=dtype), np.array(P, dtype=dtype, order="F")
    P = np.asfortranarray((P + P.T) / 2)
    lam = float(np.linalg.eigvalsh(P.astype(np.float64)).min())
    assert lam > 0.25 * P22_0, f"scenario(N={N}): smallest eigenvalue {lam:.3e}"
    return X, P


def predict_step(v=V0, swa=SWA0, Q=Q_SMALL, wb=WB, dt=DT):
    return ("predict", v, swa, np.array(Q, dtype=np.float64), wb, dt)


class Script:
    """Builds a script along a running f64 reference of the pose, so that every heading is INNOVATION away from the
    heading the filter holds at that step, with alternating sign."""

    def __init__(self, X0, P0, dtype, quirks=REF_EXACT):
        self.dtype = dtype
        # (the pose and its block evolve without reference to the map: the 3-state filter tracks X[2])
        self.ref = Replay(np.asarray(X0, np.float64)[:3], np.asarray(P0, np.float64)[:3, :3], heading_R(dtype), quirks)
        self.steps = []
        self.k = 0

    def _add(self, s):
        s = quantise([s], self.dtype)[0]
        self.ref.step(s)
        self.steps.append(s)

    def predict(self, **kw):
        self._add(predict_step(**kw))
        return self

    def heading(self):
        sign = 1.0 if self.k % 2 == 0 else -1.0
        self.k += 1
        self._add(("heading", float(self.ref.X[2]) + sign * INNOVATION))
        return self

    def control_steps(self, count, vary=False):
        """`count` x (predict; heading); vary: v and swa differ from step to step"""
        for i in range(count):
            if vary:
                self.predict(v=V0 * (1.0 + 0.011 * ((i * 7) % 13 - 6)), swa=0.05 * ((i * 5) % 11 - 5))
            else:
                self.predict()
            self.heading()
        return self


def run_script(X0, P0, dtype, count, quirks=REF_EXACT):
    return Script(X0, P0, dtype, quirks).control_steps(count).steps


def oracle_run(X0, P0, steps, dtype, quirks=REF_EXACT):
    """The CPU oracle in `dtype` over the script, heading in its rank-structured form (structured=True)."""
    o = Oracle(dtype, quirks)
    X = np.array(X0, dtype=dtype)
    P = np.array(P0, dtype=dtype, order="F")
    n = X.shape[0]
    for s in steps:
        if s[0] == "predict":
            o.predict(X, P, n, s[1], s[2], np.asfortranarray(s[3], dtype=dtype), s[4], s[5])
        elif s[0] == "heading":
            o.observe_heading(X, P, n, s[1], True, structured=True)
        elif s[0] == "augment":
            X2, P2 = np.zeros(n + 2, dtype=dtype), np.zeros((n + 2, n + 2), dtype=dtype, order="F")
            X2[:n], P2[:n, :n] = X, P
            n = o.augment(X2, P2, n, np.asfortranarray(np.reshape(s[1], (2, 1)), dtype=dtype),
                          np.asfortranarray(s[2], dtype=dtype))
            X, P = X2, P2
    return X, P


# (steps + C) u x operand magnitude.  C: 4 x the worst the CPU oracle of the same dtype needs against the reference of the
# next precision up, over every case of the GPU tests (measured by test_pose_queue_cpu.py, figures in DESIGN.md 3)
C_MARGIN = {np.dtype(np.float32): 5.2, np.dtype(np.float64): 4.0}  # the oracles need 1.295 and 0.982


def ratios(got_X, got_P, ref, dtype, c=None):
    """(worst error / bound of X, of P) with the bound (steps + c) u M"""
    dt = np.dtype(dtype)
    c = C_MARGIN[dt] if c is None else c
    f = (ref["steps"] + c) * unit_roundoff(dt)
    floor = ref["steps"] * FLT_MIN  # (+ FLT_MIN on the diagonal: the engine adds it to the pose block only)
    bx = f * ref["MX"] + floor
    bp = f * ref["MP"] + floor
    ex = np.abs(np.asarray(got_X, dtype=np.float64) - ref["X"].astype(np.float64))
    ep = np.abs(np.asarray(got_P, dtype=np.float64) - ref["P"].astype(np.float64))
    return float((ex / bx).max()), float((ep / bp).max())


def needed_c(got_X, got_P, ref, dtype):
    """the smallest c >= 0 with which `got` passes: (steps + c) u M >= error everywhere"""
    rx, rp = ratios(got_X, got_P, ref, dtype, c=0.0)
    return max(0.0, (max(rx, rp) - 1.0) * ref["steps"])


def check(got_X, got_P, ref, dtype, name=""):
    """|got - ref| <= (steps + c) u (|X_i| + sum |W_i| (|phi| + |X_2|)) and (steps + c) u (|P_ij| + sum |w_ki w_kj|),
    element-wise"""
    got_X, got_P = np.asarray(got_X), np.asarray(got_P)
    assert got_X.shape == ref["X"].shape and got_P.shape == ref["P"].shape, (name, got_X.shape, got_P.shape)
    assert np.all(np.isfinite(got_X)) and np.all(np.isfinite(got_P)), f"{name}: not finite"
    rx, rp = ratios(got_X, got_P, ref, dtype)
    assert rx <= 1.0, f"{name}: X error / bound = {rx:.3g}"
    assert rp <= 1.0, f"{name}: P error / bound = {rp:.3g}"
    return rx, rp


# ---------------------------------------------------------------------------------------------------------- the cases
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
TEXTBOOK = 0
POSE_SEQ_MAX, WCAP, CTL_SLOTS = 8, 128, 4  # kPoseSeqMax, wcap / kWcols, kCtlSlots of the two engines


def step_kinds_script(X0, P0, dtype, quirks):
    """20 steps of the pose queue with every kind: predict-only steps from predicts in a row, heading-only steps, an
    unused heading between a predict and its heading, and a predict left held at the end."""
    s = Script(X0, P0, dtype, quirks)
    s.predict().heading()                                  # 1
    s.predict().predict(swa=-0.1).heading()                # 2, 3    a predict-only step, then predict + heading
    s.heading().heading()                                  # 4, 5    heading-only steps
    s.predict(v=70.0)
    s.steps.append(("heading_off", 0.25))                  #         observeHeading(phi, false): the predict stays held
    s.heading()                                            # 6
    s.predict().predict().predict(swa=0.2).heading()       # 7, 8, 9 (the ninth step: a launch in the middle of the run)
    s.heading()                                            # 10
    s.control_steps(5)                                     # 11 - 15
    s.heading().predict().predict(swa=-0.2)                # 16, 17
    s.steps.append(("heading_off", 0.5))
    s.heading().control_steps(1)                           # 18, 19
    s.predict(v=90.0, swa=0.1)                             # 20      held: get_state resolves it
    return s.steps


class Case:
    """One handle, one script.  steps(dtype) -> (X0, P0, script in that dtype)."""

    def __init__(self, name, N, seed, builder, quirks=REF_EXACT, dtypes=(F32, F64)):
        self.name, self.N, self.seed, self.builder, self.quirks, self.dtypes = name, N, seed, builder, quirks, dtypes

    def make(self, dtype):
        X0, P0 = scenario(self.N, dtype, self.seed)
        return X0, P0, self.builder(X0, P0, dtype, self.quirks)

    def __repr__(self):
        return self.name


def _run(count):
    return lambda X0, P0, dtype, quirks: run_script(X0, P0, dtype, count, quirks)


RUN_LENGTHS = (1, 7, 8, 9, 16, 17, 131)
RUN_CASES = [Case(f"run{L}-N62", 62, 100 + L, _run(L)) for L in RUN_LENGTHS]
EDGE_CASES = [Case(f"run17-N{N}", N, 200 + N, _run(17)) for N in (63, 64, 126, 127, 190)] + \
             [Case("run131-N127", 127, 331, _run(131))]
KIND_CASES = [Case("kinds-ref_exact", 64, 400, step_kinds_script, REF_EXACT),
              Case("kinds-textbook", 64, 401, step_kinds_script, TEXTBOOK)]
EMPTY_CASE = Case("empty-N0", 0, 500, _run(20))
SECOND_CROSSING = Case("run260-N62", 62, 600, _run(260), dtypes=(F64,))
SINGLE_CASES = RUN_CASES + EDGE_CASES + KIND_CASES + [EMPTY_CASE, SECOND_CROSSING]

# The feature augmented behind the empty-map run.  Its rows of P[:, 2] are -r (sin, cos) P22, so the heading column
# behind it moves the new 2 x 2 block by r^2 P22^2 / S ~ 1e-8 at r = 300, while the block itself stays at the pose
# variance 1e-4 with this small Rz: 600 x the f32 bound.  (At r = 30 and the demo's R = diag(0.08, 0.0024) the column moves
# a block of 1.6 by 3e-10, which no f32 check can see.)
EMPTY_Z = np.array([300.0, 0.7])
EMPTY_RZ = np.diag([1e-6, 1e-12])


def empty_map_tail(X, P, dtype):
    """augment of one feature and one control step behind EMPTY_CASE, from the pose and pose block the run arrived at
    (the augment leaves both as they are)"""
    s = Script(X, P, dtype)
    s.predict().heading()
    return quantise([("augment", EMPTY_Z, EMPTY_RZ)], dtype) + s.steps


def drop_columns(headings):
    """heading steps whose loss the check must notice: first, last, both sides of every launch that a full queue forces
    (8 k - 1 | 8 k) and of the region switch (127 | 128)"""
    js = {0, headings - 1, 7, 8, 127, 128}
    for k in range(POSE_SEQ_MAX, headings, POSE_SEQ_MAX):
        js.update((k - 1, k))
    return sorted(j for j in js if 0 <= j < headings)


# -- the batched engine: I = 2 instances with their own maps and covariances and a common pose and pose block (the
#    heading observation is common to the instances, and the pose recursion does not read the map)
BATCH_I = 2
BATCH_CASES = [("batch-run9-N62", 62, 9), ("batch-run131-N62", 62, 131), ("batch-run17-N127", 127, 17)]
BATCH_RING = ("batch-each41-N62", 62, 41)


def batch_states(name, N):
    seed = 700 + sum(map(ord, name))
    return [scenario(N, np.float32, seed + 17 * i) for i in range(BATCH_I)]


def batch_common_script(name, N, count):
    states = batch_states(name, N)
    return states, run_script(states[0][0], states[0][1], np.float32, count)


def batch_each_scripts(name, N, count):
    """-> states, [script of instance i].  Per step a yaw increment common to the instances and a speed that differs by
    >= 1 % between steps and between instances; swa follows from v dt sin(swa) / wb = increment, so the headings of the
    instances stay together (to f32 rounding of the controls) and one phi serves both."""
    states = batch_states(name, N)
    t = np.float32
    vs = [[float(t(60.0 + 1.1 * ((11 * k + 19 * i) % 43) + 0.55 * i)) for i in range(BATCH_I)] for k in range(count)]
    builders = [Script(X0, P0, np.float32) for X0, P0 in states]
    for k in range(count):
        inc = 3e-3 * (((7 * k) % 9) - 4) / 4.0 + 2e-4
        for i, b in enumerate(builders):
            b.predict(v=vs[k][i], swa=float(np.arcsin(inc * WB / (vs[k][i] * DT))))
        builders[0].heading()
        phi = builders[0].steps[-1]
        for b in builders[1:]:
            b._add(phi)
    return states, [b.steps for b in builders]


# -- between updates: N = 127, m = 9 observations that include landmarks 63 and 127
BETWEEN_N, BETWEEN_RUNS = 127, (12, 131)
BETWEEN_IDF = np.array([1, 17, 63, 64, 65, 90, 126, 127, 40], dtype=np.int32)
BETWEEN_R = np.diag([0.08, 0.0024])
# TEXTBOOK: the gain of REF_EXACT (EKF.cpp's lower Cholesky factor) leaves P indefinite behind the first update of this
# scenario, and both CPU oracles then answer the second one with CHOL_ZEROED, a no-op
BETWEEN_QUIRKS = TEXTBOOK


def between_plan(dtype):
    """update, 12 control steps, update, 131 control steps, update: every input in `dtype`, laid along the f64 oracle.
    -> X0, P0, Z[3], runs[2], hi (the f64 state behind the last update), pending[2]: what a handle that defers its
    downdates (set_deferred) still has pending when run u starts, as (d, columns) per panel -- d the diagonal of P the
    panel removes, d_i = sum_q w_iq^2 without cancellation (see between_ref): the panel of update 1 in front of run 1;
    that, the 12 heading columns of run 1 and the panel of update 2 in front of run 2."""
    from helpers import OracleState, make_obs

    X0, P0 = scenario(BETWEEN_N, dtype, 800)
    hi = OracleState(X0.astype(np.float64), P0.astype(np.float64), np.float64, BETWEEN_QUIRKS)
    Z, runs, panels, pending = [], [], [], []
    for u in range(3):
        Z.append(make_obs(hi.x(), BETWEEN_IDF, dtype, seed=810 + u))
        before = np.diag(hi.p()).copy()
        assert hi.update(Z[u].astype(np.float64), BETWEEN_R, BETWEEN_IDF, True) == 0
        panels.append((np.maximum(before - np.diag(hi.p()), 0.0), 2 * len(BETWEEN_IDF)))
        if u < 2:
            pending.append(list(panels))
            runs.append(run_script(hi.x(), hi.p(), dtype, BETWEEN_RUNS[u], BETWEEN_QUIRKS))
            before = np.diag(hi.p()).copy()
            r = replay(hi.x(), hi.p(), runs[u], heading_R(dtype), BETWEEN_QUIRKS)
            hi.X[:], hi.P[:, :] = r["X"], r["P"]
            panels.append((np.maximum(before - np.diag(hi.p()), 0.0), r["headings"]))
    return {"X0": X0, "P0": P0, "Z": Z, "runs": runs, "hi": hi, "pending": pending}


def between_ref(Xa, Pa, run, dtype, pending=None, drop=None):
    """The reference of a control-step run that starts at the state (Xa, Pa) a handle read back behind an update.
    pending: panels that handle applied for the read but that are still pending when the run starts on its twin
    (set_deferred), so the P-GEMM that applies the run's columns sums theirs with them in an order of its own: their
    columns count as steps, and their magnitudes sum_q |w_iq w_jq| <= sqrt(d_i d_j) (Cauchy-Schwarz on the diagonal the
    panel removed) join the map block's."""
    ref = replay(np.asarray(Xa, np.float64), np.asarray(Pa, np.float64), run, heading_R(dtype), BETWEEN_QUIRKS, drop=drop)
    for d, cols in pending or []:
        ref["MP"][3:, 3:] += np.sqrt(np.outer(d, d))[3:, 3:]
        ref["steps"] += cols
    return ref
