"""Shared inputs of the control-run and whole-cycle tests (test_pf_cycle_cpu.py, test_pf_cycle_gpu.py,
test_adapter_cycle_gpu.py): the control sequences, the heading-known oracle chain, and the bound of the f64
device-against-oracle check of a 6-step run.

THE BOUND.  k = 6 steps of (PF::predict, PF::observeHeading) amplify a rounding error: every heading update forms
1 - W[2] with W[2] -> 1 (R = (0.01 deg)^2 is far below P22), and the next predict spreads what is left over P.  How much
is measured where it can be measured without a device: the CPU oracle runs ORACLE_RUN in f32 and in f64 from the same
f32 inputs, and the difference, per particle and per array, is expressed in units of  u32 * magnitude  (u = the unit
roundoff of the dtype, magnitude = the largest absolute entry of the f64 result's array for that particle, at least 1 for
the pose).  The same chain in f64 amplifies u64 by the same factors, so a second f64 implementation of it -- the device
-- is held to  C_CONTROL * u64 * magnitude  with C_CONTROL = 4 x the measured constant: the margin of 4 is for a third
implementation's operation order inside sin / cos / atan2 (the device's libm is neither the host's f32 nor its f64).
test_pf_cycle_cpu.py measures the constant and holds C_CONTROL to 4 x it; nothing here comes from a device run."""
import numpy as np

from pf_builders import random_particles
from pyoracle import Oracle

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
U = {F32: 2.0 ** -24, F64: 2.0 ** -53}
WB, DT = 73.0, 0.01
Q_CTRL = np.diag([0.18, 6e-4])

# the heading-known control sequence of the oracle tests: k = 6 steps whose v, swa and phi all differ
ORACLE_K = 6
ORACLE_NP = 70
ORACLE_SEED = 21

# 4 x the largest constant test_pf_cycle_cpu.py measures (there: printed with -s, and held to this value)
C_CONTROL = 85.0


def controls(k, seed=0, heading0=0.2):
    """k control steps: v around 83.33, swa in +-0.06, and phi = the noise-free heading from heading0 plus 1 mrad of
    noise -- what a compass would report.  All three differ from step to step."""
    rng = np.random.default_rng(1000 + seed)
    v = 83.33 * (1.0 + 0.05 * rng.uniform(-1, 1, size=k))
    swa = rng.uniform(-0.06, 0.06, size=k)
    phi = np.zeros(k)
    h = heading0
    for j in range(k):
        h = h + v[j] * DT * np.sin(swa[j]) / WB
        phi[j] = h + 1e-3 * rng.normal()
    return v, swa, phi


# ---- a short closed loop with the heading known: five landmarks, five cycles of k = 6 control steps from an empty map
LANDMARKS = np.array([[12.0, 9.0, 15.0, 6.0, 18.0], [3.0, -4.0, -1.0, 7.0, 5.0]])
# per cycle: (known features observed, new landmarks observed): all new, mixed, mixed, known, known
LOOP = [((), (0, 1, 2)), ((0, 2), (3,)), ((1, 3), (4,)), ((0, 1, 2, 3, 4), ()), ((4, 2), ())]
LOOP_K, LOOP_WB, LOOP_DT = 6, 2.83, 0.025
LOOP_Q = np.diag([0.09, 3e-3])
LOOP_R = np.diag([0.08, 0.0024])


def wrap(a):
    return (np.asarray(a) + np.pi) % (2 * np.pi) - np.pi


def advance(pose, v, swa, k, rng, wb=LOOP_WB, dt=LOOP_DT):
    """k noise-free motion steps from `pose` -> (the pose reached, phi[k]: its headings with 0.1 mrad of compass noise)"""
    phi = np.zeros(k)
    for j in range(k):
        pose = np.array([pose[0] + v[j] * dt * np.cos(swa[j] + pose[2]), pose[1] + v[j] * dt * np.sin(swa[j] + pose[2]),
                         float(wrap(pose[2] + v[j] * dt * np.sin(swa[j]) / wb))])
        phi[j] = pose[2] + 1e-4 * rng.normal()
    return pose, phi


def observe(pose, lms, dtype, landmarks=LANDMARKS):
    """noise-free range / bearing of the listed (0-based) landmarks from `pose`, 2 x len(lms)"""
    lms = list(lms)
    dx, dy = landmarks[0, lms] - pose[0], landmarks[1, lms] - pose[1]
    Z = np.stack([np.hypot(dx, dy), wrap(np.arctan2(dy, dx) - pose[2])]) if lms else np.zeros((2, 0))
    return np.asfortranarray(Z.astype(dtype))


def loop_cycles(dtype, pose=(0.0, 0.0, 0.0)):
    """the cycles of LOOP from `pose`: (v[k], swa[k], phi[k], idf, ZF, ZN, the true pose at the scan) per cycle; the
    controls are f32 values, so every layer that carries them in float hands the engine the same numbers"""
    pose = np.array(pose, dtype=np.float64)
    out = []
    for c, (known, new) in enumerate(LOOP):
        rng = np.random.default_rng(c)
        v = (3.0 + rng.uniform(-0.2, 0.2, LOOP_K)).astype(np.float32).astype(np.float64)
        swa = rng.uniform(-0.1, 0.3, LOOP_K).astype(np.float32).astype(np.float64)
        pose, phi = advance(pose, v, swa, LOOP_K, rng)
        phi = phi.astype(np.float32).astype(np.float64)
        idf = np.array([i + 1 for i in known], np.int32)
        out.append((v, swa, phi, idf, observe(pose, known, dtype), observe(pose, new, dtype), pose.copy()))
    return out


def oracle_run_case():
    """(particles in f32, v, swa, phi) of ORACLE_RUN"""
    parts = random_particles(ORACLE_NP, 2, np.float32, seed=ORACLE_SEED)
    return (parts,) + controls(ORACLE_K, seed=ORACLE_SEED)


def oracle_chain(parts, v, swa, phi, dtype, use_heading=True):
    """every particle's (Xv, Pv) after the run on the CPU oracle of `dtype`, from the particles' values converted"""
    o = Oracle(dtype)
    Q = np.asfortranarray(Q_CTRL.astype(dtype))
    out = []
    for p in parts:
        X = np.array(p[1], dtype=dtype)
        P = np.array(p[2], dtype=dtype, order="F")
        for j in range(len(v)):
            o.pf_predict(X, P, float(v[j]), float(swa[j]), Q, WB, DT)
            if use_heading:
                o.pf_observe_heading(X, P, float(phi[j]), True)
        out.append((X, P))
    return out


def units(got, ref, u):
    """the largest error of `got` against `ref` (lists of (Xv, Pv)) in units of u * magnitude -> (for Xv, for Pv)"""
    ex = ep = 0.0
    for (gX, gP), (rX, rP) in zip(got, ref):
        rX, rP = np.asarray(rX, np.float64), np.asarray(rP, np.float64)
        ex = max(ex, float(np.abs(np.asarray(gX, np.float64) - rX).max()) / (u * max(1.0, float(np.abs(rX).max()))))
        ep = max(ep, float(np.abs(np.asarray(gP, np.float64) - rP).max()) / (u * float(np.abs(rP).max())))
    return ex, ep
