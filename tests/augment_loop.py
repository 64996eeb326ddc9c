"""The eight-step loop of test_augment_device_gpu.py -- predict, association, update and augment on a growing sparse map
(test/main.cpp:165-189) -- built on the CPU oracle alone and proven decisive by test_augment_device_cpu.py.

The oracle (in the dtype of the run, TEXTBOOK) is driven through the steps from assoc_builders.sparse_state(NF0).  After
each predict a scan of 8 to 10 observations is built from ITS state:
  kind 1  five observations at a feature's predicted measurement plus a little noise; from the second step on, two of
          them aim at features that an EARLIER step augmented, which must associate now
  kind 2  1, 2 or 3 observations (1 + t % 3) far from every feature of the map and from everything already augmented: the
          k-th new feature of the whole run sits at range 20, 30 or 40 m (k % 3) and bearing -2.6 + 0.33 k from the
          heading, while the map's landmarks lie 60 m and more from the pose
  kind 0  two observations of other features whose nis lies between the gates (dropped)
in a random column order.  The oracle is then updated with what the f64 reference associates and augmented with the kind-2
columns in scan order.  The map grows from NF0 = 56 (n = 115) by 15 features to n = 145, across the 128-row tile boundary.
Every observation of every step is decisive by assoc_builders' margin rule (every margin >= tau, tau = 64 x the C
oracle's own error); none is left out."""
import numpy as np

from assoc_builders import GATES, R_OBS, Case, pair_reference, predicted, sparse_state
from assoc_deferred_ref import symmetric_lower
from helpers import OracleState
from pyoracle import TEXTBOOK

STEPS = 8
NF0 = 56
SIGMA = (0.05, 0.002)
CTRL = dict(v=8.0, Q=np.diag([0.18, 6e-4]), wb=2.83, dt=0.025)
N_NEW = [1 + t % 3 for t in range(STEPS)]
NF_END = NF0 + sum(N_NEW)
_LOOPS = {}


def swa_of(t):
    return 0.02 * ((t % 5) - 2)


def _scan(X, P, t, n_aug, new_so_far, dtype, rng):
    """-> (Z f64 [2, 7 + N_NEW[t]], intended kinds) from the oracle's state with n_aug features augmented so far"""
    Xd, Pd, Rd = np.asarray(X, dtype=dtype), np.asarray(P, dtype=dtype), R_OBS.astype(dtype)
    old = [int(f) for f in rng.permutation(NF0)]
    aug = [NF0 + int(f) for f in rng.permutation(n_aug)][:2]
    own = aug + old[: 5 - len(aug)]
    dropped = old[5:7]
    cols, kinds = [], []
    for f in own:
        cols.append(predicted(X, f, dtype) + rng.normal(size=2) * SIGMA)
        kinds.append(1)
    for k in range(new_so_far, new_so_far + N_NEW[t]):
        cols.append(np.array([20.0 + 10.0 * (k % 3), -2.6 + 0.33 * k]))
        kinds.append(2)
    for f in dropped:
        zp = predicted(X, f, dtype)
        grid = np.linspace(0.1, 12.0, 600)
        Zg = np.stack([zp[0] + grid, np.full_like(grid, zp[1])]).astype(dtype)
        nis = pair_reference(Xd, Pd, Zg, Rd)[0][:, f]
        cols.append(Zg[:, int(np.argmin(np.abs(nis - 12.0)))].astype(np.float64))
        kinds.append(0)
    order = rng.permutation(len(cols))
    return np.stack(cols, axis=1)[:, order], np.array(kinds)[order]


def initial_state(dtype):
    X, P = sparse_state(NF0, 21_000)
    return np.array(X, dtype=dtype), np.array(P, dtype=dtype, order="F")


def get_loop(dtype):
    """-> (steps, X_end, P_end): steps is a list of STEPS dicts -- swa, Z (dtype, 2 x (7 + N_NEW[t])), idf, kind (f64 reference on the
    oracle's state), intended (the kinds the scan was built for), margin (smallest of the scan), tau, n (state size
    before the step) -- and X_end / P_end the oracle's state after the last augment."""
    key = np.dtype(dtype).name
    if key in _LOOPS:
        return _LOOPS[key]
    dt = np.dtype(dtype).type
    X0, P0 = initial_state(dt)
    orc = OracleState(X0, P0, dt, TEXTBOOK, extra=sum(N_NEW))
    rng = np.random.default_rng(23_000)
    R = R_OBS.astype(dt)
    steps, new_so_far = [], 0
    for t in range(STEPS):
        orc.predict(CTRL["v"], swa_of(t), CTRL["Q"].astype(dt), CTRL["wb"], CTRL["dt"])
        X, P = orc.x(), symmetric_lower(orc.p())
        Zs, intended = _scan(X, P, t, new_so_far, new_so_far, dt, rng)
        case = Case(f"augment-loop-{t}", "L", dt, X, P, Zs, R_OBS, gates=GATES[:1])
        idf, kind, _ = case.decisions(GATES[0])
        steps.append(dict(swa=swa_of(t), Z=case.Z, idf=idf, kind=kind, intended=intended, n=orc.n,
                          margin=float(case.margins(GATES[0]).min()), tau=case.tau()[0]))
        assert orc.update(np.asfortranarray(case.Z[:, kind == 1]), R, idf[kind == 1], True) == 0
        if (kind == 2).any():
            orc.augment(np.asfortranarray(case.Z[:, kind == 2]), R)
        new_so_far += N_NEW[t]
    _LOOPS[key] = (steps, orc.x(), orc.p())
    return _LOOPS[key]
