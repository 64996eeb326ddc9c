"""The twelve-step loop of test_assoc_counted_gpu.py (predict + association + update on split_scan()'s map), built on the
CPU oracle alone and proven decisive by test_assoc_counted_cpu.py.

The oracle (in the dtype of the run, TEXTBOOK) is driven through the steps.  After each predict a scan is built from ITS
state with the rules of assoc_deferred_ref.split_scan -- own observations at a landmark's predicted measurement plus a
little noise (kind 1), observations far from every landmark (kind 2), observations whose nearest nis lies between the
gates (kind 0, dropped) -- and the oracle is updated with what the f64 reference associates.  Two scan shapes:
  'all'    30 observations, every one associates (the count equals the capacity of the counted update)
  'split'  40 observations with counts (30, 5, 5)
  'split32' 32 observations with counts (24, 4, 4): the largest scan a counted update takes in f64 (m_cap <= 32)
The step noise (SIGMA) is small against the landmark spacing of sparse_state (tens of sigmas), so every observation of
every step is decisive by assoc_builders' margin rule (every margin >= tau, tau = 64 x the C oracle's own error); none is
left out.  The control keeps the pose within 3 m of where split_scan's map was built, so the 'far' observations stay far."""
import numpy as np

from assoc_builders import GATES, R_OBS, Case, pair_reference, predicted
from assoc_deferred_ref import SPLIT_NF, split_scan, symmetric_lower
from helpers import OracleState
from pyoracle import TEXTBOOK

STEPS = 12
SIGMA = (0.05, 0.002)                                  # the noise of split_scan's own observations
CTRL = dict(v=8.0, Q=np.diag([0.18, 6e-4]), wb=2.83, dt=0.025)
KINDS = {"all": [1] * 30, "split": [1] * 30 + [2] * 5 + [0] * 5, "split32": [1] * 24 + [2] * 4 + [0] * 4}
_LOOPS = {}


def swa_of(t):
    return 0.02 * ((t % 5) - 2)


def _scan(X, P, kinds, dtype, rng):
    Xd, Pd, Rd = np.asarray(X, dtype=dtype), np.asarray(P, dtype=dtype), R_OBS.astype(dtype)
    feats = rng.permutation(SPLIT_NF)[: len(kinds)]
    cols = []
    for k, f in zip(kinds, feats):
        zp = predicted(X, int(f), dtype)
        if k == 1:
            cols.append(zp + rng.normal(size=2) * SIGMA)
        elif k == 2:
            cols.append(np.array([20.0 + (3.0 * len(cols)) % 7, zp[1]]))
        else:
            grid = np.linspace(0.1, 12.0, 600)
            Zg = np.stack([zp[0] + grid, np.full_like(grid, zp[1])]).astype(dtype)
            nis = pair_reference(Xd, Pd, Zg, Rd)[0][:, int(f)]
            cols.append(Zg[:, int(np.argmin(np.abs(nis - 12.0)))].astype(np.float64))
    return np.stack(cols, axis=1)[:, rng.permutation(len(kinds))]


def get_loop(shape, dtype):
    """-> list of STEPS dicts: swa, Z (dtype, 2 x m), idf, kind (f64 reference), margin (smallest of the scan), tau"""
    key = (shape, np.dtype(dtype).name)
    if key in _LOOPS:
        return _LOOPS[key]
    base = split_scan()
    dt = np.dtype(dtype).type
    orc = OracleState(base.X.astype(dt), np.asfortranarray(base.P.astype(dt)), dt, TEXTBOOK)
    rng = np.random.default_rng(19_000 + len(KINDS[shape]))
    R = R_OBS.astype(dt)
    steps = []
    for t in range(STEPS):
        orc.predict(CTRL["v"], swa_of(t), CTRL["Q"].astype(dt), CTRL["wb"], CTRL["dt"])
        X, P = orc.x(), symmetric_lower(orc.p())
        case = Case(f"loop-{shape}-{t}", "L", dt, X, P, _scan(X, P, KINDS[shape], dt, rng), R_OBS, gates=GATES[:1])
        idf, kind, _ = case.decisions(GATES[0])
        steps.append(dict(swa=swa_of(t), Z=case.Z, idf=idf, kind=kind, margin=float(case.margins(GATES[0]).min()),
                          tau=case.tau()[0]))
        assert orc.update(np.asfortranarray(case.Z[:, kind == 1]), R, idf[kind == 1], True) == 0
    _LOOPS[key] = steps
    return steps
