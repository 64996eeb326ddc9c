"""Particle sets of the read-path tests (test_pf_estimate_cpu.py, test_pf_estimate_gpu.py), in the builders' format
([w, Xv, Pv, XF, PF] per particle, see pf_builders.py)."""
import numpy as np

from pf_builders import random_particles
from pf_estimate_ref import pi2pi

OFFSET = (5000.0, -4000.0)
SPREAD = 0.05


def offset_cloud(np_, nf, dtype, seed=0):
    """A converged filter far from the origin: poses and every feature within SPREAD (sigma) of OFFSET, per-particle
    covariances a few times smaller than the scatter, weights uniform(0.5, 1.5) / np.  x^2 is 2.5e7 where the variance
    is 2.5e-3: second moments taken about the origin lose ten digits."""
    rng = np.random.default_rng(9000 + 17 * np_ + seed)
    parts = []
    for _ in range(np_):
        Xv = np.array([OFFSET[0] + rng.normal(0, SPREAD), OFFSET[1] + rng.normal(0, SPREAD), rng.normal(0.2, 0.006)],
                      dtype=dtype)
        A = rng.normal(size=(3, 3)) * np.array([0.01, 0.01, 0.001])[:, None]
        Pv = np.asfortranarray((A @ A.T + np.diag([1e-4, 1e-4, 1e-6])).astype(dtype))
        XF = np.asfortranarray((np.array(OFFSET)[:, None] + rng.normal(0, SPREAD, size=(2, nf))).astype(dtype))
        PF = np.zeros((4, nf), dtype=dtype, order="F")
        for f in range(nf):
            B = rng.normal(size=(2, 2)) * 0.01
            PF[:, f] = (B @ B.T + 1e-4 * np.eye(2)).reshape(-1, order="F")
        parts.append([dtype(rng.uniform(0.5, 1.5) / np_), Xv, Pv, XF, PF])
    return parts


def wrap_cloud(np_, nf, dtype, seed=0):
    """random_particles with headings pi2pi(3.1 + U(-0.1, 0.1)): they straddle +-pi, so their arithmetic mean is near 0
    and their arithmetic variance near pi^2, while the circular mean is near 3.1 and the variance of order 1e-3."""
    parts = random_particles(np_, nf, dtype, seed=700 + seed)
    rng = np.random.default_rng(701 + seed)
    for p in parts:
        p[1][2] = dtype(pi2pi(3.1 + rng.uniform(-0.1, 0.1)))
    return parts
