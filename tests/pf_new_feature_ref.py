"""Reference of the scan that observes only new features (test/main.cpp:314-328), composed from the CPU oracle:

    [pf_predict]  ->  L = cholesky_decomposition(Pv); X <- L z + X; Pv <- 0  ->  pf_add_features at the sampled pose

L z is accumulated in the particle dtype in column order (s = 0; s += L[r, c] * z[c], c = 0, 1, 2, every product and
sum rounded), which is how the tail of the oracle's sampleProposal and of the device's proposal kernel form it.  The
weights are not touched.  Particles are the lists [w, Xv, Pv, XF, PF] of pf_builders."""
import numpy as np

from pf_builders import copy_parts
from pyoracle import Oracle

SEED = 20250311  # the seed of the statistical case: shown inside 4 sigma on the CPU before it reaches a GPU


def sample_pose(o, Xv, Pv, z):
    """-> (X + chol(Pv) z, the factor) in o.dtype; Xv and Pv are not modified."""
    t = o.dtype.type
    L, _ = o.cholesky_decomposition(Pv)
    XS = np.zeros(3, o.dtype)
    with np.errstate(all="ignore"):
        for r in range(3):
            s = t(0)
            for c in range(3):
                s = t(s + t(L[r, c] * t(z[c])))
            XS[r] = t(s + Xv[r])
    return XS, L


def new_feature_step(parts, dtype, normals, Z=None, R=None, predict=None, Q=None, cap=None):
    """The reference of cslam_pf_[predict +] sample_pose [+ add_features] on copies of `parts`.  normals: 3 x np;
    Z: 2 x q new observations (None: none); predict: (v, swa, wb, dt) with Q, or None; cap: columns of the returned XF /
    PF (default nf0 + q)."""
    o = Oracle(dtype)
    dt = np.dtype(dtype).type
    ps = copy_parts(parts, dt)
    q = 0 if Z is None else np.asarray(Z).reshape(2, -1, order="F").shape[1]
    for i, p in enumerate(ps):
        if predict is not None:
            o.pf_predict(p[1], p[2], predict[0], predict[1], np.asarray(Q, dtype=dtype), predict[2], predict[3])
        p[1], _ = sample_pose(o, p[1], p[2], np.asarray(normals)[:, i])
        p[2] = np.zeros((3, 3), dtype=dtype, order="F")
        nf0 = p[3].shape[1]
        n = nf0 + q
        XF = np.zeros((2, n), dtype=dtype, order="F")
        PF = np.zeros((4, n), dtype=dtype, order="F")
        XF[:, :nf0], PF[:, :nf0] = p[3], p[4]
        if q:
            assert o.pf_add_features(p[1], XF, PF, nf0, np.asfortranarray(np.asarray(Z, dtype=dtype)), R) == n
        p[3], p[4] = XF, PF
    return ps


def indefinite_pv(dtype):
    """A symmetric Pv with one negative eigenvalue (-0.02): the LLT fails, the Jacobi factor holds sqrt of a negative
    number, the factor is zeroed (slam.h:425-434) and the particle keeps its pose."""
    c, s = np.cos(0.4), np.sin(0.4)
    V = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.asfortranarray((V @ np.diag([0.3, -0.02, 1e-3]) @ V.T).astype(dtype))


# ------------------------------------------------------------------------------------------------ the loop from an empty map
LOOP_NP, LOOP_CAP = 8, 6
LOOP_WB, LOOP_DT = 2.8, 0.5
# (v, swa) of the six predicts: two, scan 1 (its own predict), two, scan 2 (its own).  The steering changes from predict
# to predict, so that the rank-2 increments Gu Q Gu^T of three predicts span the pose space: Pv is positive definite
# when a scan samples from it or inverts it (test_pf_new_feature_cpu.py holds the margin)
LOOP_CONTROLS = [(3.0, 0.30), (3.0, -0.25), (3.0, 0.35), (3.0, -0.30), (3.0, 0.28), (3.0, -0.20)]
LOOP_Q = np.diag([0.09, 3e-3])
LOOP_R = np.diag([0.01, 3e-4])
LOOP_LM = np.array([[12.0, 8.0, -6.0, 15.0], [5.0, -9.0, 7.0, -3.0]])  # scan 1 sees 0, 1, 2 (new); scan 2: 0, 1 + 3 (new)


def _observe(pose, cols, dtype):
    d = LOOP_LM[:, cols] - np.array(pose[:2])[:, None]
    Z = np.stack([np.hypot(d[0], d[1]), np.arctan2(d[1], d[0]) - pose[2]])
    return np.asfortranarray(Z.astype(dtype))


def loop_inputs(dtype):
    """-> (controls, scan1 = (ZN,), scan2 = (ZF, idf, ZN)) of the loop case: observations from the noise-free pose."""
    from pf_builders import advance_pose

    pose, poses = (0.0, 0.0, 0.0), []
    for v, swa in LOOP_CONTROLS:
        pose = advance_pose(pose, v, swa, LOOP_WB, LOOP_DT)
        poses.append(pose)
    scan1 = (_observe(poses[2], [0, 1, 2], dtype),)
    scan2 = (_observe(poses[5], [0, 1], dtype), np.array([1, 2], np.int32), _observe(poses[5], [3], dtype))
    return LOOP_CONTROLS, scan1, scan2


def loop_reference(dtype, normals1, normals2=None):
    """The oracle through the loop case.  -> (particles after scan 1, the Pv scan 1 sampled from, and -- with normals2 --
    the weights after scan 2's sampleProposal and the Pv it worked on)."""
    o = Oracle(dtype)
    dt = np.dtype(dtype).type
    Q, R = LOOP_Q.astype(dtype), LOOP_R.astype(dtype)
    controls, (ZN1,), (ZF, idf, ZN2) = loop_inputs(dtype)
    parts = [[dt(1.0 / LOOP_NP), np.zeros(3, dtype), np.zeros((3, 3), dtype, order="F"), np.zeros((2, 0), dtype, order="F"),
              np.zeros((4, 0), dtype, order="F")] for _ in range(LOOP_NP)]
    for v, swa in controls[:3]:
        for p in parts:
            o.pf_predict(p[1], p[2], v, swa, Q, LOOP_WB, LOOP_DT)
    pv1 = [p[2].copy() for p in parts]
    after1 = new_feature_step(parts, dtype, normals1, ZN1, R)
    if normals2 is None:
        return after1, pv1, None, None
    ps = copy_parts(after1, dt)
    for v, swa in controls[3:]:
        for p in ps:
            o.pf_predict(p[1], p[2], v, swa, Q, LOOP_WB, LOOP_DT)
    pv2 = [p[2].copy() for p in ps]
    w = np.zeros(LOOP_NP, dtype)
    for i, p in enumerate(ps):
        wi = np.array([p[0]], dtype=dtype)
        o.pf_sample_proposal(wi, p[1], p[2], p[3], p[4], ZF, idf, R, np.asarray(normals2)[:, i].astype(dtype))
        w[i] = wi[0]
    return after1, pv1, w, pv2


# the statistical case: N particles with ONE common SPD (X, Pv); the sampled poses are N draws of N(X, Pv)
STAT_N = 4096
STAT_X = np.array([1.5, -2.0, 0.3])
STAT_PV = np.array([[0.30, 0.12, -0.010], [0.12, 0.20, 0.006], [-0.010, 0.006, 0.002]])


def assert_distribution(samples, nsigma, tag):
    """samples: N x 3 poses drawn from N(STAT_X, STAT_PV).  The mean within nsigma * sqrt(Pii / N) of X; every sample
    covariance entry within nsigma * sqrt((Pii Pjj + Pij^2) / N) of Pv (the sampling error of a Gaussian's second
    moments).  L^T in place of L gives the covariance L^T L, which is off Pv by hundreds of such sigmas."""
    S = np.asarray(samples, dtype=np.float64)
    N, P = S.shape[0], STAT_PV
    mean, cov = S.mean(axis=0), np.cov(S.T, bias=False)
    zm = (mean - STAT_X) / np.sqrt(np.diag(P) / N)
    zc = (cov - P) / np.sqrt((np.outer(np.diag(P), np.diag(P)) + P * P) / N)
    print(f"[new-feature] {tag}: mean z {np.round(zm, 2)}, covariance z max {np.abs(zc).max():.2f}")
    assert np.all(np.abs(zm) <= nsigma), (tag, zm)
    assert np.all(np.abs(zc) <= nsigma), (tag, zc)
