"""Shared reference code of the FastSLAM-1 tests (test_pf_fs1_cpu.py, test_pf_fs1_gpu.py, test_adapter_fs1_gpu.py).

  likelihood(...)       PF::likelihood (PF.cpp:343-359) of ONE particle on the CPU oracle, composed from
                        Oracle.pf_compute_jacobians and Oracle.pf_gauss_evaluate one observation at a time, the product in
                        the reference's order ((1 * l_0) * l_1) ...
  LikelihoodCase        the inputs of one cslam_pf_likelihood_update call on the tight cloud of pf_builders
  fs1_drive(...)        the closed-loop drive of pf_drive_ref.make_drive as a FastSLAM-1 filter on the CPU oracle: per
                        control step the predict with every particle's own noisy controls (no heading, as pf_drive_ref
                        explains), per scan the likelihood, the feature update, pf_normalize_resample, Pv = 0, and the new
                        features at the particle's own pose.  Control normals from synth.pf_control_normals, strata from
                        synth.pf_draw_select; the input-dtype convention of pf_drive_ref.

WHAT THE TIGHT CLOUD GIVES.  The figures are those of THIS file's cases (LikelihoodCase: nf = m + 3, the seeds
7000 + 100 m + np); another draw of the same cloud gives other figures of the same order (the design study of this step
quotes 8.8e-5 and 1.2 .. 5.3e9 for the first two).  Measured on the oracle alone (test_pf_fs1_cpu.py prints them), tight_particles / tight_obs / R_OBS: the
f32 oracle's likelihood stays within 1.7e-4 (max, relative) of the f64 one up to m = 17; the f64 values lie between 0.53
and 3.6e10 there.  At m = 65 with R_OBS they reach 5.5e34, within a factor of 6000 of the end of f32 -- hence m = 64, 65
in f64 only, and with 6 R_OBS as pf_builders.ProposalCase has it (then 5.7 .. 4.8e4).  test_pf_fs1_cpu.py holds every
case used on the GPU to 2^+-100 for m <= 17.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import pf_drive_ref as D
from pf_builders import R_OBS, copy_parts, shuffled_idf, tight_obs, tight_particles
from pyoracle import Oracle

from conan_slam_amd import synth


# ------------------------------------------------------------------------------------------------ the likelihood
def likelihood(o, particle, Z, idf, R, dtype):
    """like = ((1 * l_0) * l_1) ... of one particle [w, Xv, Pv, XF, PF] in `dtype` on Oracle o (o.dtype == dtype)."""
    t = np.dtype(dtype).type
    Z = np.asarray(Z, dtype=dtype).reshape(2, -1, order="F")
    like = t(1)
    for i in range(Z.shape[1]):
        ZP, _, _, SF = o.pf_compute_jacobians(particle[1], particle[3], particle[4], idf[i:i + 1], R)
        V = np.array([Z[0, i] - ZP[0, 0], o.pi2pi(t(Z[1, i] - ZP[1, 0]))], dtype=dtype)
        like = t(like * o.pf_gauss_evaluate(V, SF[:, 0].reshape(2, 2, order="F")))
    return like


def likelihoods(parts, Z, idf, R, dtype):
    """The likelihood of every particle of `parts` (converted to `dtype`) -> array of `dtype`."""
    o = Oracle(dtype)
    ps = copy_parts(parts, np.dtype(dtype).type)
    Zc, Rc = np.asfortranarray(np.asarray(Z).astype(dtype)), np.asfortranarray(np.asarray(R).astype(dtype))
    return np.array([likelihood(o, p, Zc, idf, Rc, dtype) for p in ps], dtype=dtype)


LIKE_M = [1, 7, 8, 9, 16, 17]         # one lane's worth, around one chunk of 8, around two
LIKE_NP = [1, 63, 64, 65, 130]        # one lane, around one workgroup's 64 particles, three workgroups
STAGING_NP, STAGING_NF = 9, 68
STAGING_M = [64, 65, 8]               # on ONE shard in this order, f64 only: no growth, the first growth, the memo path


class LikelihoodCase:
    """m observations of distinct features (feature 1 and feature nf among them for m >= 2) on a tight cloud of np_."""

    def __init__(self, m, np_, dtype, nf=None):
        self.m, self.np_, self.dtype = m, np_, dtype
        self.nf = nf if nf is not None else m + 3
        self.seed = 7000 + 100 * m + np_
        self.parts, self.base = tight_particles(np_, self.nf, dtype, self.seed)
        rng = np.random.default_rng(self.seed + 1)
        self.idf = shuffled_idf(self.nf, m, rng) if m >= 2 else np.array([self.nf], np.int32)
        self.Z = tight_obs(self.base, self.idf, dtype, seed=self.seed + 2)
        self.R = np.asfortranarray((R_OBS * (6.0 if m >= 64 else 1.0)).astype(dtype))

    def weights(self, dt):
        """w * like of every particle on the oracle of precision dt, from this case's values converted."""
        like = likelihoods(self.parts, self.Z, self.idf, self.R, dt)
        w = np.array([p[0] for p in self.parts], dtype=dt)
        return (w * like).astype(dt)


def likelihood_case_keys():
    return [(m, n, None) for m in LIKE_M for n in LIKE_NP]


@lru_cache(maxsize=None)
def likelihood_case(key, dtype_name):
    m, n, nf = key
    return LikelihoodCase(m, n, np.dtype(dtype_name).type, nf=nf)


# ------------------------------------------------------------------------------------------------ the drive
Fs1Result = namedtuple("Fs1Result", "scan rec raw norm select neff resampled keep nf")


def fs1_drive(drive, dtype, np_, seed, inputs=None):
    """The FastSLAM-1 filter over `drive` on Oracle(dtype) -> one Fs1Result per scan (empty scans included).  Control step
    k uses the control normals of step k and, at a scan, the strata of step k."""
    inputs = np.dtype(dtype if inputs is None else inputs)
    dt = np.dtype(dtype).type
    o = Oracle(dtype)
    cvt = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64).astype(inputs).astype(dtype))
    Q, R = cvt(drive.Q), cvt(drive.R)
    cap, nmin = max(drive.max_features, 1), D.n_min(np_)
    parts = [[dt(1.0 / np_), np.zeros(3, dtype), np.zeros((3, 3), dtype, order="F"), np.zeros((2, cap), dtype, order="F"),
              np.zeros((4, cap), dtype, order="F")] for _ in range(np_)]
    nf, out = 0, []
    for k, (v, swa) in enumerate(drive.controls):
        normals = synth.pf_control_normals(seed, k, 1, 0, np_, inputs.type)
        vn, swan = synth.pf_control_noise(normals, v, swa, np.asarray(drive.Q), inputs.type)
        for i, p in enumerate(parts):
            o.pf_predict(p[1], p[2], float(vn[0, i]), float(swan[0, i]), Q, D.WB, D.DT)
        scan = drive.by_step.get(k)
        if scan is None:
            continue
        if scan.kind == D.EMPTY:
            out.append(Fs1Result(scan, D.records(parts, nf), None, None, None, None, False, None, nf))
            continue
        ZF, ZN = cvt(scan.ZF), cvt(scan.ZN)
        raw = norm = neff = keep = select = None
        did = False
        if scan.kind in (D.KNOWN, D.MIXED):
            select = synth.pf_draw_select(seed, k, np_, inputs.type).astype(dtype)
            w = np.zeros(np_, dtype)
            for i, p in enumerate(parts):
                w[i] = dt(p[0] * likelihood(o, p, ZF, scan.idf, R, dtype))
                o.pf_feature_update(p[1], p[3], p[4], ZF, scan.idf, R)
                p[2] = np.zeros((3, 3), dtype, order="F")
            raw = w.copy()
            norm = w.copy()
            o.pf_normalize_resample(norm, nmin, False, select)
            neff, did, keep = o.pf_normalize_resample(w, nmin, True, select)
            for p, wi in zip(parts, norm):
                p[0] = dt(wi)
            if did:
                parts = copy_parts([parts[j] for j in keep], dt)
                for p in parts:
                    p[0] = dt(1.0) / dt(np_)
        for p in parts:
            if ZN.shape[1]:
                o.pf_add_features(p[1], p[3], p[4], nf, ZN, R)
        nf = scan.nf_after
        out.append(Fs1Result(scan, D.records(parts, nf), raw, norm, select, None if neff is None else float(neff), did, keep,
                             nf))
    return out


# The committed draw seeds, found by a CPU search over the draw seed on the drive of pf_drive_ref.KEY;
# test_pf_fs1_cpu.py asserts what the search looked for.
NP32, SEED32 = 17, 4   # one partial wave; decisive in f32 (seeds 0, 1 and 3 are not)
NP64, SEED64 = 72, 0   # two waves, the second partial


@lru_cache(maxsize=None)
def reference(which):
    """The shared FastSLAM-1 oracle drives, computed once: "f64" (np = 72), "f32" (np = 17), "f32hi" (np = 17, f64 arithmetic
    on the f32 inputs)."""
    d = D.committed_drive()
    if which == "f64":
        return fs1_drive(d, np.float64, NP64, SEED64)
    if which == "f32":
        return fs1_drive(d, np.float32, NP32, SEED32)
    assert which == "f32hi"
    return fs1_drive(d, np.float64, NP32, SEED32, inputs=np.float32)
