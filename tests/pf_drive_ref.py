"""A closed-loop FastSLAM-2 drive and its per-particle reference (test_pf_drive_cpu.py, test_pf_drive_gpu.py).

  make_drive(key)        the drive: controls, true poses, noisy scans split by a tag table.  Pure numpy, no device.
  oracle_drive(...)      the CPU oracle's per-particle calls in closed loop (test/main.cpp:279-328), optionally with ONE
                         fault (FAULTS) -- the negative controls
  assoc_drive(...)       the same loop without the tag table: per-particle gated nearest-neighbour association
                         (pf_assoc_ref), the vote on new features and the consumers, in closed loop
  margins(...)           how far every resample decision of a drive is from flipping, against the f32 rounding
  field_errors(...)      the per-scan comparison the GPU file applies: every field of every particle, relative to
                         max(1, |ref|max) of the field

The drive starts from X = 0, Pv = 0, w = 1/np and an EMPTY map; max_features is the number of landmarks it ever sees,
so the last add_features fills the store.  Heading observations are left out: at sigma = 0.01 deg they leave Pv one
rounding from singular, and the next all-new scan would sample through the eigen branch, whose factor is unique only
up to signs.

Precision convention (that of pf_builders.oracle_chain): a drive has an INPUT dtype, in which controls, noise matrices,
observations and draws are rounded, and an arithmetic dtype.  The f64 reference of an f32 run takes the f32 inputs
converted, so that what is compared is arithmetic, not input rounding.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from pf_builders import R_OBS, TOL, advance_pose, copy_parts
from pf_new_feature_ref import sample_pose
from pyoracle import Oracle

from conan_slam_amd import synth

# ------------------------------------------------------------------------------------------------ the drive
# lm_seed: landmarks and observation noise; the map is `clusters` groups of `per_cluster` landmarks (a uniform map dense
# enough for a scan of nine known features has no scan that sees only new ones after the first).
# min_sep > 0: cluster centres are redrawn until they lie at least that far apart (with per_cluster = 1 and spread = 0: a
# map of single landmarks that gated nearest-neighbour association can tell apart).
DriveKey = namedtuple("DriveKey", "lm_seed clusters per_cluster spread n_steps rmax min_sep", defaults=[0.0])
# Z: the scan as observed (2 x m, f64), tags: the landmark of each column, known: which columns the table knows;
# ZF / idf / ZN: the table's split of Z.  kind: known / new / mixed / empty
Scan = namedtuple("Scan", "step kind Z known ZF idf ZN tags nf_before nf_after")
KNOWN, NEW, MIXED, EMPTY = "known", "new", "mixed", "empty"

V, WB, DT = 3.0, 2.8, 0.5
Q_DRIVE = np.diag([0.09, 3e-3])
SCAN_EVERY = 3
AREA = ((-40.0, 17.0), (-9.0, 49.0))  # what the 90 steps of this steering drive through, with 5 m to spare


def steering(k):
    return 0.3 * np.sin(0.37 * k) + 0.12


class Drive:
    def __init__(self, key, landmarks, controls, poses, scans, order):
        self.key, self.landmarks, self.controls, self.poses, self.scans = key, landmarks, controls, poses, scans
        self.order = order                      # landmark of feature j + 1 (the tag order)
        self.max_features = len(order)
        self.truth = landmarks[:, order].T.copy()  # [max_features, 2], row j: the true position of feature j + 1
        self.Q, self.R = Q_DRIVE, R_OBS
        self.by_step = {s.step: s for s in scans}

    def kinds(self):
        return [s.kind for s in self.scans]


def make_drive(key):
    """A pure function of its key."""
    key = DriveKey(*key)
    rng = np.random.default_rng(key.lm_seed)
    centres = np.stack([rng.uniform(*AREA[0], key.clusters), rng.uniform(*AREA[1], key.clusters)])
    for c in range(key.clusters if key.min_sep > 0 else 0):
        while c and np.hypot(*(centres[:, :c] - centres[:, [c]])).min() < key.min_sep:
            centres[:, c] = rng.uniform(*AREA[0]), rng.uniform(*AREA[1])
    lm = (centres[:, :, None] + rng.normal(0.0, key.spread, (2, key.clusters, key.per_cluster))).reshape(2, -1)
    sig = np.sqrt(np.diag(R_OBS))
    pose, controls, poses, scans = (0.0, 0.0, 0.0), [], [], []
    table = -np.ones(lm.shape[1], np.int64)  # tag -> 0-based feature, -1: not in the map
    order = []
    for k in range(key.n_steps):
        swa = float(steering(k))
        controls.append((V, swa))
        pose = advance_pose(pose, V, swa, WB, DT)
        poses.append(pose)
        if k % SCAN_EVERY != SCAN_EVERY - 1:
            continue
        d = lm - np.array(pose[:2])[:, None]
        c, s = np.cos(pose[2]), np.sin(pose[2])
        seen = np.nonzero((np.hypot(d[0], d[1]) < key.rmax) & (d[0] * c + d[1] * s > 0.0))[0]  # the forward half-plane
        Z = np.stack([np.hypot(d[0, seen], d[1, seen]), np.arctan2(d[1, seen], d[0, seen]) - pose[2]])
        Z = Z + rng.normal(size=Z.shape) * sig[:, None]
        Z[1] = np.arctan2(np.sin(Z[1]), np.cos(Z[1]))
        known = table[seen] >= 0
        nf0 = len(order)
        for t in seen[~known]:
            table[t] = len(order)
            order.append(int(t))
        ZF, ZN = np.asfortranarray(Z[:, known]), np.asfortranarray(Z[:, ~known])
        idf = (table[seen[known]] + 1).astype(np.int32)
        kind = (MIXED if ZN.shape[1] else KNOWN) if ZF.shape[1] else (NEW if ZN.shape[1] else EMPTY)
        scans.append(Scan(k, kind, np.asfortranarray(Z), known.copy(), ZF, idf, ZN, seen.copy(), nf0, len(order)))
    return Drive(key, lm, controls, poses, scans, np.array(order, np.int64))


# ------------------------------------------------------------------------------------------------ the reference
FAULTS = ("stale_twin", "weights_not_reset", "weights_unnormalised", "keep_shifted", "draws_reused", "mixed_predict_dropped",
          "mixed_add_at_prior_pose", "pv_not_zeroed", "new_at_unsampled_pose")
ScanResult = namedtuple("ScanResult", "scan rec raw norm select neff resampled keep chol nf")


def n_min(np_):
    """Nmin ~ np/2, an integer (PF.cpp:490 compares Neff with an int)."""
    return (np_ + 1) // 2


def records(parts, nf, dtype=None):
    """Particle lists -> the packed records of cslam_pf_pack: [w, xv(3), pv(9), xf(2 nf), pf(4 nf)] per row."""
    rows = [np.concatenate([[p[0]], p[1], p[2].reshape(-1, order="F"), p[3][:, :nf].reshape(-1, order="F"),
                            p[4][:, :nf].reshape(-1, order="F")]) for p in parts]
    return np.array(rows, dtype=dtype if dtype is not None else parts[0][1].dtype)


def parts_of(rec, nf):
    """The inverse of records(): packed records -> particle lists [w, Xv, Pv, XF, PF]."""
    return [[r[0], r[1:4].copy(), r[4:13].reshape(3, 3, order="F").copy(), r[13:13 + 2 * nf].reshape(2, nf, order="F").copy(),
             r[13 + 2 * nf:13 + 6 * nf].reshape(4, nf, order="F").copy()] for r in rec]


def draws(seed, step, np_, inputs, dtype):
    """The draws of `step` as the _drawn calls consume them at dtype `inputs`, converted to `dtype`."""
    return (synth.pf_draw_normals(seed, step, 0, np_, inputs).astype(dtype),
            synth.pf_draw_select(seed, step, np_, inputs).astype(dtype))


def _proposal_statuses(o, p, ZF, idf, R):
    """LLT status of every covariance one sampleProposal inverts or samples from (PF.cpp:518-534): the prior Pv and the
    posterior after each observation, restated from the oracle's Jacobians in o.dtype (the statuses are what is read;
    the values need not be the oracle's to the bit)."""
    t = o.dtype
    X, P = p[1].copy(), p[2].copy()
    out = [o.cholesky_decomposition(P)[1]]
    for i in range(ZF.shape[1]):
        ZP, HV, _, SF = o.pf_compute_jacobians(X, p[3], p[4], idf[i:i + 1], R)
        H, SFI = HV.reshape(2, 3, order="F"), o.inverse(SF.reshape(2, 2, order="F"))
        v = np.array([ZF[0, i] - ZP[0, 0], o.pi2pi(ZF[1, i] - ZP[1, 0])], dtype=t)
        P = o.inverse((H.T @ SFI @ H + o.inverse(P)).astype(t))
        X = (X + P @ H.T @ SFI @ v).astype(t)
        out.append(o.cholesky_decomposition(P)[1])
    return out


def oracle_drive(drive, dtype, np_, seed, inputs=None, fault=None):
    """The oracle's per-particle calls in closed loop on Oracle(dtype) -> one ScanResult per scan (empty scans included:
    they are predict-only steps).  Every step predicts; with known features seen: proposal, feature update, normalise /
    resample (copies by keep[], w = 1/np), then add the new ones; with only new ones: sample the pose, Pv = 0, add."""
    assert fault is None or fault in FAULTS
    inputs = np.dtype(dtype if inputs is None else inputs)
    dt = np.dtype(dtype).type
    o = Oracle(dtype)
    cvt = lambda a: np.asfortranarray(np.asarray(a, dtype=np.float64).astype(inputs).astype(dtype))
    Q, R = cvt(drive.Q), cvt(drive.R)
    cap, nmin = max(drive.max_features, 1), n_min(np_)
    parts = [[dt(1.0 / np_), np.zeros(3, dtype), np.zeros((3, 3), dtype, order="F"), np.zeros((2, cap), dtype, order="F"),
              np.zeros((4, cap), dtype, order="F")] for _ in range(np_)]
    nf, nf_twin, prev_step, out = 0, 0, None, []
    for k, (v, swa) in enumerate(drive.controls):
        scan = drive.by_step.get(k)
        if not (fault == "mixed_predict_dropped" and scan is not None and scan.kind == MIXED):
            for p in parts:
                o.pf_predict(p[1], p[2], float(inputs.type(v)), float(inputs.type(swa)), Q, WB, DT)
        if scan is None:
            continue
        if scan.kind == EMPTY:
            out.append(ScanResult(scan, records(parts, nf), None, None, None, None, False, None, [], nf))
            continue
        ks = prev_step if (fault == "draws_reused" and prev_step is not None) else k
        normals, select = draws(seed, ks, np_, inputs, dtype)
        prev_step = k
        ZF, ZN = cvt(scan.ZF), cvt(scan.ZN)
        raw = norm = neff = keep = None
        did, chol = False, []
        if scan.kind in (KNOWN, MIXED):
            prior = [p[1].copy() for p in parts]
            w = np.zeros(np_, dtype)
            for i, p in enumerate(parts):
                chol += _proposal_statuses(o, p, ZF, scan.idf, R)
                wi = np.array([p[0]], dtype=dtype)
                o.pf_sample_proposal(wi, p[1], p[2], p[3], p[4], ZF, scan.idf, R, np.ascontiguousarray(normals[:, i]))
                o.pf_feature_update(p[1], p[3], p[4], ZF, scan.idf, R)
                w[i] = wi[0]
            raw = w.copy()
            norm = w.copy()
            o.pf_normalize_resample(norm, nmin, False, select)
            neff, did, keep = o.pf_normalize_resample(w, nmin, True, select)
            if fault == "keep_shifted":
                keep = np.roll(keep, 1)
            for p, wi in zip(parts, raw if fault == "weights_unnormalised" and not did else norm):
                p[0] = dt(wi)
            if did:
                old, parts = parts, copy_parts([parts[j] for j in keep], dt)
                for i, p in enumerate(parts):
                    if fault != "weights_not_reset":
                        p[0] = dt(1.0) / dt(np_)
                    if fault == "stale_twin":  # only the columns of the previous resample's nf travel
                        p[3][:, nf_twin:nf], p[4][:, nf_twin:nf] = old[i][3][:, nf_twin:nf], old[i][4][:, nf_twin:nf]
                nf_twin = nf
            if scan.kind == MIXED:
                for i, p in enumerate(parts):
                    at = prior[keep[i] if did else i] if fault == "mixed_add_at_prior_pose" else p[1]
                    o.pf_add_features(at, p[3], p[4], nf, ZN, R)
        else:
            for i, p in enumerate(parts):
                chol.append(o.cholesky_decomposition(p[2])[1])
                xs, _ = sample_pose(o, p[1], p[2], normals[:, i])
                o.pf_add_features(p[1] if fault == "new_at_unsampled_pose" else xs, p[3], p[4], nf, ZN, R)
                p[1] = xs
                if fault != "pv_not_zeroed":
                    p[2] = np.zeros((3, 3), dtype, order="F")
        nf = scan.nf_after
        out.append(ScanResult(scan, records(parts, nf), raw, norm, select, None if neff is None else float(neff), did, keep,
                              chol, nf))
    return out


# ------------------------------------------------------------------------------------------------ unknown correspondences
GATE1, GATE2, NEW_FRACTION, MISS = 4.0, 25.0, 0.5, 0.01
AssocResult = namedtuple("AssocResult", "scan rec idf kind use margin tau vote_margin resampled neff nf tags")


def assoc_drive(drive, np_, seed, dtype=np.float64):
    """The drive WITHOUT its table, in closed loop: every step predicts; a scan that observes anything associates every
    particle against its own map (pair_reference_pf + decide_cloud + resolve_duplicates, through pf_assoc_ref.Case), votes
    on the new observations (pf.new_feature_votes), runs the consumers on the oracle (consumer_reference), resamples and
    adds the voted columns.  Per scan also: the smallest f64 margin of any (particle, observation) decision with the
    measured tau, and the distance of the nearest vote from NEW_FRACTION as a share of the weight mass."""
    from pf_assoc_ref import Case, consumer_reference

    from conan_slam_amd.pf import new_feature_votes

    dt = np.dtype(dtype).type
    o = Oracle(dtype)
    Q, R = np.asfortranarray(drive.Q.astype(dtype)), np.asfortranarray(drive.R.astype(dtype))
    nmin, gates = n_min(np_), (GATE1, GATE2)
    parts = [[dt(1.0 / np_), np.zeros(3, dtype), np.zeros((3, 3), dtype, order="F"), np.zeros((2, 0), dtype, order="F"),
              np.zeros((4, 0), dtype, order="F")] for _ in range(np_)]
    nf, tags, out = 0, [], []
    for k, (v, swa) in enumerate(drive.controls):
        for p in parts:
            o.pf_predict(p[1], p[2], v, swa, Q, WB, DT)
        scan = drive.by_step.get(k)
        if scan is None or scan.kind == EMPTY:
            continue
        normals, select = draws(seed, k, np_, dtype, dtype)
        Z = np.asfortranarray(scan.Z.astype(dtype))
        case = Case(f"step{k}", dtype, parts, Z, R=R, gates=(gates,))
        idf, kind = case.decisions(gates)
        summary = case.summary(gates)
        new = new_feature_votes(summary, NEW_FRACTION)
        share = summary[:, 1] / summary[:, :3].sum(axis=1)
        use = np.where(new, 0, 1).astype(np.int32)
        parts = consumer_reference(parts, dt, Z, R, idf, use, normals, MISS)
        w = np.array([p[0] for p in parts], dtype=dtype)
        neff, did, keep = o.pf_normalize_resample(w, nmin, True, select)
        for p, wi in zip(parts, w):
            p[0] = dt(wi)
        if did:
            parts = copy_parts([parts[j] for j in keep], dt)
        ZN = np.asfortranarray(Z[:, new])
        q = ZN.shape[1]
        for p in parts:
            XF, PF = np.zeros((2, nf + q), dtype, order="F"), np.zeros((4, nf + q), dtype, order="F")
            XF[:, :nf], PF[:, :nf] = p[3], p[4]
            if q:
                o.pf_add_features(p[1], XF, PF, nf, ZN, R)
            p[3], p[4] = XF, PF
        nf += q
        tags += [int(t) for t in scan.tags[new]]
        out.append(AssocResult(scan, records(parts, nf), idf, kind, use, float(case.margins(gates).min()), case.tau()[0],
                               float(np.abs(share - NEW_FRACTION).min()), did, float(neff), nf, list(tags)))
    return out


# ------------------------------------------------------------------------------------------------ decisiveness
FACTOR = 64.0  # the factor of tests/assoc_builders.py
Margin = namedtuple("Margin", "step select_gap select_diff neff_gap neff_diff same")


def _cum(norm, dtype):
    return np.cumsum(np.asarray(norm, dtype=dtype), dtype=dtype)  # sequential in dtype: the reference's running sum


def margins(hi, lo=None):
    """Per scan with known features: the smallest |select_i - cum_j| over all i, j of the f64 drive `hi`, |Neff - Nmin|,
    and the differences of cum, select and Neff between `lo` (an f32 drive) and `hi`.  Without `lo` the differences are
    the rounding bound of the f64 sums themselves: np eps64 (np additions of values at most 1, relative to Neff <= np for
    Neff)."""
    out = []
    for j, h in enumerate(hi):
        if h.norm is None:
            continue
        np_ = h.norm.shape[0]
        cum = _cum(h.norm, np.float64)
        sel = h.select.astype(np.float64)
        gap = float(np.abs(sel[:, None] - cum[None, :]).min())
        ngap = abs(h.neff - n_min(np_))
        if lo is None:
            e = np_ * np.finfo(np.float64).eps
            out.append(Margin(h.scan.step, gap, e, ngap, e * np_, True))
            continue
        lw = lo[j]
        same = lw.resampled == h.resampled and np.array_equal(lw.keep, h.keep)
        sdiff = max(float(np.abs(_cum(lw.norm, np.float32).astype(np.float64) - cum).max()),
                    float(np.abs(lw.select.astype(np.float64) - sel).max()))
        out.append(Margin(h.scan.step, gap, sdiff, ngap, abs(lw.neff - h.neff), same))
    return out


def decisive(ms):
    return all(m.same and m.select_gap >= FACTOR * m.select_diff and m.neff_gap >= FACTOR * m.neff_diff for m in ms)


# ------------------------------------------------------------------------------------------------ the per-scan check
FIELDS = ("w", "Xv", "Pv", "XF", "PF")
EPS32 = float(np.finfo(np.float32).eps)
EPS64 = float(np.finfo(np.float64).eps)


def field_slices(nf):
    return {"w": slice(0, 1), "Xv": slice(1, 4), "Pv": slice(4, 13), "XF": slice(13, 13 + 2 * nf),
            "PF": slice(13 + 2 * nf, 13 + 6 * nf)}


def field_errors(rec, ref, nf):
    """-> {field: largest |rec - ref| over every particle, relative to max(1, |ref|max) of the field}."""
    rec, ref = np.asarray(rec, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert rec.shape == ref.shape == (ref.shape[0], 13 + 6 * nf), (rec.shape, ref.shape, nf)
    out = {}
    for name, sl in field_slices(nf).items():
        a, b = rec[:, sl], ref[:, sl]
        out[name] = float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if b.size else 0.0
    return out


def fair_bound(cpu_err):
    """The project's fairness rule for an f32 result against the f64 reference: 4 x the CPU f32 oracle's own error plus
    TOL[f32] (both relative to the field's scale)."""
    return 4.0 * cpu_err + TOL[np.dtype(np.float32)]


def amplification(lo, hi):
    """amp = (f32 oracle drive's error against the f64 drive) / eps32, relative to the fields' scales: the largest over
    every scan and field."""
    return max(max(field_errors(a.rec, b.rec, b.nf).values()) for a, b in zip(lo, hi)) / EPS32


def f64_bound(amp):
    """TOL[f64] over the whole drive, or what the reference's own amplification asks for, whichever is larger."""
    return max(TOL[np.dtype(np.float64)], 4.0 * amp * EPS64)


# ------------------------------------------------------------------------------------------------ the committed keys
# Found by a CPU search over lm_seed (the drive) and the draw seed (the particle set); test_pf_drive_cpu.py asserts every
# property the search looked for.
KEY = DriveKey(lm_seed=92, clusters=8, per_cluster=4, spread=2.5, n_steps=90, rmax=15.0)
NP32, SEED32 = 17, 0   # one partial wave; decisive in f32
NP64, SEED64 = 72, 0   # two waves, the second partial; 36 + 36 or 4 x 18 when sharded
# unknown correspondences: single landmarks at least 6 m apart, f64, np = 17
ASSOC_KEY = DriveKey(lm_seed=1, clusters=30, per_cluster=1, spread=0.0, n_steps=90, rmax=15.0, min_sep=6.0)
ASSOC_NP, ASSOC_SEED = 17, 0


@lru_cache(maxsize=None)
def assoc_reference():
    return assoc_drive(make_drive(ASSOC_KEY), ASSOC_NP, ASSOC_SEED)


@lru_cache(maxsize=None)
def committed_drive():
    return make_drive(KEY)


@lru_cache(maxsize=None)
def reference(which):
    """The shared oracle drives of the committed keys, computed once: "f64" (np = 72, f64 inputs), "f32" (np = 17),
    "f32hi" (np = 17, f64 arithmetic on the f32 inputs)."""
    d = committed_drive()
    if which == "f64":
        return oracle_drive(d, np.float64, NP64, SEED64)
    if which == "f32":
        return oracle_drive(d, np.float32, NP32, SEED32)
    assert which == "f32hi"
    return oracle_drive(d, np.float64, NP32, SEED32, inputs=np.float32)
