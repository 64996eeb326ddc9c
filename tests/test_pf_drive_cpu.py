"""The closed-loop drive of tests/pf_drive_ref.py, proved on the CPU oracle alone: what the committed keys were searched
for (every branch of the scan dispatcher, the resample patterns, Cholesky statuses, decisive resample decisions) and the
negative controls -- nine one-line faults of the loop, each of which the check of test_pf_drive_gpu.py must reject.
Every figure is printed before it is judged."""
import numpy as np
import pytest

import pf_drive_ref as D
from pyoracle import CHOL_OK

WHICH = ["f32", "f32hi", "f64"]


def _live(res):
    return [r for r in res if r.scan.kind != D.EMPTY]


def test_the_drive_is_a_pure_function_of_its_key():
    a, b = D.make_drive(D.KEY), D.make_drive(tuple(D.KEY))
    assert a.controls == b.controls and a.poses == b.poses and len(a.scans) == len(b.scans) == D.KEY.n_steps // D.SCAN_EVERY
    for x, y in zip(a.scans, b.scans):
        assert x.step == y.step and x.kind == y.kind
        assert x.ZF.tobytes() == y.ZF.tobytes() and x.ZN.tobytes() == y.ZN.tobytes() and np.array_equal(x.idf, y.idf)
    steer = [c[1] for c in a.controls]
    assert len(set(steer)) == len(steer)  # the steering changes from step to step


def test_every_branch_of_the_dispatcher_is_driven():
    d = D.committed_drive()
    kinds = d.kinds()
    counts = {k: kinds.count(k) for k in (D.KNOWN, D.NEW, D.MIXED, D.EMPTY)}
    mf = {k: [s.ZF.shape[1] for s in d.scans if s.kind == k] for k in (D.KNOWN, D.MIXED)}
    mn = {k: [s.ZN.shape[1] for s in d.scans if s.kind == k] for k in (D.NEW, D.MIXED)}
    print(f"[drive] {D.KEY}: scans {counts}, mf known {mf[D.KNOWN]} mixed {mf[D.MIXED]}, mn new {mn[D.NEW]} mixed "
          f"{mn[D.MIXED]}, max_features {d.max_features}")
    assert counts[D.KNOWN] >= 2 and counts[D.NEW] >= 2 and counts[D.MIXED] >= 2
    assert counts[D.KNOWN] + counts[D.NEW] + counts[D.MIXED] >= 12
    assert D.SCAN_EVERY >= 2  # steps without any observation lie between the scans: the predict-only branch
    assert 1 in mf[D.KNOWN] and max(mf[D.KNOWN]) >= 9  # one chunk with a single lane of work, and two chunks
    assert max(mn[D.MIXED]) >= 2
    assert max(max(v) for v in list(mf.values()) + list(mn.values())) <= 32  # every _drawn call launches without a copy
    # the table: features are numbered in the order they were first seen, the last add fills the store
    nf = 0
    for s in d.scans:
        assert s.nf_before == nf and s.nf_after == nf + s.ZN.shape[1] and np.all((1 <= s.idf) & (s.idf <= nf))
        assert len(set(s.idf.tolist())) == len(s.idf)
        nf = s.nf_after
    assert nf == d.max_features == len(set(d.order.tolist())) and d.truth.shape == (nf, 2)
    last_add = [s for s in d.scans if s.ZN.shape[1]][-1]
    assert last_add.nf_after == d.max_features


@pytest.mark.parametrize("which", WHICH)
def test_resample_pattern_and_cholesky_statuses(which):
    res = _live(D.reference(which))
    seq = [(r.scan.kind, r.resampled) for r in res]
    weighted = [r for r in res if r.norm is not None]
    n_res, n_not = sum(r.resampled for r in weighted), sum(not r.resampled for r in weighted)
    not_then_res = [(a.scan.step, b.scan.step) for a, b in zip(res, res[1:])
                    if a.norm is not None and b.norm is not None and not a.resampled and b.resampled]
    res_then_new = [(a.scan.step, b.scan.step) for a, b in zip(res, res[1:]) if a.resampled and b.scan.kind == D.NEW]
    statuses = sorted({s for r in res for s in r.chol})
    print(f"[drive] {which}: {n_res} scans resample, {n_not} do not; not-then-resample at {not_then_res}; resample-then-new "
          f"at {res_then_new}; LLT statuses of {sum(len(r.chol) for r in res)} covariances: {statuses}")
    print(f"[drive] {which}: " + " ".join(f"{r.scan.step}:{r.scan.kind[0]}{'R' if r.resampled else '-'}" for r in res))
    assert n_res >= 4 and n_not >= 2 and not_then_res and res_then_new, seq
    assert statuses == [CHOL_OK]
    assert all(len(r.chol) == (len(r.norm) * (1 + r.scan.ZF.shape[1]) if r.norm is not None else r.rec.shape[0]) for r in res)
    # after every all-new scan each particle stands at its own pose and Pv is zero
    for r in res:
        if r.scan.kind == D.NEW:
            X = r.rec[:, 1:4].astype(np.float64)
            d = np.abs(X[:, None, :] - X[None, :, :]).max(axis=2) + np.eye(X.shape[0])
            assert d.min() > 1e-3, (r.scan.step, d.min())
        assert not r.rec[:, 4:13].any(), r.scan.step
        assert np.all(np.isfinite(r.rec))
        if r.resampled:
            assert np.all(r.rec[:, 0] == r.rec.dtype.type(1.0) / r.rec.dtype.type(r.rec.shape[0]))
    # where no resample follows, the best particle of the read path is not a matter of rounding
    for r in weighted:
        if not r.resampled:
            top = np.sort(r.norm.astype(np.float64))[-2:]
            assert top[1] - top[0] > 1e-4 * top[1], (r.scan.step, top)


@pytest.mark.parametrize("which", ["f32", "f64"])
def test_every_resample_decision_is_decisive(which):
    """f32 (np = 17): the f32 and the f64 oracle drives take the same decision and the same keep[] at every scan, and
    every gap is at least 64 x the f32-against-f64 difference of that scan.  f64 (np = 72): the gaps against the rounding
    of the f64 sums themselves.  No scan and no slot is left out."""
    ms = D.margins(D.reference("f32hi"), D.reference("f32")) if which == "f32" else D.margins(D.reference("f64"))
    for m in ms:
        print(f"[margin] {which} step {m.step}: select gap {m.select_gap:.3e} / diff {m.select_diff:.3e} = "
              f"{m.select_gap / m.select_diff:.1f}; Neff gap {m.neff_gap:.3e} / diff {m.neff_diff:.3e} = "
              f"{m.neff_gap / max(m.neff_diff, 1e-300):.1f}; same decision and keep[]: {m.same}")
    print(f"[margin] {which}: smallest select ratio {min(m.select_gap / m.select_diff for m in ms):.1f}, smallest Neff ratio "
          f"{min(m.neff_gap / max(m.neff_diff, 1e-300) for m in ms):.1f} (required {D.FACTOR:.0f})")
    assert len(ms) >= 8
    assert D.decisive(ms)


def test_amplification_of_the_reference():
    amp = D.amplification(D.reference("f32"), D.reference("f32hi"))
    print(f"[drive] amp = {amp:.1f} (f32 oracle drive against the f64 one, in units of eps32 of the field's scale); "
          f"f64 bound {D.f64_bound(amp):.3e}")
    assert np.isfinite(amp) and D.f64_bound(amp) >= D.TOL[np.dtype(np.float64)]


@pytest.mark.parametrize("fault", D.FAULTS)
def test_negative_controls(fault):
    """The f64 oracle drive with ONE fault against the unfaulted one, under the looser of the two device checks (the f32
    fairness bound): in at least one scan a field exceeds what the check lets pass by a factor of 4 or more."""
    d = D.committed_drive()
    hi, lo = D.reference("f32hi"), D.reference("f32")
    bad = D.oracle_drive(d, np.float64, D.NP32, D.SEED32, inputs=np.float32, fault=fault)
    best, where, first = 0.0, None, None
    for f, h, l in zip(bad, hi, lo):
        ef, ec = D.field_errors(f.rec, h.rec, h.nf), D.field_errors(l.rec, h.rec, h.nf)
        for name in D.FIELDS:
            factor = ef[name] / D.fair_bound(ec[name])
            if factor >= 4.0 and first is None:
                first = (h.scan.step, name, round(factor, 1))
            if factor > best:
                best, where = factor, (h.scan.step, name)
    print(f"[fault] {fault}: {best:.1f} x the bound at (step, field) {where}; first caught at (step, field, factor) {first}")
    assert best >= 4.0, (fault, best)


def test_unknown_correspondences_are_decisive():
    """The drive without its table (ASSOC_KEY: single landmarks at least 6 m apart, f64, np = 17): every (particle,
    observation) decision of every scan has an f64 margin of at least the measured tau of pf_assoc_ref (the rule behind
    TAU_SEARCH), every vote is at least 0.1 of the weight mass away from new_fraction, and the policy builds the table's
    map -- the same landmarks in the same order."""
    from pf_assoc_ref import TAU_SEARCH

    d = D.make_drive(D.ASSOC_KEY)
    res = D.assoc_reference()
    live = [s for s in d.scans if s.kind != D.EMPTY]
    assert len(res) == len(live) >= 8
    for r in res:
        print(f"[assoc] step {r.scan.step}: m {r.scan.Z.shape[1]}, new {int((1 - r.use).sum())}, matched "
              f"{int((r.kind == 1).sum())} ambiguous {int((r.kind == 0).sum())} of {r.kind.size}; smallest margin "
              f"{r.margin:.3e} (tau {r.tau:.3e}); nearest vote {r.vote_margin:.2f} from {D.NEW_FRACTION}; resampled {r.resampled}")
        assert r.margin >= r.tau and r.margin >= TAU_SEARCH[np.dtype(np.float64)], (r.scan.step, r.margin, r.tau)
        assert r.vote_margin >= 0.1, (r.scan.step, r.vote_margin)
        assert np.array_equal(r.use == 0, ~r.scan.known), r.scan.step  # the vote splits the scan as the table does
        assert r.nf == r.scan.nf_after and np.all(np.isfinite(r.rec))
    print(f"[assoc] {D.ASSOC_KEY}: {len(res)} scans, {sum(r.resampled for r in res)} resample, smallest margin "
          f"{min(r.margin for r in res):.3e}, largest tau {max(r.tau for r in res):.3e}, nearest vote "
          f"{min(r.vote_margin for r in res):.2f}, {sum(int((r.kind == 0).sum()) for r in res)} decisions pay miss_likelihood")
    assert res[-1].tags == d.order.tolist() and res[-1].nf == d.max_features
    assert sum(r.resampled for r in res) >= 4 and sum(not r.resampled for r in res) >= 2
    assert any((r.kind == 0).any() for r in res) and any((r.kind == 1).any() for r in res)
