"""The input conditions of test_assoc_edges_gpu.py, proved on the CPU oracle alone (no GPU):
  * the numpy f64 pair reference of assoc_builders.py equals Oracle(f64).compute_association on sampled pairs of every
    case;
  * every observation of every case is DECISIVE: each comparison that fixes its (idf, kind) has an f64 margin of at
    least tau, with tau = 64 x the measured error of the C oracle in the case's dtype against that reference (printed);
    none is left out;
  * every coverage property the families promise holds (assoc_builders.check_*);
  * Oracle(f32).data_associate and Oracle(f64).data_associate both return the builder's decisions;
  * negative controls: the decision rule re-run in numpy with one deliberate fault changes at least one decision of the
    family that claims to test it."""
import numpy as np
import pytest

from assoc_builders import (CASE_KEYS, CHECKS, case_id, decide, family_keys, get_case, pair_reference)
from pyoracle import Oracle


@pytest.mark.parametrize("key", CASE_KEYS, ids=case_id)
def test_pair_reference_matches_the_f64_oracle(key):
    """Up to 40 pairs per case, the near ones first (they decide), to 1e-12 relative."""
    case = get_case(key)
    nis, nd = case.ref()[:2]
    o = Oracle(np.float64)
    X, P = case.X.astype(np.float64), np.asfortranarray(case.P.astype(np.float64))
    R = case.R.astype(np.float64)
    near = [tuple(p) for p in case.near_pairs()]
    rng = np.random.default_rng(5)
    pick = [near[k] for k in rng.permutation(len(near))[:30]]
    pick += [(int(rng.integers(case.m)), int(rng.integers(case.nf))) for _ in range(10)]
    worst = 0.0
    for i, j in pick:
        a, b = o.compute_association(X, P, case.n, case.Z[:, i].astype(np.float64), R, j + 1)
        assert abs(a - nis[i, j]) <= 1e-12 * max(1.0, abs(nis[i, j])), (case, i, j, a, nis[i, j])
        assert np.isnan(b) == np.isnan(nd[i, j]), (case, i, j)
        if not np.isnan(b):
            assert abs(b - nd[i, j]) <= 1e-12 * max(1.0, abs(nd[i, j])), (case, i, j, b, nd[i, j])
        worst = max(worst, abs(a - nis[i, j]) / max(1.0, abs(nis[i, j])))
    print(f"{case}: {len(pick)} pairs, worst relative difference in nis {worst:.2e}")


@pytest.mark.parametrize("key", CASE_KEYS, ids=case_id)
def test_every_observation_is_decisive_and_the_oracles_agree(key):
    case = get_case(key)
    found = CHECKS[case.family](case)
    tau, err = case.tau()
    left_out = 0
    for gates in case.gates:
        mg = case.margins(gates)
        print(f"{case} gates {gates}: tau {tau:.3e} (oracle error {err:.3e} over {len(case.near_pairs())} pairs), "
              f"margins [{mg.min():.3e}, {mg.max():.3e}]")
        left_out += int((mg < tau).sum())
        idf, kind, _ = case.decisions(gates)
        for dt in (np.float32, np.float64):
            if np.dtype(dt).itemsize > case.dtype.itemsize or np.dtype(dt) == case.dtype:
                io, ko = case.oracle_decisions(dt, gates)
                assert np.array_equal(io, idf) and np.array_equal(ko, kind), (case, gates, np.dtype(dt).name, io, idf, ko, kind)
    print(f"{case}: coverage {found}; observations {case.m}, left out {left_out}")
    assert left_out == 0, case


def _family_decisions(fam, fault=None, ranked_on_nis=False, **ref_faults):
    """Concatenated (idf, kind) of every case and gate pair of a family, optionally with one fault."""
    out = []
    for key in family_keys(fam):
        case = get_case(key)
        if ref_faults:
            nis, nd = pair_reference(case.X, case.P, case.Z, case.R, **ref_faults)[:2]
        else:
            nis, nd = case.ref()[:2]
        for gates in case.gates:
            idf, kind, _ = decide(nis, nis if ranked_on_nis else nd, *gates, fault=fault)
            out += [idf, kind]
    return np.concatenate(out)


CONTROLS = [
    ("B", dict(fault="inclusive")),
    ("B", dict(fault="last_tie")),
    ("C", dict(fault="gate_on_nd")),
    ("D", dict(fault="outer_first_chunk")),
    ("F", dict(fault="outer_ungated_only")),
    ("E", dict(r_from="r10")),
    ("E", dict(r_from="r01")),
    ("E", dict(no_swap_sign=True)),
    ("E", dict(no_wrap=True)),
    ("A", dict(drop_pose_cross=True)),
    ("A", dict(ranked_on_nis=True)),
]


@pytest.mark.parametrize("fam,fault", CONTROLS, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_a_deliberate_fault_changes_a_decision(fam, fault):
    """(`outer` fed only by ungated features can show only where a gated feature sets no record: family F, where the
    degenerate feature is inside gate1.  In family D nothing is gated, and its control is the reduction of `outer` over
    the first chunk only.)"""
    good = _family_decisions(fam)
    bad = _family_decisions(fam, **fault)
    changed = int((good != bad).sum())
    print(f"family {fam}, fault {fault}: {changed} of {good.size} outputs change")
    assert changed > 0


def test_each_structure_control_is_caught_by_the_case_built_for_it():
    """Within family E: one off-diagonal entry of R taken for both by the non-symmetric R (R[1] and R[2] exchanged cannot
    show: nis and det S are symmetric in S01 and S10), the missing sign by the pivot case, the missing wrap by the wrap
    case."""
    for sub, fault in (("nonsym", dict(r_from="r10")), ("nonsym", dict(r_from="r01")), ("pivot", dict(no_swap_sign=True)), ("wrap", dict(no_wrap=True))):
        case = get_case(("E", sub, "float32"))
        nis, nd = pair_reference(case.X, case.P, case.Z, case.R, **fault)[:2]
        changed = 0
        for gates in case.gates:
            idf, kind, _ = case.decisions(gates)
            i2, k2, _ = decide(nis, nd, *gates)
            changed += int((idf != i2).sum() + (kind != k2).sum())
        print(f"{case}: {fault} changes {changed} outputs")
        assert changed > 0, case
