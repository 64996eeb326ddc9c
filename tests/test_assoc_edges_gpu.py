"""cslam_ekf_associate (ekf_assoc_feature_kernel + ekf_assoc_scan_kernel) where candidates compete.

Every case of assoc_builders.py is DECISIVE: each comparison that fixes an observation's (idf, kind) has a margin in the
f64 reference of at least 64 x the C oracle's own error in the case's dtype (test_assoc_edges_cpu.py proves it, and that
the f32 and f64 oracles return the builder's decisions).  That is what makes equality of integers the right assertion
here: this file compares integers and copied observations only.
  A  dense cluster: up to 257 features inside gate1, winners at the ends of the 64-lane chunks and in later chunks
  B  exact ties between twin landmarks: the lower index wins, within a chunk and across chunks
  C  the lowest nd lies outside gate1: gating is on nis, ranking on nd
  D  nothing gated: `outer` just under / over gate2, its minimum in every position of the reduction
  E  non-symmetric R, both branches of the pivoted 2 x 2 LU, bearing innovations beyond +-pi
  F  a feature with det S < 0 (nd is NaN): never a record, but it feeds `outer`
  G  the host side: held predict, queued heading step, pending downdates, growing m, a growing map, m = 0, m > nf"""
import numpy as np
import pytest

from assoc_builders import CASE_KEYS, case_id, get_case, predicted
from pyoracle import REF_EXACT, TEXTBOOK

pytestmark = pytest.mark.gpu

QUIRKS = [REF_EXACT, TEXTBOOK]
Q_CTRL = np.diag([0.18, 6e-4])
PREDICT = (83.33, 0.03, 73.0, 0.01)


def _engine(case, quirks, extra=0):
    from conan_slam_amd import EKF

    e = EKF(case.nf + extra, dtype=case.dtype.type, quirks=quirks)
    e.set_state(case.X, case.P)
    return e


@pytest.mark.parametrize("quirks", QUIRKS, ids=["ref_exact", "textbook"])
@pytest.mark.parametrize("key", CASE_KEYS, ids=case_id)
def test_associate_returns_the_decisive_reference(gpu_required, key, quirks):
    case = get_case(key)
    eng = _engine(case, quirks)
    for gates in case.gates:
        idf_r, kind_r, _ = case.decisions(gates)
        idf, kind = eng.associate(case.Z, case.R, *gates)
        assert np.array_equal(kind, kind_r), (case, gates, kind, kind_r)
        assert np.array_equal(idf, idf_r), (case, gates, idf, idf_r)
        ZF, ZN, idff = eng.data_associate(case.Z, case.R, *gates)
        assert np.array_equal(ZF, case.Z[:, kind_r == 1]) and np.array_equal(idff, idf_r[kind_r == 1]), (case, gates)
        if quirks == REF_EXACT:
            assert ZN.shape == (0, 0)
        else:
            assert np.array_equal(ZN, case.Z[:, kind_r == 2]), (case, gates)
    eng.close()


# ------------------------------------------------------------------------------------------------
# family G: the host side of associate
# ------------------------------------------------------------------------------------------------
def _fresh_answer(eng, case, gates, Z=None):
    """associate on a fresh handle loaded with eng's get_state()."""
    from conan_slam_amd import EKF

    X, P = eng.get_state()
    fresh = EKF((X.shape[0] - 3) // 2, dtype=case.dtype.type, quirks=eng.quirks)
    fresh.set_state(X, P)
    out = fresh.associate(case.Z if Z is None else Z, case.R, *gates)
    fresh.close()
    return out


def _own_obs(case, feats, dr=0.05):
    return np.asfortranarray(np.stack([predicted(case.X, f - 1, case.dtype) + [dr, 0.001] for f in feats], axis=1).astype(case.dtype))


@pytest.mark.parametrize("state", ["held_predict", "queued_heading", "pending_downdates"])
@pytest.mark.parametrize("nf", [65, 257])
def test_associate_meets_work_the_handle_holds_back(gpu_required, nf, state):
    """associate after a held predict, after predict + observe_heading queued, and under set_deferred(128) with two
    updates pending equals, exactly, the call on a fresh handle loaded with this one's get_state()."""
    case = get_case(("A", nf, "float32"))
    eng = _engine(case, TEXTBOOK)
    if state == "pending_downdates":
        eng.set_deferred(128)
        for feats in (np.arange(1, 9), np.arange(9, 17)):
            eng.update(_own_obs(case, feats), case.R, feats.astype(np.int32), batch=True)
    else:
        eng.predict(PREDICT[0], PREDICT[1], Q_CTRL, PREDICT[2], PREDICT[3])
        if state == "queued_heading":
            eng.observe_heading(float(case.X[2]) + 0.01, True)
    for gates in case.gates:
        idf, kind = eng.associate(case.Z, case.R, *gates)
        idf_f, kind_f = _fresh_answer(eng, case, gates)
        assert np.array_equal(idf, idf_f) and np.array_equal(kind, kind_f), (state, gates, idf, idf_f, kind, kind_f)
        assert (kind == 1).any()
    eng.close()


@pytest.mark.parametrize("nf", [65, 257])
def test_associate_with_m_growing_and_shrinking_on_one_handle(gpu_required, nf):
    """m = 1, then 40 (the output buffer grows), then 3: every call returns the builder's decisions of its columns."""
    case = get_case(("A", nf, "float32"))
    eng = _engine(case, REF_EXACT)
    gates = case.gates[0]
    idf_r, kind_r, _ = case.decisions(gates)
    for m in (1, 40, 3):
        cols = np.arange(m) % case.m if m != 3 else np.array([case.m - 1, 0, 5])
        idf, kind = eng.associate(np.asfortranarray(case.Z[:, cols]), case.R, *gates)
        assert np.array_equal(idf, idf_r[cols]) and np.array_equal(kind, kind_r[cols]), (m, idf, idf_r[cols])
    eng.close()


@pytest.mark.parametrize("nf", [65, 257])
def test_associate_after_the_map_grew(gpu_required, nf):
    """associate at nf - 1 features (the builder's case without its last landmark), augment one landmark (64 -> 65 and
    256 -> 257: a new chunk of the scan, and past the feature kernel's first workgroup), associate again: the per-feature
    buffer grows, and the answer equals a fresh handle's."""
    case = get_case(("A", nf, "float32"))
    from conan_slam_amd import EKF

    n0 = case.n - 2
    eng = EKF(nf, dtype=np.float32, quirks=TEXTBOOK)
    eng.set_state(case.X[:n0], np.asfortranarray(case.P[:n0, :n0]))
    gates = case.gates[0]
    idf0, kind0 = eng.associate(case.Z, case.R, *gates)
    assert np.array_equal(idf0, _fresh_answer(eng, case, gates)[0]) and idf0.max() <= nf - 1
    z_new = np.asfortranarray(case.Z[:, case.m - 1:case.m])
    eng.augment(z_new, case.R)
    assert eng.n == case.n
    # the new landmark sits exactly where the last observation puts it: that observation must now find it or a rival
    idf1, kind1 = eng.associate(case.Z, case.R, *gates)
    idf_f, kind_f = _fresh_answer(eng, case, gates)
    assert np.array_equal(idf1, idf_f) and np.array_equal(kind1, kind_f), (idf1, idf_f, kind1, kind_f)
    assert np.all(kind1 == 1)
    eng.close()


def test_associate_without_observations_returns_empty_arrays(gpu_required):
    case = get_case(("A", 65, "float32"))
    eng = _engine(case, REF_EXACT)
    idf, kind = eng.associate(np.zeros((2, 0), dtype=np.float32), case.R, 4.0, 25.0)
    assert idf.shape == (0,) and kind.shape == (0,)
    ZF, ZN, idff = eng.data_associate(np.zeros((2, 0), dtype=np.float32), case.R, 4.0, 25.0)
    assert ZF.shape == (2, 0) and idff.shape == (0,)
    # ... and the handle still answers afterwards
    idf, kind = eng.associate(case.Z, case.R, *case.gates[0])
    assert np.array_equal(idf, case.decisions(case.gates[0])[0])
    eng.close()
