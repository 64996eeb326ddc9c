"""CPU side of the particle filter's data association: the reference of pf_assoc_ref.py is DECISIVE on every case the GPU
file uses (each comparison that fixes an (idf, kind), duplicate claims included, has an f64 margin of at least the measured
tau, for EVERY particle and observation), the cases cover what they promise, deliberate faults of the rule change answers,
and the host-side policy `data_associate` does what it documents.  No device here."""
import numpy as np
import pytest

import pf_assoc_ref as ref
from pf_assoc_ref import ALL_KEYS, CASE_KEYS, case_id, get_case


@pytest.mark.parametrize("key", ALL_KEYS, ids=case_id)
def test_every_gpu_case_is_decisive(key):
    case = get_case(key)
    tau, err = case.tau()
    worst = min(case.margins(g).min() for g in case.gates)
    print(f"[decisive] {case}: tau {tau:.3e} (dtype error {err:.3e}), smallest margin {worst:.3e}")
    for g in case.gates:
        mg = case.margins(g)
        assert mg.shape == (case.m, case.np_)                      # no (particle, observation) is left out
        assert np.all(mg >= tau), (case, g, float(mg.min()), tau)
    assert tau < 0.1 * min(g[0] for g in case.gates), (case, tau)  # tau is small against the gates themselves
    case.check_twins()


@pytest.mark.parametrize("key", [k for k in CASE_KEYS if k[-1] == "float32"], ids=case_id)
def test_cloud_rule_equals_the_sequential_rule(key):
    """decide_cloud (vectorised) against assoc_builders.decide (the sequential loop of EKF.cpp:235-326) on particles 0, the
    middle one and the last."""
    case = get_case(key)
    if case.nf == 0:
        return
    nis, nd = case.ref()
    for g in case.gates:
        idf, kind, _ = case.raw(g)
        for p in sorted({0, case.np_ // 2, case.np_ - 1}):
            i1, k1, _ = ref.decide(nis[p], nd[p], *g)
            assert np.array_equal(i1, idf[:, p]) and np.array_equal(k1, kind[:, p]), (case, g, p)


def _changed(case, idf, kind):
    return any(not (np.array_equal(idf[g], case.decisions(g)[0]) and np.array_equal(kind[g], case.decisions(g)[1]))
               for g in case.gates)


def _with(case, **faults):
    nis, nd = case.ref(**faults)
    out = {g: ref.resolve_duplicates(*ref.decide_cloud(nis, nd, *g)) for g in case.gates}
    return {g: o[0] for g, o in out.items()}, {g: o[1] for g, o in out.items()}


def _sequential(case, fault):
    nis, nd = case.ref()
    idf, kind = {}, {}
    for g in case.gates:
        raw_i, raw_k, nb = (np.zeros((case.m, case.np_), np.int32), np.zeros((case.m, case.np_), np.int32),
                            np.full((case.m, case.np_), np.inf))
        for p in range(case.np_):
            i1, k1, _ = ref.decide(nis[p], nd[p], *g, fault=fault)
            raw_i[:, p], raw_k[:, p] = i1, k1
            nb[:, p] = [nd[p, j, i1[j] - 1] if i1[j] else np.inf for j in range(case.m)]
        idf[g], kind[g] = ref.resolve_duplicates(raw_i, raw_k, nb)
    return idf, kind


def test_negative_controls_change_answers():
    """Each deliberate fault changes at least one (idf, kind) in at least one case: the cases can tell them apart."""
    ties, dense = get_case(("B", "float32")), get_case(("A", 65, 2 * ref.C + 3, 33, "float32"))
    wrap, dups, gates = get_case(("D", "float32")), get_case(("E", "float32")), get_case(("C0", "float32"))
    assert _changed(ties, *_sequential(ties, "inclusive"))                 # `<=` in the record test
    assert _changed(ties, *_sequential(ties, "last_tie"))                  # the last index among equal minima
    nis, nd = dense.ref()
    on_nd = {g: ref.resolve_duplicates(*ref.decide_cloud(nis, nd, *g, gate_on_nd=True)) for g in dense.gates}
    assert _changed(dense, {g: o[0] for g, o in on_nd.items()}, {g: o[1] for g, o in on_nd.items()})   # gate applied to nd
    assert _changed(gates, *_with(gates, drop_pose=True)) or _changed(dense, *_with(dense, drop_pose=True))   # HV Pv HV^T
    assert _changed(wrap, *_with(wrap, no_wrap=True))                      # no bearing wrap
    unresolved_i = {g: dups.raw(g)[0] for g in dups.gates}                 # duplicates left unresolved
    unresolved_k = {g: dups.raw(g)[1] for g in dups.gates}
    assert _changed(dups, unresolved_i, unresolved_k)


def test_families_cover_what_they_promise():
    C = ref.C
    # A: several features inside gate1 for many (particle, observation) pairs, winners in every chunk of the scan
    dense = get_case(("A", 65, 2 * C + 3, 33, "float32"))
    nis = dense.ref()[0]
    assert ((nis < dense.gates[0][0]).sum(axis=2) >= 2).mean() > 0.4
    winners = set(np.unique(dense.decisions(dense.gates[0])[0])) - {0}
    assert {(w - 1) // C for w in winners} == {0, 1, 2}
    # B: the first twin wins wherever the group wins, in one chunk, across the boundary and chunks apart
    ties = get_case(("B", "float32"))
    for g in ties.gates:
        raw = ties.raw(g)[0]
        later = {t + 1 for grp in ties.twins for t in grp[1:]}
        assert not (set(np.unique(raw)) & later), (g, np.unique(raw))
        assert {grp[0] + 1 for grp in ties.twins} <= set(np.unique(raw))
    assert any(grp[0] // C != grp[-1] // C for grp in ties.twins) and any(grp[0] // C == grp[1] // C for grp in ties.twins)
    # C: one isolated feature 4 TAU_SEARCH under / over gate1 and gate2, the same for every (identical) particle
    for key, g in [((fam, dt), ref.GATES[int(fam[1])]) for fam in ("C0", "C1") for dt in ("float32", "float64")]:
        c = get_case(key)
        idf, kind = c.decisions(g)
        assert np.all(kind == np.array([1, 0, 0, 2])[:, None]) and np.all(idf[1:] == 0) and np.all(idf[0] == 1), (c, kind[:, 0])
        d = 4.0 * ref.TAU_SEARCH[c.dtype]
        near = np.sort(c.ref()[0][0], axis=1)[:, 0]
        assert np.allclose(near, [g[0] - d, g[0] + d, g[1] - d, g[1] + d], rtol=0, atol=0.1 * d), (c, near)
    # D: predicted bearings on both sides of the cut, raw innovations beyond pi, everything still matched
    for dt in ("float32", "float64"):
        c = get_case(("D", dt))
        Xv, XF = c.Xv.astype(np.float64), c.XF.astype(np.float64)
        zb = np.arctan2(XF[:, 1, 0] - Xv[:, 1], XF[:, 0, 0] - Xv[:, 0]) - Xv[:, 2]
        zb = np.asarray(ref.pi2pi(zb))
        assert (zb > 3.0).any() and (zb < -3.0).any(), (c, zb.min(), zb.max())
        rawinn = c.Z.astype(np.float64)[1][None, :] - zb[:, None]
        assert (np.abs(rawinn) > np.pi).mean() > 0.25
        assert all(np.all(c.raw(g)[1] == 1) for g in c.gates)
    # E: two and three observations of one particle claim one feature; an exact repeat loses to the lower index
    for dt in ("float32", "float64"):
        c = get_case(("E", dt))
        g = c.gates[0]
        raw = c.raw(g)[0]
        claims = [np.bincount(raw[:, p][raw[:, p] > 0], minlength=c.nf + 2).max() for p in range(c.np_)]
        assert max(claims) >= 4 and np.mean(np.array(claims) >= 3) > 0.5, claims
        idf = c.decisions(g)[0]
        assert np.all(idf[-1] == 0) and np.array_equal(raw[-1], raw[0])
        for p in range(c.np_):
            kept = idf[:, p][idf[:, p] > 0]
            assert len(set(kept)) == len(kept)
    # F: the NaN feature is inside gate1 and never wins; where nothing else is gated the observation is dropped
    for dt in ("float32", "float64"):
        c = get_case(("F", dt))
        nis, nd = c.ref()
        for f in (ref.F_BAD, ref.F_LONE):
            assert np.all(np.isnan(nd[:, :, f]))
        assert not np.isnan(np.delete(nd, [ref.F_BAD, ref.F_LONE], axis=2)).any()
        for g in c.gates:
            idf, kind = c.decisions(g)
            assert not np.isin(idf, [ref.F_BAD + 1, ref.F_LONE + 1]).any()
            assert (nis[:, :3, ref.F_BAD] < g[0]).mean() > 0.9       # ahead of the winner (lower index) and gated
            assert (c.raw(g)[0][:3] == ref.F_WIN + 1).mean() > 0.9
            assert np.all(nis[:, 3:, ref.F_LONE] < g[0]) and np.all(idf[3:] == 0) and np.all(kind[3:] == 0)
    # the consumers' cases: uniform complete tables; the whole step adds three observations that are new for everybody
    for key in ref.UNIFORM_KEYS + ref.STEP_KEYS:
        c = get_case(key)
        m, n_new = key[3], key[4]
        for g in c.gates:
            idf, kind = c.decisions(g)
            assert np.all(idf == idf[:, :1]) and len(set(idf[:m, 0])) == m and np.all(kind[:m] == 1), c
            assert np.all(kind[m:] == 2) and c.m == m + n_new, c
    # the cross-check against the EKF has no duplicate claims
    for key in ref.EKF_KEYS:
        c = get_case(key)
        assert c.np_ == 1 and all(np.array_equal(c.raw(g)[0], c.decisions(g)[0]) for g in c.gates), c
        assert ((c.ref()[0] < c.gates[0][0]).sum(axis=2) >= 2).any(), c
    # the mixed tables have unmatched entries and matched ones in most particles
    for key in ref.MIXED_KEYS:
        c = get_case(key)
        idf = c.decisions(c.gates[0])[0]
        assert key in CASE_KEYS and (idf == 0).any() and (idf != 0).mean() > 0.4, c
    # the empty map
    c = get_case(("A", 65, 0, ref.OBS_CHUNK + 1, "float32"))
    assert all(np.all(c.decisions(g)[1] == 2) and np.all(c.decisions(g)[0] == 0) for g in c.gates)


def test_sizes_cover_every_path():
    C, OC = ref.C, ref.OBS_CHUNK
    keys = [k for k in CASE_KEYS if k[0] == "A"]
    assert {k[1] for k in keys} == {1, 63, 64, 65, 130}
    assert {k[2] for k in keys} == {0, 1, C - 1, C, C + 1, 2 * C + 3}
    assert {1, OC, OC + 1, 33, 64} <= {k[3] for k in keys}
    assert {k[-1] for k in keys} == {"float32", "float64"}
    from conan_slam_amd import _capi

    assert (_capi.PF_ASSOC_FEAT_CHUNK, _capi.PF_ASSOC_OBS_CHUNK) == (C, OC)
    src = open(_capi.HEADER_PATH.replace("include/cslam.h", "conan_slam_amd/csrc/pf_assoc_kernels.hpp")).read()
    assert f"kPfAssocFeatChunk = {C};" in src and f"kPfAssocObsChunk = {OC};" in src


def test_summary_reference_adds_up():
    c = get_case(("A", 65, 2 * ref.C + 3, 33, "float32"))
    s = c.summary(c.gates[0])
    assert np.allclose(s[:, :3].sum(axis=1), c.w.astype(np.float64).sum(), rtol=1e-14)
    assert np.array_equal(s[:, 3], (c.decisions(c.gates[0])[1] == 1).sum(axis=1))


class _FakeShard:
    """Stands in for ParticleShard in the policy test: records the call, returns a synthetic summary."""
    dtype = np.dtype(np.float32)

    def __init__(self, summary):
        self.summary, self.called = np.asarray(summary, dtype=np.float64), None

    def associate(self, Z, R, g1, g2):
        self.called = (np.asarray(Z).shape, g1, g2)

    def association(self):
        return None, None, self.summary


def test_data_associate_policy():
    from conan_slam_amd import pf

    Z = np.asfortranarray(np.arange(10, dtype=np.float32).reshape(2, 5, order="F"))
    #            matched new   ambiguous count
    summary = [[0.9, 0.1, 0.0, 9],      # matched by nearly everybody: used
               [0.1, 0.9, 0.0, 1],      # new for nearly everybody: a new feature
               [0.5, 0.5, 0.0, 5],      # exactly the fraction: new (>=)
               [0.3, 0.3, 0.4, 3],      # 0.3 of the mass says new: used
               [0.0, 0.0, 1.0, 0]]      # ambiguous for everybody: used (every particle pays miss_likelihood)
    sh = _FakeShard(summary)
    use, ZN = pf.data_associate(sh, Z, np.eye(2), 4.0, 25.0)
    assert sh.called == ((2, 5), 4.0, 25.0)
    assert use.dtype == np.int32 and use.tolist() == [1, 0, 0, 1, 1]
    assert np.array_equal(ZN, Z[:, [1, 2]]) and ZN.flags.f_contiguous
    use, ZN = pf.data_associate(sh, Z, np.eye(2), 4.0, 25.0, new_fraction=0.25)
    assert use.tolist() == [1, 0, 0, 0, 1] and ZN.shape == (2, 3)
    use, ZN = pf.data_associate(sh, Z, np.eye(2), 4.0, 25.0, new_fraction=0.95)
    assert use.tolist() == [1, 1, 1, 1, 1] and ZN.shape == (2, 0)
    # no weight mass, or nobody calling it new: never new, even with new_fraction = 0
    assert pf.new_feature_votes(np.zeros((2, 4))).tolist() == [False, False]
    assert pf.new_feature_votes(np.array([[1.0, 0.0, 0.0, 4], [0.5, 0.25, 0.25, 2]]), new_fraction=0.0).tolist() == [False, True]
    # unnormalised weights: the fraction is of the mass present
    assert pf.new_feature_votes(np.array([[1.0, 3.0, 0.0, 1], [3.0, 1.0, 0.0, 3]])).tolist() == [True, False]
    use, ZN = pf.data_associate(_FakeShard(np.zeros((0, 4))), np.zeros((2, 0), np.float32), np.eye(2), 4.0, 25.0)
    assert use.shape == (0,) and ZN.shape == (2, 0)


def test_new_symbols_are_declared_and_bound():
    from conan_slam_amd import _capi

    names = _capi.declared_symbols()
    for sym in ("cslam_pf_associate", "cslam_pf_get_association", "cslam_pf_sample_proposal_assoc",
                "cslam_pf_feature_update_assoc"):
        assert sym in names and sym in _capi.PF_ASSOC_SYMBOLS
    text = open(_capi.HEADER_PATH).read()
    assert text.count("EKF.cpp:131-144, 235-326") >= 4
