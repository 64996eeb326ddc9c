"""cslam_pf_associate and the consumers of its per-particle table on the device.

Every case of pf_assoc_ref.py is DECISIVE for every (particle, observation): each comparison that fixes an (idf, kind),
duplicate claims included, has a margin in the f64 reference of at least 64 x the error of a numpy evaluation in the case's
dtype (test_pf_assoc_cpu.py proves it).  That makes equality of integers the right assertion here.
  A  dense clusters at every size at which the scan / merge / resolve kernels take another path
  B  exact ties between twin features: the lower index wins, inside a chunk of the scan and across chunks (the merge)
  C  one feature just under / over gate1 and gate2
  D  bearings on both sides of +-pi
  E  two and three observations of a particle claim one feature; an exact repeat
  F  a feature whose nd is NaN
then the growth of the handle's tables, the EKF's own associate on one particle, the consumers bit for bit on uniform
complete tables and against the per-particle oracle restatement on mixed ones, one whole step, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import pf_assoc_ref as ref
from pf_assoc_ref import CASE_KEYS, case_id, get_case
from pf_builders import PREDICT, Q_CTRL, TOL, assert_weights_fair, compare

pytestmark = pytest.mark.gpu

MISS = 1e-3


def upload(case, nfcap=None, parts=None):
    from conan_slam_amd._capi import check
    from conan_slam_amd.pf import ParticleShard

    parts = case.parts if parts is None else parts
    sh = ParticleShard(case.np_, max(case.nf, 1) if nfcap is None else nfcap, dtype=case.dtype.type)
    for i, (w, Xv, Pv, XF, PF) in enumerate(parts):
        if case.nf:
            sh.set_particle(i, w, Xv, Pv, XF, PF)
        else:   # an empty map
            wv, Xc = np.array([w], case.dtype), np.ascontiguousarray(Xv, case.dtype)
            Pc = np.asfortranarray(np.asarray(Pv, case.dtype).reshape(3, 3))
            check(sh._L.cslam_pf_set_particle(sh._h, C.c_int(i), wv.ctypes.data_as(C.c_void_p), Xc.ctypes.data_as(C.c_void_p),
                                              Pc.ctypes.data_as(C.c_void_p), None, None, C.c_int(0)))
    return sh


def check_tables(sh, case, gates, tag=""):
    idf_r, kind_r = case.decisions(gates)
    sh.associate(case.Z, case.R, *gates)
    idf, kind, summary = sh.association()
    bad = np.argwhere((idf != idf_r) | (kind != kind_r))
    assert bad.shape[0] == 0, (tag, case, gates, bad[:5].tolist(), [(int(idf[j, p]), int(idf_r[j, p]), int(kind[j, p]),
                                                                     int(kind_r[j, p])) for j, p in bad[:5]])
    s_r = case.summary(gates)
    assert np.array_equal(summary[:, 3], s_r[:, 3]), (tag, case)
    assert np.all(np.abs(summary[:, :3] - s_r[:, :3]) <= 1e-12 * np.abs(s_r[:, :3])), (tag, case, summary, s_r)
    return idf, kind, summary


@pytest.mark.parametrize("key", CASE_KEYS, ids=case_id)
def test_associate_returns_the_decisive_reference(gpu_required, key):
    case = get_case(key)
    sh = upload(case)
    for gates in case.gates:
        first = check_tables(sh, case, gates)
        again = check_tables(sh, case, gates, "second call")
        assert all(np.array_equal(a, b) for a, b in zip(first, again)), (case, gates)
    sh.close()


def test_tables_regrow_with_a_larger_m(gpu_required):
    """9 observations, then 70 (more than the tables were first sized for), then the 9 again, on one handle."""
    small, big = get_case(("G9", "float32")), get_case(("G70", "float32"))
    sh = upload(big)
    for case in (small, big, small):
        check_tables(sh, case, case.gates[0])
    sh.close()


@pytest.mark.parametrize("key", ref.EKF_KEYS, ids=case_id)
def test_one_particle_agrees_with_the_ekf(gpu_required, key):
    """cslam_ekf_associate on P = blockdiag(Pv, PF_1, ...) and cslam_pf_associate on the particle return the same."""
    from conan_slam_amd import EKF

    case = get_case(key)
    n = 3 + 2 * case.nf
    X = np.concatenate([case.Xv[0], case.XF[0].T.reshape(-1)]).astype(case.dtype)
    P = np.zeros((n, n), case.dtype, order="F")
    P[:3, :3] = case.Pv[0]
    for f in range(case.nf):
        P[3 + 2 * f: 5 + 2 * f, 3 + 2 * f: 5 + 2 * f] = case.PF[0, :, f].reshape(2, 2, order="F")
    ekf = EKF(case.nf, dtype=case.dtype.type)
    ekf.set_state(X, P)
    sh = upload(case)
    for gates in case.gates:
        idf_e, kind_e = ekf.associate(case.Z, case.R, *gates)
        idf, kind, _ = check_tables(sh, case, gates)
        assert np.array_equal(idf[:, 0], idf_e) and np.array_equal(kind[:, 0], kind_e), (case, gates, idf[:, 0], idf_e)
    ekf.close()
    sh.close()


def _fields(sh, n):
    return [sh.get_particle(i) for i in range(n)]


def _assert_bitwise(a, b, tag):
    for i, (pa, pb) in enumerate(zip(a, b)):
        for name, x, y in zip(("w", "Xv", "Pv", "XF", "PF"), pa, pb):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (tag, i, name, x, y)


@pytest.mark.parametrize("key", ref.UNIFORM_KEYS, ids=case_id)
def test_uniform_complete_table_is_bitwise_the_known_association_path(gpu_required, key):
    """Every particle holds the same complete idf and use is all ones: sample_proposal_assoc leaves every field of every
    particle bitwise equal to sample_proposal + feature_update on a twin shard; so does the unfused pair
    sample_proposal + feature_update_assoc; so does feature_update_assoc alone against feature_update alone."""
    case = get_case(key)
    gates = case.gates[0]
    idf = case.decisions(gates)[0][:, 0].astype(np.int32)
    normals = np.random.default_rng(5).normal(size=(3, case.np_)).astype(case.dtype)
    twin = upload(case)
    twin.sample_proposal(case.Z, idf, case.R, normals)
    twin.feature_update(case.Z, idf, case.R)
    want = _fields(twin, case.np_)
    twin.close()

    fused = upload(case)
    check_tables(fused, case, gates)
    fused.sample_proposal_assoc(case.Z, case.R, normals, np.ones(case.m, np.int32), MISS)
    _assert_bitwise(_fields(fused, case.np_), want, "fused")
    fused.close()

    pair = upload(case)
    pair.associate(case.Z, case.R, *gates)
    pair.sample_proposal(case.Z, idf, case.R, normals)
    pair.feature_update_assoc(case.Z, case.R)
    _assert_bitwise(_fields(pair, case.np_), want, "unfused pair")
    pair.close()

    alone, twin = upload(case), upload(case)
    alone.associate(case.Z, case.R, *gates)
    alone.feature_update_assoc(case.Z, case.R, np.ones(case.m, np.int32))
    twin.feature_update(case.Z, idf, case.R)
    _assert_bitwise(_fields(alone, case.np_), _fields(twin, case.np_), "feature update alone")
    alone.close()
    twin.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "feature_update_only"])
@pytest.mark.parametrize("key", ref.MIXED_KEYS, ids=case_id)
def test_mixed_tables_match_the_per_particle_oracle(gpu_required, key, fused):
    """Per-particle tables with unmatched entries and a mask with holes, after a predict (a positive-definite Pv for
    everybody): poses, features and weights against each particle's own oracle run (pf_assoc_ref.consumer_reference, fed
    with the table the device returned), tolerances of pf_builders.TOL and the weight rule of assert_weights_fair."""
    case = get_case(key)
    dt = case.dtype.type
    gates = case.gates[0]
    sh = upload(case)
    sh.predict(PREDICT[0], PREDICT[1], Q_CTRL, PREDICT[2], PREDICT[3])
    sh.associate(case.Z, case.R, *gates)
    idf, kind, _ = sh.association()
    assert (idf == 0).any() and (idf != 0).any(), case
    use = np.ones(case.m, np.int32)
    use[1::4] = 0
    normals = np.random.default_rng(6).normal(size=(3, case.np_)).astype(dt)
    if fused:
        sh.sample_proposal_assoc(case.Z, case.R, normals, use, MISS)
    else:
        sh.feature_update_assoc(case.Z, case.R, use)
    start = ref.predicted_parts(case.parts, dt)
    want = ref.consumer_reference(start, dt, case.Z, case.R, idf, use, normals, MISS, proposal=fused)
    compare(sh, want, dt, f"{case} fused={fused}", wtol=np.inf)
    if fused:
        hi = ref.consumer_reference(ref.predicted_parts(case.parts, np.float64), np.float64, case.Z, case.R, idf, use,
                                    normals, MISS)
        wg = [sh.get_particle(i)[0] for i in range(case.np_)]
        assert_weights_fair(str(case), wg, [p[0] for p in want], [p[0] for p in hi], dt)
        # a particle with unmatched used observations has paid for them
        unmatched = ((idf == 0) & (use[:, None] == 1)).sum(axis=0)
        assert unmatched.max() > 0
    else:
        wg = np.array([sh.get_particle(i)[0] for i in range(case.np_)])
        assert np.array_equal(wg, case.w), case      # the unfused feature update touches no weight
    sh.close()


@pytest.mark.parametrize("key", ref.STEP_KEYS, ids=case_id)
def test_one_step_with_unknown_associations(gpu_required, key):
    """associate -> data_associate (the host policy) -> sample_proposal_assoc -> resample_local -> add_features(ZN) on 130
    particles and 20 features; three observations are of unmapped landmarks.  The map grows by 3 and the estimate agrees
    with the same step run with known associations."""
    from conan_slam_amd import pf

    case = get_case(key)
    dt = case.dtype.type
    gates = case.gates[0]
    m, n_new = key[3], key[4]
    idf_known = case.decisions(gates)[0][:m, 0].astype(np.int32)
    rng = np.random.default_rng(8)
    normals = rng.normal(size=(3, case.np_)).astype(dt)
    select = pf.stratified_random(case.np_, rng.uniform(size=case.np_), dt)
    sh = upload(case, nfcap=case.nf + n_new)
    use, ZN = pf.data_associate(sh, case.Z, case.R, *gates)
    assert use.tolist() == [1] * m + [0] * n_new and np.array_equal(ZN, case.Z[:, m:])
    idf, kind, summary = sh.association()
    assert np.array_equal(idf, case.decisions(gates)[0]) and np.array_equal(kind, case.decisions(gates)[1])
    sh.sample_proposal_assoc(case.Z, case.R, normals, use, MISS)
    sh.resample_local(select, case.np_, True)
    sh.add_features(ZN, case.R)
    assert sh.n_features == case.nf + n_new

    known = upload(case, nfcap=case.nf + n_new)
    known.sample_proposal(case.Z[:, :m], idf_known, case.R, normals)
    known.feature_update(case.Z[:, :m], idf_known, case.R)
    known.resample_local(select, case.np_, True)
    known.add_features(case.Z[:, m:], case.R)
    a, b = sh.estimate(), known.estimate()
    tol = TOL[case.dtype]
    for name in ("Xv", "Pv", "XF", "PF"):
        x, y = np.asarray(getattr(a, name), np.float64), np.asarray(getattr(b, name), np.float64)
        assert np.all(np.isfinite(x)) and np.abs(x - y).max() <= tol * max(1.0, np.abs(y).max()), (case, name)
    assert abs(a.w_sum - b.w_sum) <= tol * abs(b.w_sum) and abs(a.neff - b.neff) <= tol * b.neff
    sh.close()
    known.close()


def test_argument_errors(gpu_required):
    from conan_slam_amd import CslamError, _capi

    case = get_case(("U", 17, 30, 9, 0, "float32"))
    sh = upload(case)
    L, h = sh._L, sh._h
    Z, R = np.ascontiguousarray(case.Z.reshape(-1, order="F")), np.asfortranarray(case.R)
    zp, rp = Z.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p)
    normals = np.zeros((3, case.np_), np.float32)
    use = np.ones(case.m, np.int32)

    def code(fn):
        with pytest.raises(CslamError) as ei:
            fn()
        assert str(ei.value).strip() != "", "cslam_last_error carries a text"
        return ei.value.code

    # before any associate
    assert code(sh.association) == _capi.ERR_BAD_ARG
    assert code(lambda: _capi.check(L.cslam_pf_get_association(h, None, None, None))) == _capi.ERR_BAD_ARG
    assert code(lambda: sh.sample_proposal_assoc(case.Z, case.R, normals, use, MISS)) == _capi.ERR_BAD_ARG
    assert code(lambda: sh.feature_update_assoc(case.Z, case.R, use)) == _capi.ERR_BAD_ARG
    # associate itself
    assert code(lambda: _capi.check(L.cslam_pf_associate(h, zp, C.c_int(-1), rp, C.c_double(4.0), C.c_double(25.0)))) == _capi.ERR_BAD_ARG
    assert code(lambda: sh.associate(case.Z, case.R, np.inf, 25.0)) == _capi.ERR_BAD_ARG
    assert code(lambda: sh.associate(case.Z, case.R, 4.0, np.nan)) == _capi.ERR_BAD_ARG
    assert code(lambda: _capi.check(L.cslam_pf_associate(None, zp, C.c_int(1), rp, C.c_double(4.0), C.c_double(25.0)))) == _capi.ERR_BAD_ARG
    assert code(sh.association) == _capi.ERR_BAD_ARG     # none of the refused calls counts
    sh.associate(case.Z, case.R, *case.gates[0])
    _capi.check(L.cslam_pf_get_association(h, None, None, None))   # all three pointers may be NULL
    # the consumers take the observations of the last associate
    other = case.Z.copy()
    other[0, 0] += 1.0
    assert code(lambda: sh.sample_proposal_assoc(other, case.R, normals, use, MISS)) == _capi.ERR_BAD_ARG
    assert code(lambda: sh.sample_proposal_assoc(case.Z[:, :-1], case.R, normals, use[:-1], MISS)) == _capi.ERR_BAD_ARG
    assert code(lambda: sh.feature_update_assoc(other, case.R, use)) == _capi.ERR_BAD_ARG
    bad_use = use.copy()
    bad_use[2] = 2
    assert code(lambda: sh.sample_proposal_assoc(case.Z, case.R, normals, bad_use, MISS)) == _capi.ERR_BAD_ARG
    assert code(lambda: sh.sample_proposal_assoc(case.Z, case.R, normals, use, np.nan)) == _capi.ERR_BAD_ARG
    # ... and none of the refusals disturbed the table
    assert np.array_equal(sh.association()[0], case.decisions(case.gates[0])[0])
    # the table is per particle slot: once particles may have moved the consumers refuse it until the next associate
    select = np.linspace(0.0, 1.0, case.np_, endpoint=False, dtype=np.float32) + np.float32(0.5 / case.np_)
    w, Xv, Pv, XF, PF = sh.get_particle(0)
    for move in (lambda: sh.resample_local(select, case.np_ + 1, True), lambda: sh.set_particle(0, w, Xv, Pv, XF, PF)):
        sh.associate(case.Z, case.R, *case.gates[0])
        sh.feature_update_assoc(case.Z, case.R, np.zeros(case.m, np.int32))   # accepted (and masks everything)
        move()
        assert code(lambda: sh.sample_proposal_assoc(case.Z, case.R, normals, use, MISS)) == _capi.ERR_BAD_ARG
        assert code(lambda: sh.feature_update_assoc(case.Z, case.R, use)) == _capi.ERR_BAD_ARG
        sh.association()                                                     # the tables themselves can still be read
    # a refused associate leaves the wrapper nothing to size its buffers from
    sh.associate(case.Z, case.R, *case.gates[0])
    assert code(lambda: sh.associate(case.Z, case.R, np.inf, 25.0)) == _capi.ERR_BAD_ARG
    assert code(sh.association) == _capi.ERR_BAD_ARG
    # m = 0 is a valid (empty) association
    sh.associate(np.zeros((2, 0), np.float32), case.R, 4.0, 25.0)
    idf, kind, summary = sh.association()
    assert idf.shape == (0, case.np_) and summary.shape == (0, 4)
    sh.close()
