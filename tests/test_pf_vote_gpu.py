"""The vote on new features kept on the device (cslam_pf_associate_vote and the calls that consume it).

The vote kernel reads the very doubles the host policy reads -- the summary cslam_pf_associate left in HBM -- so every
comparison here is exact: use, new_idx, ZN and q against pf.new_feature_votes applied to association().summary, the _voted
consumers against the _assoc consumers fed the host policy's mask, the one-call scan against the separate calls, the
sharded vote against the shards' summaries added in rank order.  The clouds need not be decisive for that: whatever the
per-particle tables are, both sides read the same ones."""
import ctypes as C

import numpy as np
import pytest

import pf_assoc_ref as ref
import pf_drive_ref as D
import pf_vote_ref as V
from pf_builders import DTYPES, PREDICT, Q_CTRL

pytestmark = pytest.mark.gpu

GATES = (4.0, 25.0)
MISS = 1e-3
FRACTIONS = V.FRACTIONS  # 0, 0.5, 1, 1.5
# (np, nf, m): every np and nf at which the association kernels take another path, every m at a wave (64) or tile (256)
# edge of the compaction and at the 32-observation edge of the drawn staging; nf = 0 makes everything new (q = m)
SHAPES = [(1, 0, 1), (63, 1, 8), (64, 32, 9), (65, 33, 33), (130, 70, 64), (65, 32, 65), (63, 33, 255), (64, 70, 256),
          (130, 1, 257), (65, 70, 600), (130, 0, 257), (1, 33, 600), (64, 0, 65)]


def _cloud(np_, nf, dtype, seed, m):
    """A clustered cloud and m observations of mixed fate: near a feature (most particles match it), between features
    (ambiguous for many), far from all (new for everybody), and 4 - 8 m short of or beyond a feature, where the share of
    the cloud that calls the observation new takes every value between 0 and 1 (measured on the f64 reference)."""
    dt = np.dtype(dtype).type
    parts, base = ref.cluster_cloud(np_, nf, dt, seed)
    rng = np.random.default_rng(seed + 77)
    cols = []
    for j in range(m):
        kind = j % 4 if nf else 2
        if kind == 2:
            cols.append([rng.uniform(60.0, 90.0), rng.uniform(-3.0, 3.0)])
        elif kind == 3:
            z = ref.measure(base, int(rng.integers(nf)))
            cols.append(z + np.array([rng.uniform(4.0, 8.0) * rng.choice([-1.0, 1.0]), rng.normal() * 0.005]))
        else:
            z = ref.measure(base, int(rng.integers(nf)))
            cols.append(z + rng.normal(size=2) * ((0.2, 0.005) if kind == 0 else (1.2, 0.04)))
    Z = np.asfortranarray(np.array(cols, dtype=np.float64).T.reshape(2, m).astype(dtype))
    return parts, Z


def _upload(parts, np_, nf, dtype, nfcap=None, n_global=None):
    from conan_slam_amd._capi import check
    from conan_slam_amd.pf import ParticleShard

    dtype = np.dtype(dtype)
    sh = ParticleShard(np_, max(nf, 1) if nfcap is None else nfcap, dtype=dtype.type, n_global=n_global)
    for i, (w, Xv, Pv, XF, PF) in enumerate(parts):
        if nf:
            sh.set_particle(i, w, Xv, Pv, XF, PF)
        else:
            wv, Xc = np.array([w], dtype), np.ascontiguousarray(Xv, dtype)
            Pc = np.asfortranarray(np.asarray(Pv, dtype).reshape(3, 3))
            check(sh._L.cslam_pf_set_particle(sh._h, C.c_int(i), wv.ctypes.data_as(C.c_void_p), Xc.ctypes.data_as(C.c_void_p),
                                              Pc.ctypes.data_as(C.c_void_p), None, None, C.c_int(0)))
    return sh


def _records(sh):
    from test_pf_edges_gpu import _bulk_read

    return _bulk_read(sh)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _device_vote(sh, m):
    use, idx, ZN, q = sh.vote()
    return V.Vote(use, idx, ZN, q, (q, m))


def _check_vote(sh, Z, R, f, tag):
    """associate_vote, then vote() and vote_wait() against the host policy on association().summary -> the Vote."""
    m = Z.shape[1]
    sh.associate_vote(Z, R, *GATES, f)
    q_wait, use_wait = sh.vote_wait()
    got = _device_vote(sh, m)
    _, _, summary = sh.association()
    want = V.host_policy(summary, Z, f)
    assert V.same(got, want), (tag, f, got.q, want.q, got.use.tolist()[:16], want.use.tolist()[:16])
    assert V.same(got, V.vote(summary, Z, f)), (tag, f, "the restatement")
    assert q_wait == got.q and np.array_equal(use_wait, got.use), (tag, f, "vote_wait")
    assert sh.vote_wait()[0] == got.q, (tag, "a second wait")
    return got


# ------------------------------------------------------------------------------------------------ 1. vote = host policy
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "np%d-nf%d-m%d" % s)
def test_vote_is_the_host_policy(gpu_required, shape, dtype):
    np_, nf, m = shape
    parts, Z = _cloud(np_, nf, dtype, 100 * np_ + nf + m, m)
    R = ref.R_OBS.astype(dtype)
    sh = _upload(parts, np_, nf, dtype)
    try:
        qs = []
        for f in FRACTIONS:
            tag = (shape, np.dtype(dtype).name)
            first = _check_vote(sh, Z, R, f, tag)
            again = _check_vote(sh, Z, R, f, tag)
            assert V.same(first, again), (tag, f, "a second call")
            qs.append(first.q)
            if nf == 0:
                assert first.q == (m if f <= 1.0 else 0), (tag, f, first.q)
        print(f"[vote] np {np_} nf {nf} m {m} {np.dtype(dtype).name}: q per fraction {dict(zip(FRACTIONS, qs))}")
        assert qs[0] >= qs[1] >= qs[2] >= qs[3] == 0
        if nf and m >= 8:
            assert 0 < qs[1] < m, (shape, qs)  # the scan is mixed: the compaction has holes to close
    finally:
        sh.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_vote_extra_cases(gpu_required, dtype):
    dt = np.dtype(dtype)
    # an all-matched scan: q = 0
    case = ref.get_case(("U", 17, 30, 9, 0, dt.name))
    sh = _upload(case.parts, case.np_, case.nf, dtype)
    try:
        got = _check_vote(sh, case.Z, case.R, 0.5, "all matched")
        assert got.q == 0 and got.use.tolist() == [1] * case.m
        # a set with all weights zero: nothing is new, not even with new_fraction = 0
        sh.set_weights(np.zeros(case.np_, dtype))
        for f in (0.0, 0.5):
            assert _check_vote(sh, case.Z, case.R, f, "no mass").q == 0
    finally:
        sh.close()
    parts, Z = _cloud(65, 0, dtype, 5, 9)
    sh = _upload(parts, 65, 0, dtype)
    try:
        sh.set_weights(np.zeros(65, dtype))
        assert _check_vote(sh, Z, ref.R_OBS.astype(dtype), 0.0, "no mass, empty map").q == 0
    finally:
        sh.close()
    # equality: np = 4, uniform weights 1/4 (exact), exactly two particles call the observation new
    t = dt.type
    parts = []
    for i in range(4):
        XF = np.array([[10.0], [0.0 if i < 2 else 30.0]], dtype=dtype, order="F")
        PF = np.array([[0.01], [0.0], [0.0], [0.01]], dtype=dtype, order="F")
        parts.append([t(0.25), np.zeros(3, dtype), np.asfortranarray(np.eye(3, dtype=dtype) * t(1e-4)), XF, PF])
    Z = np.array([[10.0], [0.0]], dtype=dtype, order="F")
    sh = _upload(parts, 4, 1, dtype)
    try:
        got = _check_vote(sh, Z, ref.R_OBS.astype(dtype), 0.5, "equality")
        _, kind, summary = sh.association()
        assert kind.tolist() == [[1, 1, 2, 2]] and summary.tolist() == [[0.5, 0.5, 0.0, 2.0]]
        assert got.q == 1 and got.use.tolist() == [0] and got.new_idx.tolist() == [0] and _bits(got.ZN, Z)
        assert _check_vote(sh, Z, ref.R_OBS.astype(dtype), float(np.nextafter(0.5, 1.0)), "just above equality").q == 0
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------ 2. consumers bit for bit
def _pair(np_, nf, m, dtype, seed):
    parts, Z = _cloud(np_, nf, dtype, seed, m)
    a, b = (_upload(parts, np_, nf, dtype, nfcap=nf + m) for _ in range(2))
    for sh in (a, b):
        sh.seed_draws(11)
        sh.predict(PREDICT[0], PREDICT[1], Q_CTRL, PREDICT[2], PREDICT[3])  # a positive-definite Pv for everybody
    return a, b, Z, ref.R_OBS.astype(dtype)


@pytest.mark.parametrize("drawn", [True, False], ids=["drawn", "host_normals"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("np_,m", [(17, 9), (65, 33), (17, 33), (65, 9)])
def test_voted_consumers_equal_the_host_policy_sequence(gpu_required, np_, m, dtype, drawn):
    """A: data_associate -> sample_proposal_assoc[_drawn](use) -> resample_local_drawn -> add_features(ZN).
    B: associate_vote -> sample_proposal_voted[_drawn] -> resample_local_drawn -> add_features_voted.  Every record, the
    weights and n_features bit for bit."""
    from conan_slam_amd import pf

    nf, step = 40, 3
    a, b, Z, R = _pair(np_, nf, m, dtype, 900 + np_ + m)
    try:
        normals = np.random.default_rng(2).normal(size=(3, np_)).astype(dtype)
        use, ZN = pf.data_associate(a, Z, R, *GATES, 0.5)
        assert 0 < ZN.shape[1] < m, (np_, m, ZN.shape)
        if drawn:
            a.sample_proposal_assoc_drawn(Z, R, step, use, MISS)
        else:
            a.sample_proposal_assoc(Z, R, normals, use, MISS)
        a.resample_local_drawn(step, np_ + 1, True)
        a.add_features(ZN, R)

        b.associate_vote(Z, R, *GATES, 0.5)
        if drawn:
            b.sample_proposal_voted_drawn(Z, R, step, MISS)
        else:
            b.sample_proposal_voted(Z, R, normals, MISS)
        b.resample_local_drawn(step, np_ + 1, True, want_result=False)
        q = b.add_features_voted(R)
        assert q == ZN.shape[1] and a.n_features == b.n_features == nf + q
        ra, rb = _records(a), _records(b)
        assert ra.shape == (np_, 13 + 6 * (nf + q)) and _bits(ra, rb), (np_, m, np.dtype(dtype).name, drawn)
        assert _bits(a.get_weights(), b.get_weights())
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("np_,m", [(17, 9), (65, 33)])
def test_feature_update_voted_equals_feature_update_assoc(gpu_required, np_, m, dtype):
    from conan_slam_amd import pf

    a, b, Z, R = _pair(np_, 40, m, dtype, 700 + np_ + m)
    try:
        use, _ = pf.data_associate(a, Z, R, *GATES, 0.5)
        a.feature_update_assoc(Z, R, use)
        b.associate_vote(Z, R, *GATES, 0.5)
        b.feature_update_voted(Z, R)
        assert _bits(_records(a), _records(b)), (np_, m, np.dtype(dtype).name)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 3. the whole drive
def test_the_drive_in_one_call_per_scan(gpu_required):
    """The committed unknown-correspondence drive (f64, np = 17): assoc_scan_step_drawn on one handle, the host-policy
    sequence of test_pf_drive_gpu.py::test_unknown_correspondences on another.  After every scan records, nf and q are
    bitwise equal and the vote's use is the reference's."""
    from conan_slam_amd import pf
    from conan_slam_amd.pf import ParticleShard

    dtype = np.float64
    d, npart = D.make_drive(D.ASSOC_KEY), D.ASSOC_NP
    nmin = D.n_min(npart)
    want = {r.scan.step: r for r in D.assoc_reference()}
    a, b = (ParticleShard(npart, d.max_features, dtype=dtype) for _ in range(2))
    try:
        for sh in (a, b):
            sh.seed_draws(D.ASSOC_SEED)
        scans = 0
        for k in range(len(d.controls)):
            r = want.get(k)
            a.predict(*d.controls[k], d.Q, D.WB, D.DT)
            if r is None:
                assert b.assoc_scan_step_drawn(*d.controls[k], d.Q, D.WB, D.DT, np.zeros((2, 0)), d.R, D.GATE1, D.GATE2, k,
                                               nmin, True, D.NEW_FRACTION, D.MISS) == 0
                continue
            Z = r.scan.Z
            use, ZN = pf.data_associate(a, Z, d.R, D.GATE1, D.GATE2, D.NEW_FRACTION)
            a.sample_proposal_assoc_drawn(Z, d.R, k, use, D.MISS)
            a.resample_local_drawn(k, nmin, True)
            if ZN.shape[1]:
                a.add_features(ZN, d.R)
            q = b.assoc_scan_step_drawn(*d.controls[k], d.Q, D.WB, D.DT, Z, d.R, D.GATE1, D.GATE2, k, nmin, True,
                                        D.NEW_FRACTION, D.MISS)
            assert q == ZN.shape[1] and a.n_features == b.n_features == r.nf, (k, q, ZN.shape, r.nf)
            qw, use_b = b.vote_wait()
            assert qw == q and np.array_equal(use_b, r.use) and np.array_equal(use, r.use), (k, use_b, r.use)
            assert _bits(_records(a), _records(b)), (k, "records")
            scans += 1
        assert scans == len(want) and b.n_features == d.max_features
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 4. sharded
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_vote(gpu_required, world):
    """np = 72 split evenly over a loopback world: every rank's vote is identical and is new_feature_votes of the shards'
    own summaries added in rank order in float64 (the order of comm_loop_sum_kernel); on inputs whose vote margin in the
    f64 reference is at least 1e-6 its decisions are the unsharded handle's, and add_features_voted leaves the
    concatenated shards bitwise equal to the single handle."""
    from conan_slam_amd.pf import LoopbackComm
    from test_pf_gpu import _run_ranks

    dtype, npart, nf, m, f, step = np.float64, 72, 33, 40, 0.5, 5
    L = npart // world
    parts, Z = _cloud(npart, nf, dtype, 4242, m)
    R = ref.R_OBS.astype(dtype)
    # (the association sees the particles after the predict: so does the reference)
    case = ref.Case("sharded", dtype, ref.predicted_parts(parts, dtype), Z, R=R, gates=(GATES,))
    s = case.summary(GATES)
    share = s[:, 1] / s[:, :3].sum(axis=1)
    margin = float(np.abs(share - f).min())
    print(f"[sharded vote] world {world}: smallest vote margin of the f64 reference {margin:.3e}")
    assert margin >= 1e-6, margin

    single = _upload(parts, npart, nf, dtype, nfcap=nf + m)
    shards, comms = [], []
    try:
        single.seed_draws(9)
        single.predict(PREDICT[0], PREDICT[1], Q_CTRL, PREDICT[2], PREDICT[3])
        whole = _check_vote(single, Z, R, f, "single")
        assert 0 < whole.q < m
        single.sample_proposal_voted_drawn(Z, R, step, MISS)
        assert single.add_features_voted(R) == whole.q
        shards = [_upload(parts[r * L:(r + 1) * L], L, nf, dtype, nfcap=nf + m, n_global=npart) for r in range(world)]
        comms = LoopbackComm.create(world)

        def rank(r):
            sh = shards[r]
            sh.seed_draws(9, r * L, npart)
            sh.predict(PREDICT[0], PREDICT[1], Q_CTRL, PREDICT[2], PREDICT[3])
            sh.associate_vote(Z, R, *GATES, f, comm=comms[r])
            got = _device_vote(sh, m)
            own = sh.association()[2]
            sh.sample_proposal_voted_drawn(Z, R, step, MISS)
            q = sh.add_features_voted(R)
            return got, own, q, _records(sh), sh.n_features

        res = _run_ranks([(lambda r=r: rank(r)) for r in range(world)])
        acc = np.zeros((m, 4))
        for r in range(world):
            acc = acc + res[r][1]  # rank order, float64
        want = V.host_policy(acc, Z, f)
        for r in range(world):
            assert V.same(res[r][0], want), (world, r, "the rank-order sum")
            assert V.same(res[r][0], res[0][0]), (world, r, "identical on every rank")
            assert res[r][2] == want.q and res[r][4] == nf + want.q
        assert V.same(res[0][0], whole), (world, "the unsharded handle's decisions")
        assert _bits(np.concatenate([res[r][3] for r in range(world)]), _records(single)), (world, "records")
    finally:
        for c in comms:
            c.close()
        for sh in shards:
            sh.close()
        single.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def _code(fn):
    from conan_slam_amd import CslamError

    with pytest.raises(CslamError) as ei:
        fn()
    assert str(ei.value).strip() != ""
    return ei.value.code, str(ei.value)


def _state(sh, with_vote, m):
    out = [_records(sh).tobytes(), sh.n_features]
    out += [x.tobytes() for x in sh.association()]
    if with_vote:
        v = _device_vote(sh, m)
        out += [v.use.tobytes(), v.new_idx.tobytes(), v.ZN.tobytes(order="F"), v.q]
    return out


def test_refusals_change_nothing(gpu_required):
    from conan_slam_amd import _capi
    from conan_slam_amd.pf import ParticleShard

    dtype, np_, nf, m = np.float32, 17, 20, 9
    BAD, CAP = _capi.ERR_BAD_ARG, _capi.ERR_CAPACITY
    parts, Z = _cloud(np_, nf, dtype, 31, m)
    R = ref.R_OBS.astype(dtype)
    normals = np.zeros((3, np_), dtype)
    sh = _upload(parts, np_, nf, dtype, nfcap=nf + 1)
    try:
        sh.seed_draws(1)
        sh.predict(PREDICT[0], PREDICT[1], Q_CTRL, PREDICT[2], PREDICT[3])
        consumers = (lambda: sh.sample_proposal_voted(Z, R, normals, MISS), lambda: sh.sample_proposal_voted_drawn(Z, R, 0, MISS),
                     lambda: sh.feature_update_voted(Z, R))
        # before any vote, and after a plain associate
        for prepare in (lambda: None, lambda: sh.associate(Z, R, *GATES)):
            prepare()
            before = _records(sh).tobytes()
            for fn in consumers + (lambda: sh.add_features_voted(R), sh.vote_wait, sh.vote):
                assert _code(fn)[0] == BAD
            assert _records(sh).tobytes() == before and sh.n_features == nf
        # a non-finite new_fraction changes nothing: the tables and the (absent) vote stay
        tables = [x.tobytes() for x in sh.association()]
        for f in (np.nan, np.inf, -np.inf):
            assert _code(lambda: sh.associate_vote(Z, R, *GATES, f))[0] == BAD
        assert [x.tobytes() for x in sh.association()] == tables and _code(sh.vote_wait)[0] == BAD
        # a live vote: another Z, another m
        sh.associate_vote(Z, R, *GATES, 0.5)
        q = sh.vote_wait()[0]
        assert q > 1, q  # more than the one free feature slot
        before = _state(sh, True, m)
        other = Z.copy()
        other[0, 0] += 1.0
        for fn in (lambda: sh.sample_proposal_voted(other, R, normals, MISS), lambda: sh.feature_update_voted(other, R),
                   lambda: sh.sample_proposal_voted_drawn(Z[:, :-1], R, 0, MISS),
                   lambda: sh.sample_proposal_voted(Z, R, normals, np.nan)):
            assert _code(fn)[0] == BAD
        # capacity overflow: refused, and the vote is still there
        assert _code(lambda: sh.add_features_voted(R))[0] == CAP
        assert _code(lambda: sh.add_features_voted(R))[0] == CAP
        assert _state(sh, True, m) == before
        # ... still addable on a smaller q: the same scan voted on with a fraction nobody reaches, then a shorter scan
        sh.associate_vote(Z, R, *GATES, 1.5)
        assert sh.add_features_voted(R) == 0 and sh.n_features == nf
        code, text = _code(lambda: sh.add_features_voted(R))  # a second add
        assert code == BAD and "already" in text
        use_full = V.host_policy(sh.association()[2], Z, 0.5).use
        keep = sorted([int(np.nonzero(use_full == 1)[0][0])] + [int(j) for j in np.nonzero(use_full == 0)[0][:1]])
        Zs = np.asfortranarray(Z[:, keep])
        sh.associate_vote(Zs, R, *GATES, 0.5)
        qs = sh.vote_wait()[0]
        assert qs == 1, qs
        # consumers after a resample say "moved"; the add is still allowed
        sh.resample_local_drawn(0, np_ + 1, True, want_result=False)
        before = _records(sh).tobytes()
        for fn in (lambda: sh.sample_proposal_voted(Zs, R, normals, MISS), lambda: sh.sample_proposal_voted_drawn(Zs, R, 0, MISS),
                   lambda: sh.feature_update_voted(Zs, R)):
            code, text = _code(fn)
            assert code == BAD and "moved" in text, text
        assert _records(sh).tobytes() == before
        assert sh.add_features_voted(R) == qs and sh.n_features == nf + qs
        assert _code(lambda: sh.add_features_voted(R))[0] == BAD
        assert sh.n_features == nf + qs
    finally:
        sh.close()
    # assoc_scan_step_drawn on an unseeded handle
    sh = ParticleShard(np_, 8, dtype=dtype)
    try:
        before = _records(sh).tobytes()
        assert _code(lambda: sh.assoc_scan_step_drawn(1.0, 0.0, Q_CTRL, 2.8, 0.1, Z, R, *GATES, 0, np_, True))[0] == BAD
        assert _records(sh).tobytes() == before and sh.n_features == 0 and _code(sh.vote_wait)[0] == BAD
        # ... and on a capacity overflow the scan has run and no feature was added (an empty map: all nine are new)
        sh.seed_draws(1)
        assert _code(lambda: sh.assoc_scan_step_drawn(1.0, 0.0, Q_CTRL, 2.8, 0.1, Z, R, *GATES, 0, np_, True))[0] == CAP
        assert sh.n_features == 0 and sh.vote_wait()[0] == m and _records(sh).tobytes() != before
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------ 6. no round trip
@pytest.mark.parametrize("m", [8, 32])
def test_no_round_trip(gpu_required, m):
    """assoc_scan_step_drawn with m <= 32 adds at most the association's one staged copy; associate_vote +
    sample_proposal_voted_drawn + resample_local_drawn(want_result=False) queue behind one another with no synchronise in
    between -- held by the state after a later synchronise, not by timing."""
    from conan_slam_amd import pf

    dtype, np_, nf, step = np.float32, 65, 40, 2
    a, b, Z, R = _pair(np_, nf, m, dtype, 300 + m)
    c = None
    try:
        use, ZN = pf.data_associate(a, Z, R, *GATES, 0.5)
        a.sample_proposal_assoc_drawn(Z, R, step, use, MISS)
        a.resample_local_drawn(step, np_ + 1, True)
        a.add_features(ZN, R)
        n0 = b.stage_copies()
        b.associate_vote(Z, R, *GATES, 0.5)
        b.sample_proposal_voted_drawn(Z, R, step, MISS)
        b.resample_local_drawn(step, np_ + 1, True, want_result=False)
        assert b.stage_copies() - n0 <= 1
        assert b.add_features_voted(R) == ZN.shape[1]
        b.synchronize()
        assert _bits(_records(a), _records(b))
        # the one-call form: a twin of the pair before its predict, the same control in the call
        parts, _ = _cloud(np_, nf, dtype, 300 + m, m)
        c = _upload(parts, np_, nf, dtype, nfcap=nf + m)
        c.seed_draws(11)
        c.synchronize()
        n0 = c.stage_copies()
        q = c.assoc_scan_step_drawn(PREDICT[0], PREDICT[1], Q_CTRL, PREDICT[2], PREDICT[3], Z, R, *GATES, step, np_ + 1, True,
                                    0.5, MISS)
        assert c.stage_copies() - n0 <= 1 and q == ZN.shape[1]
        assert _bits(_records(a), _records(c))
    finally:
        for sh in (a, b, c):
            if sh is not None:
                sh.close()
