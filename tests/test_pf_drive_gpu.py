"""The particle filter AS A FILTER on the device: the closed-loop drive of tests/pf_drive_ref.py (90 control steps from an
empty map, 18 scans of every dispatcher branch, 10 resamples on a map that grows between them) through
ParticleShard.scan_step_drawn, against the CPU oracle's per-particle calls in the same closed loop, after EVERY scan.

What only a closed loop reaches is the host-side state of cslam_pf.hip: launch_resample sizes the gather by the nf of
that moment and swaps the store with its twin, which holds stale columns beyond the nf it was last written with; nf then
grows and the next resample must carry the new columns; the branch that does not resample must leave normalised weights
for the next proposal's product; each dispatcher branch must consume the draws of its own step.
test_pf_drive_cpu.py proves on the oracle alone that every resample decision of the drive is decisive (so keep[] is not a
matter of rounding) and that each of nine such slips would fail the check applied here."""
import numpy as np
import pytest

import pf_drive_ref as D
from pf_builders import DTYPES, TOL, assert_weights_fair
from pf_estimate_ref import all_features_ref, best_ref, cov_errors, estimate_ref, mean_errors, stack, _judge
from pf_score_ref import PfScoreRef
from test_pf_edges_gpu import _bulk_read, _same_bits
from test_pf_gpu import _run_ranks

pytestmark = pytest.mark.gpu

NP = {np.dtype(np.float32): D.NP32, np.dtype(np.float64): D.NP64}
SEED = {np.dtype(np.float32): D.SEED32, np.dtype(np.float64): D.SEED64}
NONE_Z, NONE_IDF = np.zeros((2, 0)), np.zeros(0, np.int32)


def _refs(dtype):
    """(same-dtype oracle drive, f64 oracle drive on the same inputs): one and the same for f64."""
    if np.dtype(dtype) == np.float64:
        return D.reference("f64"), D.reference("f64")
    return D.reference("f32"), D.reference("f32hi")


def _shard(dtype, n_local=None, first=0, seeded=True):
    from conan_slam_amd.pf import ParticleShard

    n = NP[np.dtype(dtype)]
    sh = ParticleShard(n_local or n, D.committed_drive().max_features, dtype=dtype, n_global=n)
    if seeded:
        sh.seed_draws(SEED[np.dtype(dtype)], first, n)
    assert sh.n_features == 0
    return sh


def _scan_inputs(scan):
    if scan is None:
        return NONE_Z, NONE_IDF, NONE_Z
    return scan.ZF, scan.idf, scan.ZN


def _step_fused(sh, d, k, nmin):
    ZF, idf, ZN = _scan_inputs(d.by_step.get(k))
    sh.scan_step_drawn(*d.controls[k], d.Q, D.WB, D.DT, ZF, idf, ZN, d.R, k, nmin, True)


def _step_separate(sh, d, k, nmin):
    """The same step as separate _drawn calls -> (neff, resampled) or None."""
    scan = d.by_step.get(k)
    sh.predict(*d.controls[k], d.Q, D.WB, D.DT)
    if scan is None or scan.kind == D.EMPTY:
        return None
    if scan.kind == D.NEW:
        sh.sample_pose_drawn(k)
        sh.add_features(scan.ZN, d.R)
        return None
    sh.sample_proposal_drawn(scan.ZF, scan.idf, d.R, k)
    sh.feature_update(scan.ZF, scan.idf, d.R)
    res = sh.resample_local_drawn(k, nmin, True)
    if scan.kind == D.MIXED:
        sh.add_features(scan.ZN, d.R)
    return res


def _step_host_arrays(sh, d, k, nmin, normals, select):
    """The same step through the host-array forms, fed the draws of step k."""
    scan = d.by_step.get(k)
    if scan is None or scan.kind == D.EMPTY:
        sh.predict(*d.controls[k], d.Q, D.WB, D.DT)
    elif scan.kind == D.NEW:
        sh.new_feature_step(*d.controls[k], d.Q, D.WB, D.DT, scan.ZN, d.R, normals)
    else:
        sh.observation_step(*d.controls[k], d.Q, D.WB, D.DT, scan.ZF, scan.idf, d.R, normals, select, nmin, True)
        if scan.kind == D.MIXED:
            sh.add_features(scan.ZN, d.R)


_FUSED = {}


def _fused_records(dtype):
    """The records after every scan of the single-handle drive through scan_step_drawn (run once per dtype)."""
    key = np.dtype(dtype)
    if key not in _FUSED:
        d, nmin = D.committed_drive(), D.n_min(NP[key])
        sh = _shard(dtype)
        try:
            out = []
            for k in range(len(d.controls)):
                _step_fused(sh, d, k, nmin)
                if k in d.by_step:
                    out.append(_bulk_read(sh))
        finally:
            sh.close()
        _FUSED[key] = out
    return _FUSED[key]


# ------------------------------------------------------------------------------------------------ 1, 2. known correspondences
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_drive_against_the_oracle(gpu_required, dtype):
    """f64, np = 72: every field of every particle after every scan within max(1e-12, 4 amp eps64) of the f64 oracle
    drive, relative to max(1, |ref|max) of the field.  f32, np = 17: the fairness rule -- device error against the f64
    drive <= 4 x the CPU f32 drive's error against it + TOL[f32].  Both: weights exactly 1/np where the oracle resampled,
    the device's cumulative (calls, resamples) the oracle's decisions, last_neff within tolerance, n_features by the
    table, Pv bitwise zero after every scan that saw something, the store full at the end."""
    dt = np.dtype(dtype)
    f64 = dt == np.float64
    d, npart = D.committed_drive(), NP[dt]
    nmin = D.n_min(npart)
    lo, hi = _refs(dtype)
    bound64 = D.f64_bound(D.amplification(D.reference("f32"), D.reference("f32hi")))
    sh = _shard(dtype)
    try:
        j, calls, resamples, worst = 0, 0, 0, 0.0
        for k in range(len(d.controls)):
            _step_fused(sh, d, k, nmin)
            scan = d.by_step.get(k)
            if scan is None:
                continue
            rl, rh = lo[j], hi[j]
            j += 1
            tag = f"{dt.name} step {k} ({scan.kind})"
            assert sh.n_features == scan.nf_after == rh.nf, tag
            rec = _bulk_read(sh)
            assert rec.dtype == dt and rec.shape == (npart, 13 + 6 * rh.nf), tag
            e_dev, e_cpu = D.field_errors(rec, rh.rec, rh.nf), D.field_errors(rl.rec, rh.rec, rh.nf)
            print(f"[drive] {tag}: device " + " ".join(f"{n} {e_dev[n]:.2e}" for n in D.FIELDS)
                  + ("" if f64 else "; cpu " + " ".join(f"{n} {e_cpu[n]:.2e}" for n in D.FIELDS)))
            for name in D.FIELDS:
                bound = bound64 if f64 else D.fair_bound(e_cpu[name])
                worst = max(worst, e_dev[name] / bound)
                assert e_dev[name] <= bound, (tag, name, e_dev[name], bound)
            if scan.kind != D.EMPTY:
                assert rec[:, 4:13].tobytes() == np.zeros((npart, 9), dtype).tobytes(), (tag, "Pv")
            if rh.norm is not None:
                calls, resamples = calls + 1, resamples + int(rh.resampled)
                got_calls, got_res, neff = sh.resample_stats()
                assert (got_calls, got_res) == (calls, resamples), (tag, got_calls, got_res, calls, resamples)
                tol_neff = TOL[dt] * max(1.0, rh.neff) + (0.0 if f64 else 4.0 * abs(rl.neff - rh.neff))
                print(f"[drive] {tag}: Neff {neff:.9g} (oracle {rh.neff:.9g}, Nmin {nmin}), resampled {rh.resampled}")
                assert abs(neff - rh.neff) <= tol_neff, (tag, neff, rh.neff, tol_neff)
                if rh.resampled:
                    assert np.all(rec[:, 0] == dt.type(1.0) / dt.type(npart)), (tag, "weights after a resample")
                else:
                    assert_weights_fair(tag, rec[:, 0], rl.norm, rh.norm, dtype)
        assert j == len(hi) and sh.n_features == d.max_features
        print(f"[drive] {dt.name}: largest device error over the drive = {worst:.3f} of its bound")
    finally:
        sh.close()


# ------------------------------------------------------------------------------------------------ 3. the three forms
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_separate_and_host_array_forms_agree(gpu_required, dtype):
    """scan_step_drawn against predict + sample_proposal_drawn + feature_update + resample_local_drawn + add_features
    (all-new scans: predict + sample_pose_drawn + add_features) and against observation_step / new_feature_step fed
    draws(k): the whole store bit for bit after every scan, across ten swaps of the store and a map grown from 0 to 30."""
    dt = np.dtype(dtype)
    d, nmin = D.committed_drive(), D.n_min(NP[dt])
    _, hi = _refs(dtype)
    fused = _fused_records(dtype)
    b, c = _shard(dtype), _shard(dtype, seeded=False)
    try:
        j = 0
        for k in range(len(d.controls)):
            normals, select = b.draws(k)
            res = _step_separate(b, d, k, nmin)
            _step_host_arrays(c, d, k, nmin, normals, select)
            if k not in d.by_step:
                continue
            if res is not None:
                assert res[1] == hi[j].resampled, (k, res)
            rb, rc = _bulk_read(b), _bulk_read(c)
            assert b.n_features == c.n_features == d.by_step[k].nf_after, k
            assert _same_bits(fused[j], rb), (dt.name, k, "fused against the separate calls")
            assert _same_bits(fused[j], rc), (dt.name, k, "fused against the host-array forms")
            j += 1
        assert j == len(fused)
    finally:
        b.close()
        c.close()


# ------------------------------------------------------------------------------------------------ 4. sharded
_SHARDED = {}


def _sharded_run(world):
    """The f64 drive over a loopback world (run once per world): every rank seeds its global slots and runs the separate
    _drawn calls with resample_sharded_drawn (new_feature_step_drawn on the all-new scans).
    -> (per scan the concatenated records, per rank the (neff, resampled) of every resample call)."""
    from conan_slam_amd.pf import LoopbackComm

    if world in _SHARDED:
        return _SHARDED[world]
    dtype = np.float64
    d, npart = D.committed_drive(), D.NP64
    nmin, L = D.n_min(npart), npart // world
    assert L * world == npart
    shards, comms = [], []
    try:
        shards = [_shard(dtype, n_local=L, first=r * L) for r in range(world)]
        comms = LoopbackComm.create(world)

        def rank(r):
            sh, out, decisions = shards[r], [], []
            for k in range(len(d.controls)):
                scan = d.by_step.get(k)
                if scan is None or scan.kind == D.EMPTY:
                    sh.predict(*d.controls[k], d.Q, D.WB, D.DT)
                elif scan.kind == D.NEW:
                    sh.new_feature_step_drawn(*d.controls[k], d.Q, D.WB, D.DT, scan.ZN, d.R, k)
                else:
                    sh.predict(*d.controls[k], d.Q, D.WB, D.DT)
                    sh.sample_proposal_drawn(scan.ZF, scan.idf, d.R, k)
                    sh.feature_update(scan.ZF, scan.idf, d.R)
                    decisions.append(sh.resample_sharded_drawn(comms[r], k, nmin, True))
                    if scan.kind == D.MIXED:
                        sh.add_features(scan.ZN, d.R)
                if scan is not None:
                    out.append(_bulk_read(sh))
            assert sh.n_features == d.max_features
            return out, decisions

        res = _run_ranks([(lambda r=r: rank(r)) for r in range(world)])
    finally:
        for c in comms:
            c.close()
        for sh in shards:
            sh.close()
    recs = [np.concatenate([res[r][0][j] for r in range(world)]) for j in range(len(d.scans))]
    _SHARDED[world] = (recs, [res[r][1] for r in range(world)])
    return _SHARDED[world]


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))).max()) if a.size else 0.0


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_drive_equals_the_single_handle(gpu_required, world):
    """f64, np = 72 over loopback worlds of 2 and 4 (36 + 36, 4 x 18): after every scan the concatenated shards against
    the single-handle drive, bit for bit -- every rank's decision and Neff, the whole state (poses, Pv, the map) at EVERY
    scan, and the weights wherever they are reset.  The exchange plan, pack / unpack and the record length work on a map
    that grows between resamples.  (The weights a scan leaves when it does NOT resample are held by the test below: they depend on the order of a sum.)"""
    d, hi = D.committed_drive(), D.reference("f64")
    recs, decisions = _sharded_run(world)
    fused = _fused_records(np.float64)
    want = [(h.neff, h.resampled) for h in hi if h.norm is not None]
    for r in range(world):
        assert [x[1] for x in decisions[r]] == [x[1] for x in want], r
        assert all(abs(a[0] - b[0]) <= TOL[np.dtype(np.float64)] * max(1.0, b[0]) for a, b in zip(decisions[r], want)), r
    assert len(recs) == len(fused) == len(hi)
    for got, whole, h in zip(recs, fused, hi):
        tag = (world, h.scan.step, h.scan.kind)
        assert got.shape == whole.shape, tag
        assert _same_bits(got[:, 1:], whole[:, 1:]), (tag, "state", _ulps(got[:, 1:], whole[:, 1:]))
        if h.norm is None or h.resampled:
            assert _same_bits(got[:, 0], whole[:, 0]), (tag, "weights", _ulps(got[:, 0], whole[:, 0]))


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_weights_without_a_resample_equal_the_single_handle(gpu_required, world):
    """The rest of the comparison above: the normalised weights a scan leaves when it does not resample, bit for bit
    against the single handle.  Both paths scale by (T)(1 / sum w) with the sum formed in double, so the sums must be
    the same bits: every rank of cslam_pf_resample_sharded forms them from the gathered weights with the one-shard
    reduction.  (An all-reduce of per-rank sums adds the same terms in another order: it left the four scans of this
    drive that do not resample 2 - 3 ulp from the single handle, in 47 to 72 of the 72 weights.)"""
    hi = D.reference("f64")
    recs, _ = _sharded_run(world)
    fused = _fused_records(np.float64)
    off = []
    for got, whole, h in zip(recs, fused, hi):
        if not _same_bits(got[:, 0], whole[:, 0]):
            off.append((h.scan.step, h.scan.kind, int((got[:, 0] != whole[:, 0]).sum()), _ulps(got[:, 0], whole[:, 0])))
    print(f"[sharded] world {world}: weights differ at (step, kind, particles, largest difference in ulps) {off}")
    assert not off, off


# ------------------------------------------------------------------------------------------------ 5. the readers
def _assert_moments(tag, got, ref, dtype, scale, npart):
    """pf_estimate_ref.assert_moments with one addition for the sets a resample leaves: where every particle is a copy of
    ONE (Neff = 1 before the resample) the true pose covariance is zero and the helper's bound, 1e-9 of the reference's
    largest entry, is 1e-9 of a rounding residue.  A mean off by d turns a centred second moment into var + d^2, and the
    f64 sum of np terms of magnitude `scale` is off by at most np eps64 scale: the covariances get that square as a floor
    (3e-25 here, against pose variances of 1e-2 wherever the particles differ)."""
    assert abs(got.w_sum - ref.w_sum) <= 1e-12 * abs(ref.w_sum), (tag, got.w_sum, ref.w_sum)
    assert abs(got.neff - ref.neff) <= 1e-12 * abs(ref.neff), (tag, got.neff, ref.neff)
    floor = (npart * D.EPS64 * scale) ** 2
    _judge(tag, "Xv", *mean_errors(got.Xv, ref.Xv, dtype, heading=2))
    _judge(tag, "XF", *mean_errors(got.XF, ref.XF, dtype))
    for name in ("Pv", "PF"):
        err, bound = cov_errors(getattr(got, name), getattr(ref, name), dtype)
        _judge(tag, name, err, bound + floor)


def _assert_readers(tag, sh, rec, nf, dtype, oracle_rec=None):
    """estimate / best_particle / all_features of a store that has been swapped some number of times, against the float64
    helpers applied to the set the store holds (and, where given, to the oracle's set), at those helpers' tolerances."""
    scale, npart = float(np.abs(rec[:, 1:].astype(np.float64)).max()), rec.shape[0]
    assert_moments = lambda t, got, ref, dt: _assert_moments(t, got, ref, dt, scale, npart)
    arrs = stack(D.parts_of(rec, nf))
    est = sh.estimate()
    assert est.XF.shape == (2, nf) and est.PF.shape == (4, nf), tag
    assert_moments(tag, est, estimate_ref(*arrs), dtype)
    if oracle_rec is not None:
        assert_moments(tag + " (oracle's set)", est, estimate_ref(*stack(D.parts_of(oracle_rec, nf))), dtype)
        assert best_ref(oracle_rec[:, 0], "max") == best_ref(rec[:, 0], "max"), tag
    best = sh.best_particle("max")
    i = best_ref(arrs[0], "max")
    assert best.index == i, (tag, best.index, i)
    got = np.concatenate([[best.w], best.Xv, best.Pv.reshape(-1, order="F"), best.XF.reshape(-1, order="F"),
                          best.PF.reshape(-1, order="F")]).astype(dtype)
    assert _same_bits(got, rec[i]), (tag, "best particle's record")
    allf = sh.all_features()
    assert _same_bits(allf, np.asfortranarray(all_features_ref(arrs[3]).astype(dtype))), (tag, "all_features")


@pytest.mark.parametrize("dtype", DTYPES)
def test_readers_along_the_drive(gpu_required, dtype):
    """After EVERY scan that saw something (so after an odd and an even number of swaps, the last resampling scan and the
    end of the drive among them): estimate(), best_particle("max") and all_features() against pf_estimate_ref on the set
    the store holds -- in f64 also on the oracle's set -- and score() of both estimators against pf_score_ref with the
    drive's true pose and its landmarks in tag order, the track bit for bit."""
    dt = np.dtype(dtype)
    d, nmin = D.committed_drive(), D.n_min(NP[dt])
    _, hi = _refs(dtype)
    live = [s for s in d.scans if s.kind != D.EMPTY]
    shards = {"mean": _shard(dtype), "best": _shard(dtype)}
    try:
        refs = {}
        for est, sh in shards.items():
            sh.score_reset(est, series_capacity=len(live))
            refs[est] = PfScoreRef(dtype, est, series_capacity=len(live))
        j, swaps, parities = 0, 0, set()
        for k in range(len(d.controls)):
            for sh in shards.values():
                _step_fused(sh, d, k, nmin)
            scan = d.by_step.get(k)
            if scan is None:
                continue
            h = hi[j]
            j += 1
            if scan.kind == D.EMPTY:
                continue
            swaps += int(h.resampled)
            parities.add(swaps % 2)
            tag = f"readers {dt.name} step {k} ({scan.kind}, {swaps} swaps)"
            sh = shards["mean"]
            rec = _bulk_read(sh)
            _assert_readers(tag, sh, rec, h.nf, dtype, h.rec if dt == np.float64 else None)
            truth = d.truth[:h.nf]
            for est, s in shards.items():
                s.score_set_truth(truth)
                refs[est].add(s.estimate() if est == "mean" else s.best_particle("max"), truth, np.array(d.poses[k]))
                s.score(d.poses[k])
        assert parities == {0, 1} and shards["mean"].n_features == d.max_features
        for est, s in shards.items():
            got = s.scores()
            assert got.calls == len(live)
            refs[est].check(got, f"score {dt.name} {est}")
    finally:
        for s in shards.values():
            s.close()


# ------------------------------------------------------------------------------------------------ 6. unknown correspondences
def test_unknown_correspondences(gpu_required):
    """f64, np = 17, the drive of ASSOC_KEY without its table: per scan predict, pf.data_associate(4, 25),
    sample_proposal_assoc_drawn, resample_local_drawn, add_features of the voted columns.  association() equals the
    reference's tables in every scan (test_pf_drive_cpu.py holds every decision decisive), the vote the reference's, and
    the records agree with the closed-loop reference at the bound of the known-correspondence drive."""
    from conan_slam_amd import pf
    from conan_slam_amd.pf import ParticleShard

    dtype = np.float64
    d, npart = D.make_drive(D.ASSOC_KEY), D.ASSOC_NP
    nmin = D.n_min(npart)
    ref = {r.scan.step: r for r in D.assoc_reference()}
    bound = D.f64_bound(D.amplification(D.reference("f32"), D.reference("f32hi")))
    sh = ParticleShard(npart, d.max_features, dtype=dtype)
    try:
        sh.seed_draws(D.ASSOC_SEED)
        worst = 0.0
        for k in range(len(d.controls)):
            sh.predict(*d.controls[k], d.Q, D.WB, D.DT)
            r = ref.get(k)
            if r is None:
                continue
            Z = r.scan.Z
            use, ZN = pf.data_associate(sh, Z, d.R, D.GATE1, D.GATE2, D.NEW_FRACTION)
            idf, kind, _ = sh.association()
            assert np.array_equal(idf, r.idf) and np.array_equal(kind, r.kind), (k, "association")
            assert np.array_equal(use, r.use), (k, use, r.use)
            sh.sample_proposal_assoc_drawn(Z, d.R, k, use, D.MISS)
            neff, did = sh.resample_local_drawn(k, nmin, True)
            if ZN.shape[1]:
                sh.add_features(ZN, d.R)
            assert did == r.resampled and abs(neff - r.neff) <= TOL[np.dtype(dtype)] * max(1.0, r.neff), (k, neff, did, r.neff)
            assert sh.n_features == r.nf, k
            rec = _bulk_read(sh)
            err = D.field_errors(rec, r.rec, r.nf)
            print(f"[assoc drive] step {k}: " + " ".join(f"{n} {err[n]:.2e}" for n in D.FIELDS))
            worst = max(worst, max(err.values()))
            assert max(err.values()) <= bound, (k, err, bound)
            if did:
                assert np.all(rec[:, 0] == 1.0 / npart), k
        assert sh.n_features == d.max_features
        print(f"[assoc drive] largest error {worst:.3e} (bound {bound:.1e})")
    finally:
        sh.close()
