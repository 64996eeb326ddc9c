"""Particle weights at the ENDS of the floating-point range on the device (conan_slam_amd/csrc/pf_kernels.hpp,
cslam_pf.hip, conan_slam_amd/pf.py): subnormal weights and sums, sums whose reciprocal overflows the particle dtype, sums
beyond its largest finite number, total underflow, a NaN or +inf weight -- through every resample route -- then the
proposal kernels under exact scaling and in gradual underflow, and the readers under scaling.  The inputs and every
property claimed of them are built and proved in pf_weight_range_ref.py / test_pf_weight_range_cpu.py."""
import numpy as np
import pytest

import pf_assoc_ref as aref
import pf_weight_range_ref as wr
from pf_builders import random_particles, shard_from, tagged_records
from score_ref import POSE_BAD
from test_pf_assoc_gpu import upload
from test_pf_edges_gpu import _assert_kept, _bulk_read, _bulk_shard, _same_bits
from test_pf_gpu import _run_ranks

pytestmark = pytest.mark.gpu

NEFF_TOL = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-12}  # of test_pf_edges_cpu.test_exact_resample_inputs
ROUTES = ("local", "fused", "host")
STILL = (0.0, 0.03, 73.0, 0.01)   # v, swa, wheel base, dt of the fused route's predict: a vehicle at rest keeps xv[0]
Q_CTRL = np.diag([0.18, 6e-4])
R_OBS = np.diag([0.08, 0.0024])


def _ids(k):
    return "-".join(map(str, k))


def _run(route, rec, dtype, sel, n_eff, status, report=False):
    """One resample of the records `rec` through a route -> (neff or None, resampled or None, records before the
    resample decision, records after, the shard).  The fused route predicts first (a vehicle at rest): its `before` is a
    twin shard's records after the same predict."""
    from conan_slam_amd.pf import SingleComm, resample_particles

    n = rec.shape[0]
    sh = _bulk_shard(rec, dtype)
    sh.set_degenerate_policy(report)
    before = rec
    if route == "local":
        neff, did = sh.resample_local(sel, n_eff, status)
    elif route == "host":
        sh.host_resample = True
        neff, did = resample_particles(sh, SingleComm(), n_eff, status, select=sel)
    elif route == "drawn":
        sh.seed_draws(7)
        neff, did = sh.resample_local_drawn(0, n_eff, status)
    else:
        twin = _bulk_shard(rec, dtype)
        twin.predict(STILL[0], STILL[1], Q_CTRL.astype(dtype), STILL[2], STILL[3])
        before = _bulk_read(twin)
        twin.close()
        assert _same_bits(before[:, :2], rec[:, :2]), "the predict of a vehicle at rest moved a weight or xv[0]"
        sh.observation_step(STILL[0], STILL[1], Q_CTRL.astype(dtype), STILL[2], STILL[3], np.zeros((2, 0), dtype),
                            np.zeros(0, np.int32), R_OBS.astype(dtype), np.zeros((3, n), dtype), sel, n_eff, status)
        _, did, neff = sh.resample_stats()
        did = bool(did)
    return neff, did, before, _bulk_read(sh), sh


def _check_normalised(tag, case, neff, did, before, got, want_w):
    assert not did, tag
    assert _same_bits(got[:, 0].copy(), want_w), (tag, "weights", got[:8, 0], want_w[:8])
    assert abs(neff - case.neff) <= NEFF_TOL[case.dtype] * case.neff, (tag, neff, case.neff)
    assert _same_bits(got[:, 1:], before[:, 1:]), (tag, "a normalisation alone changed a pose, covariance or feature")


# ------------------------------------------------------------------------------------------------ 1. normalisation and plan
@pytest.mark.parametrize("key", wr.scaled_case_keys(), ids=_ids)
def test_scaled_exact_cases_through_every_single_handle_route(gpu_required, key):
    """pf_resample_plan_kernel (resample_local; the fused observation_step with m = 0), and the host-planned path
    (weight_sums, scale_weights / divide_weights, stratified_keep, gather_local), on ExactResampleCase times 2^e with
    n = 10 and n = 257 (a second trip of the 256-lane strides): sums with subnormal weights, with the last finite
    reciprocal of T, with the first that overflows it, with unit weights at the smallest subnormal, with the scale at and
    under the smallest normal, and (f32, n = 257) beyond T's largest finite number.  Without resampling the weights are
    k / G bit for bit, Neff the case's, nothing else changes; with n_effective = n + 1 slot c is particle keep[c] bit for
    bit and the weights are 1 / n."""
    case = wr.scaled_case(key)
    dt, n = case.dtype.type, case.n
    rec = tagged_records(n, case.raw_weights(), dt)
    sel = case.select()
    for route in ROUTES:
        tag = f"{case} {route}"
        neff, did, before, got, sh = _run(route, rec, dt, sel, n + 1, False)
        _check_normalised(tag, case, neff, did, before, got, case.norm_weights())
        sh.close()
        neff, did, before, got, sh = _run(route, rec, dt, sel, n + 1, True)
        assert did and abs(neff - case.neff) <= NEFF_TOL[case.dtype] * case.neff, (tag, neff, did)
        _assert_kept(got, before, case.keep, n, dt, tag)
        sh.close()


@pytest.mark.parametrize("key", [k for k in wr.scaled_case_keys(ns=(257,))], ids=_ids)
def test_scaled_exact_cases_with_device_drawn_strata(gpu_required, key):
    """resample_local_drawn once per sum, normalisation only (its strata are not ours to set): k / G bit for bit."""
    case = wr.scaled_case(key)
    rec = tagged_records(case.n, case.raw_weights(), case.dtype.type)
    neff, did, before, got, sh = _run("drawn", rec, case.dtype.type, None, case.n + 1, False)
    _check_normalised(f"{case} drawn", case, neff, did, before, got, case.norm_weights())
    sh.close()


def _run_sharded(rec, dtype, world, sel, n_eff, status, report=False):
    from conan_slam_amd.pf import LoopbackComm

    N = rec.shape[0]
    L = N // world
    shards = [_bulk_shard(rec[r * L:(r + 1) * L], dtype) for r in range(world)]
    for sh in shards:
        sh.set_degenerate_policy(report)
    comms = LoopbackComm.create(world)
    res = _run_ranks([(lambda r=r: shards[r].resample_sharded(comms[r], sel, n_eff, status)) for r in range(world)])
    got = np.concatenate([_bulk_read(sh) for sh in shards])
    for c in comms:
        c.close()
    return res, got, shards


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("key", wr.scaled_case_keys(ns=(16,)), ids=_ids)
def test_scaled_exact_cases_sharded(gpu_required, key, world):
    """cslam_pf_resample_sharded (both normalising launches: the rank's own weights, and the gathered weights that
    pf_keep_kernel plans from) over loopback worlds of 2 and 4 at N = 16, same cases, same demands; every rank reports
    the same Neff and decision.  (N = 16 has no `beyond_max` case: with G = 2^7 its largest weight is not finite in f32.)"""
    case = wr.scaled_case(key)
    dt, N = case.dtype.type, case.n
    rec = tagged_records(N, case.raw_weights(), dt)
    res, got, shards = _run_sharded(rec, dt, world, case.select(), N + 1, False)
    for r in range(world):
        _check_normalised(f"{case} world={world} rank {r}", case, res[r][0], res[r][1], rec, got, case.norm_weights())
    for sh in shards:
        sh.close()
    res, got, shards = _run_sharded(rec, dt, world, case.select(), N + 1, True)
    for r in range(world):
        assert res[r][1] and abs(res[r][0] - case.neff) <= NEFF_TOL[case.dtype] * case.neff, (case, r, res[r])
    _assert_kept(got, rec, case.keep, N, dt, f"{case} world={world}")
    for sh in shards:
        sh.close()


@pytest.mark.parametrize("key", wr.NONPOW2_KEYS, ids=_ids)
def test_sums_that_are_no_power_of_two(gpu_required, key):
    """resample_local and the host-planned path on integer weights whose sum K is no power of two, in the subnormal range
    of T and near its top: within 2 ulp of k / K computed exactly and rounded to T (one rounding of the scale or quotient,
    one of the product, half an ulp each, rounded up), the two routes bit for bit alike."""
    case = wr.nonpow2_case(key)
    dt = case.dtype.type
    rec = tagged_records(case.n, case.raw_weights(), dt)
    sel = np.linspace(0.0, 1.0, case.n, endpoint=False).astype(dt)
    want, seen = case.expected(), []
    for route in ("local", "host"):
        neff, did, before, got, sh = _run(route, rec, dt, sel, case.n + 1, False)
        worst = float(wr.ulps(got[:, 0], want).max())
        print(f"[ulp] {case} {route}: largest error {worst:.3g} ulp")
        assert not did and worst <= 2.0, (case, route, worst)
        assert abs(neff - case.neff) <= NEFF_TOL[case.dtype] * case.neff, (case, route, neff, case.neff)
        assert _same_bits(got[:, 1:], before[:, 1:])
        seen.append(got[:, 0].copy())
        sh.close()
    assert _same_bits(seen[0], seen[1]), (case, "the device plan and the host-planned path differ")


# ------------------------------------------------------------------------------------------------ 2. degenerate sums
def _assert_degenerate(tag, sh, neff, did, before, got, want_w, stats):
    assert did is False or did == 0, (tag, did)
    assert np.isnan(neff), (tag, neff)
    assert np.array_equal(got[:, 0], want_w, equal_nan=True), (tag, got[:, 0], want_w)
    assert _same_bits(got[:, 1:], before[:, 1:]), (tag, "a pose, covariance or feature changed")
    if stats:
        calls, resamples, last = sh.resample_stats()
        assert (calls, resamples) == (1, 0) and np.isnan(last), (tag, calls, resamples, last)
    est = sh.estimate()
    assert np.isnan(est.Xv).all() and np.isnan(est.Pv).all() and np.isnan(est.XF).all() and np.isnan(est.PF).all(), (tag, est)
    sh.score_reset("mean")
    sh.score(np.zeros(3), with_map=False)
    assert sh.scores().totals[POSE_BAD] == 1, tag


@pytest.mark.parametrize("key", wr.degenerate_keys(), ids=_ids)
def test_degenerate_sums_are_reported_not_resampled(gpu_required, key):
    """All weights zero (total underflow), one NaN, one +inf, and (f64) finite weights whose double sum is +inf, through
    every route -- resample_local, the fused step, the host-planned path, the drawn form, loopback worlds of 2 and 4 -- on
    handles with cslam_pf_set_degenerate_policy(CSLAM_PF_REPORT), n_effective = n + 1 and resampling on.  The sum is not
    a positive finite number: nothing is resampled, Neff is NaN, the weights are the IEEE w / sum w, every pose, covariance
    and feature keeps its bits, resample_stats counts a call and no resample, the host-planned path returns (nan, False)
    and does not raise; the estimate is NaN afterwards and one score call counts POSE_BAD (include/cslam.h).  The policy a
    handle starts with, CSLAM_PF_REPAIR, is the defect this rule replaces (every slot resampled onto particle 0, weights
    1 / n) and is asserted nowhere; DESIGN.md section 8 says what still runs on it."""
    kind, dtn = key
    dt = np.dtype(dtn).type
    case, w = wr.degenerate_weights(kind, dt)
    n, sel, want = case.n, case.select(dt), wr.ieee_quotients(w, dt)
    rec = tagged_records(n, np.ones(n), dt)
    rec[:, 0] = w
    for route in ROUTES + ("drawn",):
        neff, did, before, got, sh = _run(route, rec, dt, sel, n + 1, True, report=True)
        _assert_degenerate(f"{kind} {dtn} {route}", sh, neff, did, before, got, want, stats=route != "host")
        sh.close()
    for world in (2, 4):
        res, got, shards = _run_sharded(rec, dt, world, sel, n + 1, True, report=True)
        L = n // world
        for r, sh in enumerate(shards):
            _assert_degenerate(f"{kind} {dtn} world={world} rank {r}", sh, res[r][0], res[r][1], rec[r * L:(r + 1) * L],
                               got[r * L:(r + 1) * L], want[r * L:(r + 1) * L], stats=False)
            sh.close()


def test_degenerate_policy_leaves_healthy_sums_alone(gpu_required):
    """The same healthy resample under both policies, every single-handle route: the same bits (the policy is read only
    where the sum is not positive and finite); a policy that is neither is refused."""
    from conan_slam_amd import CslamError, _capi

    case = wr.scaled_case(("control", 257, "float32"))
    rec = tagged_records(case.n, case.raw_weights(), np.float32)
    for route in ROUTES:
        outs = []
        for report in (False, True):
            neff, did, _, got, sh = _run(route, rec, np.float32, case.select(), case.n + 1, True, report=report)
            outs.append((neff, did, got))
            sh.close()
        assert outs[0][:2] == outs[1][:2] and outs[0][1] and _same_bits(outs[0][2], outs[1][2]), route
    sh = _bulk_shard(rec, np.float32)
    with pytest.raises(CslamError) as ei:
        _capi.check(sh._L.cslam_pf_set_degenerate_policy(sh._h, 2))
    assert ei.value.code == _capi.ERR_BAD_ARG
    sh.close()


# ------------------------------------------------------------------------------------------------ 3. proposal weights
def _propose(kernel, case, parts):
    """The proposal of `case` on the particles `parts` -> (weights, every particle's other fields, the table or None)."""
    dt = np.dtype(case.dtype).type
    if kernel == "proposal":
        sh = shard_from(parts, case.nf, dt)
        sh.sample_proposal(case.Z, case.idf, case.R, case.normals)
        idf = None
    else:
        sh = upload(aref.Case("weight-range", dt, parts, case.Z, R=case.R.astype(np.float64)))
        sh.associate(case.Z, case.R, *case.gates)
        idf = sh.association()[0]
        sh.sample_proposal_assoc(case.Z, case.R, case.normals, case.use, wr.MISS)
    w = sh.get_weights()
    fields = [sh.get_particle(i)[1:] for i in range(len(parts))]
    sh.close()
    return w, fields, idf


@pytest.mark.parametrize("dtype", wr.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", wr.PROPOSAL_SHAPES, ids=lambda s: f"m{s[0]}-np{s[1]}")
@pytest.mark.parametrize("kernel", wr.KERNELS)
def test_proposal_weights_scale_exactly_inside_the_normal_range(gpu_required, kernel, shape, dtype):
    """pf_sample_proposal_kernel and pf_sample_proposal_assoc_kernel with every input weight times 2^e, e = -E_NORMAL- and
    +E_NORMAL+ (two binades inside the exponents up to which the same-dtype oracle scales exactly): the weights are
    2^e x those of the unscaled call on a twin shard bit for bit; poses and maps, which do not depend on w, are equal bit
    for bit.  The sibling's product holds the miss factor (a used observation somebody has no match for)."""
    case = wr.proposal_case(kernel, shape, dtype)
    w0, f0, idf0 = _propose(kernel, case, case.parts)
    assert np.all(np.isfinite(w0)) and np.all(w0 > 0)
    if kernel == "assoc":
        assert ((idf0 == 0) & (case.use[:, None] == 1)).any() and (idf0 != 0).any(), case
    lo, hi = wr.E_NORMAL[(kernel, shape[0], np.dtype(dtype).name)]
    for e in (-lo, hi):
        we, fe, idfe = _propose(kernel, case, wr.scaled_parts(case.parts, e, dtype))
        want = wr.scale2(w0, e, dtype)
        assert np.all(np.isfinite(want)) and np.all(want > 0)
        bad = np.nonzero(we != want)[0]
        assert bad.size == 0, (kernel, shape, e, f"{bad.size} weights differ; first: particle {bad[0]}", we[bad[0]], want[bad[0]])
        assert idf0 is None or np.array_equal(idf0, idfe)
        for i, (a, b) in enumerate(zip(f0, fe)):
            assert all(_same_bits(x, y) for x, y in zip(a, b)), (kernel, shape, e, "pose or map of particle", i)


@pytest.mark.parametrize("shape", wr.PROPOSAL_SHAPES, ids=lambda s: f"m{s[0]}-np{s[1]}")
@pytest.mark.parametrize("kernel", wr.KERNELS)
def test_proposal_weights_in_gradual_underflow(gpu_required, kernel, shape):
    """f32, the exponents wr.E_SUB: most weights leave the call on the subnormal grid.  The rule of assert_weights_fair
    over every particle, none left out, in the measure |g - wh| / max(wh, 2^-126) (wh: the f64 oracle on the same
    inputs; one step of the subnormal grid is one ulp in it): device maximum and median within 4x the f32 oracle's
     + 1e-6 / 1e-7; a particle whose f64 weight is below 2^-150 comes back as 0 or at most two grid steps.
    Measured on the MI355X (device max / median against f32-oracle max / median; weights the device left subnormal / zero):
      proposal m=1 e=-122   1.469e-05 / 7.625e-07   against 1.457e-05 / 9.732e-07    61 / 0
      proposal m=9 e=-135   7.018e-05 / 5.265e-06   against 6.522e-05 / 5.682e-06    57 / 0
      assoc    m=1 e=-122   9.105e-06 / 1.056e-07   against 9.105e-06 / 1.335e-08    62 / 0
      assoc    m=1 e=-135   7.187e-07 / 3.004e-08   against 7.187e-07 / 3.004e-08    33 / 32
      assoc    m=9 e=-90    5.025e-05 / 5.911e-06   against 5.049e-05 / 5.353e-06    17 / 4
    The device keeps f32 subnormals and follows the oracle into gradual underflow; no kernel had to change."""
    case = wr.proposal_case(kernel, shape, np.float32)
    for e in wr.E_SUB[(kernel, shape[0])]:
        parts = wr.scaled_parts(case.parts, e, np.float32)
        g, _, idf = _propose(kernel, case, parts)
        wh = wr.oracle_weights(kernel, case, np.float64, e, idf)
        wc = wr.oracle_weights(kernel, case, np.float32, e, idf)
        gmax, gmed, cmax, cmed = wr.sub_errors(g, wc, wh)
        print(f"[subnormal weights] {kernel} m={shape[0]} e={e}: device max {gmax:.3e} median {gmed:.3e}; cpu max {cmax:.3e} "
              f"median {cmed:.3e}; (subnormal, normal, below 2^-150) by the f64 oracle {wr.sub_census(wh)}, "
              f"device weights subnormal {int(((g > 0) & (g < 2.0 ** -126)).sum())} zero {int((g == 0).sum())}")
        assert np.all(np.isfinite(g)) and np.all(g >= 0), (kernel, shape, e)
        assert gmax <= 4.0 * cmax + 1e-6, (kernel, shape, e, gmax, cmax)
        assert gmed <= 4.0 * cmed + 1e-7, (kernel, shape, e, gmed, cmed)
        # (kernel == "proposal": `under` is empty -- no exponent hands the plain kernel such a weight, see wr.E_SUB and
        # test_pf_weight_range_cpu.py::test_subnormal_exponents; the condition is exercised by the sibling alone)
        under = wh < 2.0 ** -150
        assert under.any() == (kernel == "assoc" and e == min(wr.E_SUB[(kernel, shape[0])])), (kernel, shape, e)
        assert np.all(g[under] <= 2.0 * 2.0 ** -149), (kernel, shape, e, g[under].max())


# ------------------------------------------------------------------------------------------------ 4. readers under scaling
def _small_weights(n, dtype, seed):
    """Weights k / 256 with k in [1, 255]: eight bits, so that 2^e times them is exact down to a unit of 2^-149."""
    return (np.random.default_rng(seed).integers(1, 256, size=n) / 256.0).astype(dtype)


READER_E = {np.dtype(np.float32): (-135,), np.dtype(np.float64): (-900, 900)}
_READS = {}


def _read_scaled(dtype, e):
    """(estimate, (best max, best min), (use, new_idx, q)) with every weight times 2^e; built once per (dtype, e)."""
    key = (np.dtype(dtype).name, e)
    if key not in _READS:
        npart, nf = 65, 3
        parts = random_particles(npart, nf, dtype, seed=301)
        w0 = _small_weights(npart, dtype, 302)
        we = wr.scale2(w0, e, dtype)
        assert np.array_equal(we.astype(np.float64), np.ldexp(w0.astype(np.float64), e)), "the scaling is not exact"
        if e and dtype == np.float32:
            assert 0 < float(we.astype(np.float64).sum()) < 2.0 ** -126
        sh = shard_from(parts, nf, dtype)
        sh.set_weights(we)
        est, best = sh.estimate(), (sh.best_particle("max").index, sh.best_particle("min").index)
        sh.close()
        vote_case = aref.get_case(("U", 130, 20, 6, 3, np.dtype(dtype).name))
        vs = upload(vote_case, nfcap=vote_case.nf + 3)
        vs.set_weights(wr.scale2(_small_weights(vote_case.np_, dtype, 303), e, dtype))
        vs.associate_vote(vote_case.Z, vote_case.R, *vote_case.gates[0])
        use, idx, _, q = vs.vote()
        vs.close()
        _READS[key] = (est, best, (use.copy(), idx.copy(), q))
    return _READS[key]


@pytest.mark.parametrize("dtype", wr.DTYPES, ids=lambda d: np.dtype(d).name)
def test_readers_under_scaling(gpu_required, dtype):
    """estimate, best_particle and associate_vote on weights times 2^e against the unscaled twin.  f32: e = -135, sum w
    about 2^-130 (subnormal), unit 2^-143; f64: e = -900 and +900.  The readers accumulate in double, where the scaling is
    exact: W scales exactly, every moment keeps its bits, the best particle keeps its index, the vote its use[], new_idx
    and q; f32: Neff keeps its bits too (f64: test_estimate_neff_under_scaling_f64, and sharded below)."""
    est0, best0, vote0 = _read_scaled(dtype, 0)
    assert vote0[2] == 3 and np.isfinite(est0.neff)
    for e in READER_E[np.dtype(dtype)]:
        est, best, vote = _read_scaled(dtype, e)
        assert est.w_sum == float(np.ldexp(est0.w_sum, e)), (e, est.w_sum, est0.w_sum)
        if dtype == np.float32:
            assert est.neff == est0.neff, (e, est.neff, est0.neff)
        for name in ("Xv", "Pv", "XF", "PF"):
            assert _same_bits(getattr(est, name), getattr(est0, name)), (e, name, getattr(est, name), getattr(est0, name))
        assert best == best0, (e, best, best0)
        assert np.array_equal(vote[0], vote0[0]) and np.array_equal(vote[1], vote0[1]) and vote[2] == vote0[2], (e, vote, vote0)


def test_estimate_neff_under_scaling_f64(gpu_required):
    """The Neff that estimate() returns, f64, weights times 2^-900 and 2^+900, against the unscaled twin: bit-equal, as
    every other figure of the readers is.  The squares of such weights leave the range of double (the plain W * W / W2 was
    0 / 0 = NaN below and inf / inf = NaN above, measured on the MI355X against 50.512626546473456 unscaled), so an f64
    set carries the sums of the squares of 2^512 w and 2^-512 w through partials and rank summaries
    (pf_estimate_kernels.hpp, est_neff); a power of two scales every term exactly, hence the same bits."""
    est0 = _read_scaled(np.float64, 0)[0]
    for e in READER_E[np.dtype(np.float64)]:
        est = _read_scaled(np.float64, e)[0]
        print(f"[estimate Neff] e = {e}: {est.neff!r} against {est0.neff!r} unscaled")
        assert est.neff == est0.neff, (e, est.neff, est0.neff)


def test_sharded_estimate_neff_under_scaling_f64(gpu_required):
    """estimate_sharded over a loopback world of 2 (the scaled sums of squares travel in the rank summaries and
    pf_est_combine_kernel adds them): f64 weights times 2^-900 and 2^+900 give the Neff of the unscaled set bit for bit on
    every rank, and that is the single handle's (the weights are k / 256: every sum is exact in either order)."""
    from conan_slam_amd.pf import LoopbackComm

    world, L, nf = 2, 65, 3
    parts = random_particles(world * L, nf, np.float64, seed=311)
    w0 = _small_weights(world * L, np.float64, 312)
    whole = shard_from(parts, nf, np.float64)
    whole.set_weights(w0)
    want = whole.estimate().neff
    whole.close()
    assert np.isfinite(want)
    for e in (0,) + READER_E[np.dtype(np.float64)]:
        shards = [shard_from(parts[r * L:(r + 1) * L], nf, np.float64) for r in range(world)]
        for r, sh in enumerate(shards):
            sh.set_weights(wr.scale2(w0[r * L:(r + 1) * L], e, np.float64))
        comms = LoopbackComm.create(world)
        ests = _run_ranks([(lambda r=r: shards[r].estimate_sharded(comms[r])) for r in range(world)])
        for r in range(world):
            assert ests[r].neff == want, (e, r, ests[r].neff, want)
            assert ests[r].w_sum == ests[0].w_sum and np.all(np.isfinite(ests[r].Xv)), (e, r)
        for c in comms:
            c.close()
        for sh in shards:
            sh.close()
