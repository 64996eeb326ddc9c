"""The batched scan generator (cslam_sim_batch_*, BatchSimulator) and the two batch calls that consume its scans
(EKFBatch.update_scan / augment_scan): integers and noise-free values against the oracle and the single-scan Simulator,
the device-side noise against the numpy restatement of slam.h:168-178 with synth.normal, the edges, the slot ring under
unsynchronised consumption, the demo study driven from the device generator, and misuse."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_close
from pyoracle import Oracle, TEXTBOOK

pytestmark = pytest.mark.gpu

F = np.float32
N_MAP, STEPS, RMAX, SWA = 2000, 120, 50.0, 0.4176
R = np.diag([0.08, 0.0024]).astype(F)
RE = (8 * R).astype(F)
SEEDS = [77, 78, 5, 77]


def _map():
    return np.asfortranarray(np.random.default_rng(11).uniform(-400, 400, (2, N_MAP)).astype(F))


def _truth():
    """f64 truth from (0, 0, 0.3), steps 1..120; returns the f32 poses."""
    x, y, phi, out = 0.0, 0.0, 0.3, []
    for _ in range(STEPS):
        x += 9.0 * np.cos(SWA + phi)
        y += 9.0 * np.sin(SWA + phi)
        phi = (phi + 9.0 * np.sin(SWA) / 73.0 + np.pi) % (2 * np.pi) - np.pi
        out.append(np.array([x, y, phi], dtype=F))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _raises(code, fn, *args):
    from conan_slam_amd import CslamError

    with pytest.raises(CslamError) as ei:
        fn(*args)
    assert ei.value.code == code, (ei.value.code, code)


# ------------------------------------------------------------------------------------------------------ 1. noise-free


def test_integers_exact_and_noise_free_values_bit_equal(gpu_required):
    from conan_slam_amd import BatchSimulator, Simulator

    LM = _map()
    o = Oracle(F)
    bs = BatchSimulator(LM, 4, SEEDS)
    one = Simulator(LM)
    table = np.zeros(N_MAP, dtype=np.int32)
    nf, both, sizes = 0, 0, []
    for step, xv in enumerate(_truth(), start=1):
        m, mf, mn = bs.scan(xv, RMAX, None, step)
        Zo, tags_o = o.get_observations(xv, LM, RMAX)
        ZFo, ZNo, idfo = o.data_associate_table(Zo, tags_o, table, nf)
        assert (m, mf, mn) == (len(tags_o), ZFo.shape[1], ZNo.shape[1]), step
        Z1, tags1 = one.get_observations(xv, RMAX)
        ZF1, ZN1, idf1 = one.data_associate_table(nf)
        for i in range(4):
            ZF, idf, ZN, tags = bs.get_scan(i)
            assert np.array_equal(tags, tags_o) and np.array_equal(idf, idfo), (step, i)
            assert _same(ZF, ZF1) and _same(ZN, ZN1), (step, i)
        assert np.array_equal(bs.table, table), step
        nf += mn
        both += (mf > 0 and mn > 0)
        sizes.append((m, mf, mn))
    # the scenario stays inside the 32-observation cap without leaving a step out
    assert min(s[0] for s in sizes) >= 1 and max(s[0] for s in sizes) <= 32
    assert nf == 336 and both > 50
    bs.close()
    one.close()


# ----------------------------------------------------------------------------------------------------------- 2. noise


def _restate(Z0, seed, step):
    """slam.h:168-178 in f32 on the whole scan Z0 (2 x m), g = synth.normal(seed + 1, (10_000_000 + step) * 64 + 2c + r)."""
    from conan_slam_amd.synth import normal

    m = Z0.shape[1]
    base = (10_000_000 + step) * 64
    c = np.arange(m, dtype=np.uint64)
    out, term = np.empty_like(Z0), np.empty_like(Z0)
    for r in range(2):
        g = normal(seed + 1, np.uint64(base + r) + np.uint64(2) * c).astype(F)
        term[r] = (g * F(np.sqrt(R[r, r]))).astype(F)
        out[r] = (Z0[r] + term[r]).astype(F)
    return out, term


def test_device_noise_matches_the_numpy_restatement(gpu_required):
    from conan_slam_amd import BatchSimulator

    LM = _map()
    gen = BatchSimulator(LM, 4, SEEDS)
    twin = BatchSimulator(LM, 4, SEEDS)
    solo = BatchSimulator(LM, 1, SEEDS[:1])
    clean = BatchSimulator(LM, 1, [0])
    total = differ = 0
    draws = []
    for step, xv in enumerate(_truth(), start=1):
        before = gen.table
        sizes = gen.scan(xv, RMAX, R, step)
        assert twin.scan(xv, RMAX, R, step) == sizes and solo.scan(xv, RMAX, R, step) == sizes
        assert clean.scan(xv, RMAX, None, step) == sizes
        ZF0, idf0, ZN0, tags = clean.get_scan(0)
        known = before[tags - 1] != 0
        Z0 = np.empty((2, sizes[0]), dtype=F)
        Z0[:, known], Z0[:, ~known] = ZF0, ZN0
        got = []
        for i in range(4):
            ZF, idf, ZN, tg = gen.get_scan(i)
            assert np.array_equal(idf, idf0) and np.array_equal(tg, tags)
            want, term = _restate(Z0, SEEDS[i], step)
            Z = np.empty_like(Z0)
            Z[:, known], Z[:, ~known] = ZF, ZN
            ulp = np.spacing(np.maximum(np.abs(Z), np.abs(term)).astype(F)).astype(np.float64)
            err = np.abs(Z.astype(np.float64) - want.astype(np.float64))
            assert np.all(err <= 3 * ulp), (step, i, float((err / ulp).max()))
            total += Z.size
            differ += int(np.count_nonzero(_bits(Z) != _bits(want)))
            got.append((ZF, ZN))
            if i < 3:
                draws.append((Z[0].astype(np.float64) - Z0[0].astype(np.float64)) / float(np.sqrt(R[0, 0])))
            ZFt, _, ZNt, _ = twin.get_scan(i)
            assert _same(ZF, ZFt) and _same(ZN, ZNt), (step, i)  # the same (seed, step): the same scan
        assert _same(got[0][0], got[3][0]) and _same(got[0][1], got[3][1]), step  # equal seeds
        assert not (_same(got[0][0], got[1][0]) and _same(got[0][1], got[1][1])), step
        ZFs, _, ZNs, _ = solo.get_scan(0)
        assert _same(ZFs, got[0][0]) and _same(ZNs, got[0][1]), step  # instance 0 does not depend on I
    print(f"noise: {differ} of {total} entries not bitwise equal to the restatement")
    assert differ <= 0.01 * total, (differ, total)
    d = np.concatenate(draws)
    K = d.size
    print(f"range draws: K = {K}, mean {d.mean():.4f}, variance {d.var():.4f}")
    assert abs(d.mean()) <= 5.0 / np.sqrt(K) and abs(d.var() - 1.0) <= 5.0 * np.sqrt(2.0 / K), (K, d.mean(), d.var())
    for s in (gen, twin, solo, clean):
        s.close()


# ----------------------------------------------------------------------------------------------------------- 3. edges


def test_edges(gpu_required):
    from conan_slam_amd import BatchSimulator, EKFBatch, _capi

    LM = _map()
    poses = _truth()
    gen = BatchSimulator(LM, 4, SEEDS)
    twin = BatchSimulator(LM, 4, SEEDS)
    for step in range(1, 11):
        assert gen.scan(poses[step - 1], RMAX, R, step) == twin.scan(poses[step - 1], RMAX, R, step)
    table, held = gen.table, [gen.get_scan(i) for i in range(4)]
    sizes = (gen.m, gen.mf, gen.mn)
    _raises(_capi.ERR_CAPACITY, gen.scan, poses[10], 400.0, R, 11)  # more than 32 visible landmarks
    gen.m, gen.mf, gen.mn = sizes
    assert np.array_equal(gen.table, table)
    for i in range(4):
        for a, b in zip(held[i], gen.get_scan(i)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for step in range(11, 14):  # continues as if the call had not been made (the table, nf and the noise)
        assert gen.scan(poses[step - 1], RMAX, R, step) == twin.scan(poses[step - 1], RMAX, R, step)
        for i in range(4):
            for a, b in zip(gen.get_scan(i), twin.get_scan(i)):
                assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(gen.table, twin.table)
    # a pose that sees nothing: both consumers are no-ops
    assert gen.scan(poses[13], 1e-3, R, 14) == (0, 0, 0)
    b = EKFBatch(4, 0, quirks=TEXTBOOK, max_landmarks=8)
    X0 = [b.get_state(i) for i in range(4)]
    b.update_scan(gen, RE)
    b.augment_scan(gen, RE)
    assert b.n == 3
    for i in range(4):
        X, P = b.get_state(i)
        assert np.array_equal(X, X0[i][0]) and np.array_equal(P, X0[i][1])
    b.close()
    gen.close()
    twin.close()
    # an empty map and a single instance
    e = BatchSimulator(np.zeros((2, 0), dtype=F), 1, [5])
    assert e.scan([0.0, 0.0, 0.0], RMAX, R, 1) == (0, 0, 0)
    assert e.table.size == 0
    e.close()
    # bad arguments
    _raises(_capi.ERR_BAD_ARG, BatchSimulator, LM, 256, list(range(256)))
    L = _capi.lib()
    h = C.c_void_p()
    seeds = (C.c_longlong * 2)(1, 2)
    assert L.cslam_sim_batch_create(None, 10, 2, seeds, -1, C.byref(h)) == _capi.ERR_BAD_ARG and not h.value
    assert L.cslam_sim_batch_create(LM.ctypes.data_as(C.c_void_p), N_MAP, 2, None, -1, C.byref(h)) == _capi.ERR_BAD_ARG
    assert not h.value


# ----------------------------------------------------------------------------------------------------- 4. consumption


def _run_scan_batch(LM, poses, QE, sync, keep=None):
    """Batch A of item 4: scan + update_scan + augment_scan.  keep: list that receives every instance's downloaded scan."""
    from conan_slam_amd import BatchSimulator, EKFBatch

    gen = BatchSimulator(LM, 4, SEEDS)
    a = EKFBatch(4, 0, quirks=TEXTBOOK, max_landmarks=384)
    for step, xv in enumerate(poses, start=1):
        a.predict(900.0, SWA, QE, 73.0, 0.01)
        a.observe_heading(float(xv[2]))
        gen.scan(xv, RMAX, R, step)
        a.update_scan(gen, RE)
        if sync:
            a.synchronize()
        a.augment_scan(gen, RE)
        if sync:
            a.synchronize()
        if keep is not None:
            keep.append([gen.get_scan(i) for i in range(4)])
    states = [a.get_state(i) for i in range(4)]
    n, flags = a.n, a.factor_status()
    a.close()
    gen.close()
    return states, n, flags


def test_consumption_is_the_old_path_bit_for_bit(gpu_required):
    import torch

    from conan_slam_amd import EKFBatch
    from conan_slam_amd.synth import noise_matrices
    from sim_driver import OracleBackend

    LM, poses = _map(), _truth()
    QE = noise_matrices(F)[2]
    scans = []
    sa, na, fa = _run_scan_batch(LM, poses, QE, sync=False, keep=scans)
    # batch B: every scan downloaded, uploaded into the caller's own device tensors, update_device / augment_device
    b = EKFBatch(4, 0, quirks=TEXTBOOK, max_landmarks=384)
    hold = []
    for xv, sc in zip(poses, scans):
        b.predict(900.0, SWA, QE, 73.0, 0.01)
        b.observe_heading(float(xv[2]))
        mf, mn = sc[0][0].shape[1], sc[0][2].shape[1]
        if mf:
            dz = [torch.from_numpy(np.ascontiguousarray(s[0].reshape(-1, order="F"))).cuda() for s in sc]
            di = [torch.from_numpy(np.ascontiguousarray(s[1])).cuda() for s in sc]
            hold += dz + di
            b.update_device([t.data_ptr() for t in dz], [t.data_ptr() for t in di], mf, RE)
        if mn:
            dn = [torch.from_numpy(np.ascontiguousarray(s[2].reshape(-1, order="F"))).cuda() for s in sc]
            hold += dn
            b.augment_device([t.data_ptr() for t in dn], mn, RE)
    sb = [b.get_state(i) for i in range(4)]
    assert na == b.n == 675 and fa == [0] * 4 and b.factor_status() == [0] * 4
    b.close()
    for i in range(4):
        assert np.array_equal(sa[i][0], sb[i][0]) and np.array_equal(sa[i][1], sb[i][1]), i
    # the slot ring: the same run with a synchronise after every call
    ss, ns, fs = _run_scan_batch(LM, poses, QE, sync=True)
    assert ns == 675 and fs == [0] * 4
    for i in range(4):
        assert np.array_equal(sa[i][0], ss[i][0]) and np.array_equal(sa[i][1], ss[i][1]), i
    # instances 0 (seed 77) and 2 (seed 5) against their oracles, fed the downloaded scans
    for i in (0, 2):
        lo, hi = OracleBackend(F, TEXTBOOK, max_landmarks=384), OracleBackend(np.float64, TEXTBOOK, max_landmarks=384)
        for xv, sc in zip(poses, scans):
            ZF, idf, ZN, _ = sc[i]
            for o, dt in ((lo, F), (hi, np.float64)):
                o.predict(900.0, SWA, QE.astype(dt), 73.0, 0.01)
                o.observe_heading(float(xv[2]), True)
                if ZF.shape[1]:
                    assert o.update(np.asfortranarray(ZF.astype(dt)), RE.astype(dt), idf, True) == 0
                if ZN.shape[1]:
                    o.augment(np.asfortranarray(ZN.astype(dt)), RE.astype(dt))
        assert lo.n == 675
        assert_close(f"X[{i}]", sa[i][0], lo.get_x(), 1e-4, hi.get_x(), fair=8.0)


# ------------------------------------------------------------------------------------------------- 5. the demo study


def _demo_truth(LM, WP, steps):
    """run_demo's truth side through the same harness helpers: per control step the true pose (f32), the steering angle
    and whether the step observes."""
    from sim_driver import SlamConfig

    cfg = SlamConfig()
    sim = Oracle(F)
    XTrue = np.zeros(3, dtype=F)
    WPd = WP.astype(F, order="F")
    dt = cfg.dt_controls
    iwp, swa, loops, dtsum, out = 1, F(0.0), float(cfg.number_loops), 0.0, []
    while 0 < iwp <= WP.shape[1] and len(out) < steps:
        iwp, swa = sim.compute_swa(XTrue, WPd, iwp, cfg.at_waypoint, swa, cfg.rate_swa, cfg.max_swa, F(dt), True)
        if iwp == 0 and loops > 1:
            iwp, loops = 1, loops - 1
        sim.vehicle_model(XTrue, cfg.velocity, swa, cfg.wheel_base, F(dt))
        dtsum += dt
        observe = dtsum >= cfg.dt_observe
        if observe:
            dtsum = 0.0
        out.append((XTrue.copy(), F(swa), observe))
    return cfg, out


def test_demo_study_from_the_device_generator(gpu_required):
    from conan_slam_amd import BatchSimulator, EKFBatch
    from conan_slam_amd.synth import control_noise, noise_matrices
    from sim_driver import OracleBackend, load_demo_map, run_demo
    from test_batch_mc_demo_gpu import _Rec, _check_against_oracles

    STEPS_DEMO, seeds = 2400, [1000 + i for i in range(8)]
    I = len(seeds)
    LM, WP = load_demo_map()
    cfg, truth = _demo_truth(LM, WP, STEPS_DEMO)
    Qm, Rm, QE, REm = noise_matrices(F)
    gen = BatchSimulator(LM, I, seeds)
    b = EKFBatch(I, 0, quirks=TEXTBOOK, max_landmarks=64)
    lo = [OracleBackend(F, TEXTBOOK) for _ in seeds]
    hi = [OracleBackend(np.float64, TEXTBOOK) for _ in seeds]
    wb, dt = float(cfg.wheel_base), float(F(cfg.dt_controls))
    updates, scans = 0, []
    for step, (xv, swa, observe) in enumerate(truth, start=1):
        vn, swan = control_noise(seeds, step, cfg.velocity, swa, Qm)
        b.predict_each(vn, swan, QE, wb, dt)
        b.observe_heading(float(xv[2]))
        for i in range(I):
            for o, t in ((lo[i], F), (hi[i], np.float64)):
                o.predict(t(vn[i]), t(swan[i]), QE.astype(t), t(wb), t(dt))
                o.observe_heading(t(xv[2]), True)
        if not observe:
            continue
        m, mf, mn = gen.scan(xv, float(cfg.max_range), Rm, step)
        b.update_scan(gen, REm)
        b.augment_scan(gen, REm)
        updates += mf > 0
        got = [gen.get_scan(i) for i in range(I)]
        if m:
            scans.append(got)
        for i in range(I):
            ZF, idf, ZN, _ = got[i]
            for o, t in ((lo[i], F), (hi[i], np.float64)):
                if mf:
                    o.update(np.asfortranarray(ZF.astype(t)), REm.astype(t), idf, True)
                if mn:
                    o.augment(np.asfortranarray(ZN.astype(t)), REm.astype(t))
    refs = [{"final_n": o.n, "updates": updates, "X": o.get_x(), "trace_P": float(np.trace(o.get_p().astype(np.float64)))}
            for o in lo]
    his = [{"X": o.get_x(), "trace_P": float(np.trace(o.get_p().astype(np.float64)))} for o in hi]
    assert updates > 300
    _check_against_oracles(b, updates, refs, his)
    b.close()
    gen.close()
    # the device scans beside the harness's recorded scans of run_demo(noise_seed): idf and shapes exact, values within the
    # f32 bound of the noise-free scan (2e-6 relative) plus the 3 ulps of the noise arithmetic
    for i, s in enumerate(seeds):
        r = _Rec(OracleBackend(F, TEXTBOOK))
        run_demo(r, LM, WP, noise_seed=s, max_steps=STEPS_DEMO)
        k = 0
        calls = [c for c in r.calls if c[0] in "UA"]
        for sc in scans:
            ZF, idf, ZN, _ = sc[i]
            for Zd, kind in ((ZF, "U"), (ZN, "A")):
                if Zd.shape[1] == 0:
                    continue
                c = calls[k]
                k += 1
                assert c[0] == kind and c[1].shape == Zd.shape, (i, k)
                if kind == "U":
                    assert np.array_equal(c[2], idf), (i, k)
                ref = c[1].astype(np.float64)
                tol = 2e-6 * np.maximum(1.0, np.abs(ref)) + 3 * np.spacing(np.abs(c[1]).astype(F)).astype(np.float64)
                assert np.all(np.abs(Zd.astype(np.float64) - ref) <= tol), (i, k)
        assert k == len(calls), (i, k, len(calls))


# ---------------------------------------------------------------------------------------------------------- 6. misuse


def test_misuse_changes_nothing(gpu_required):
    from conan_slam_amd import BatchSimulator, EKFBatch, _capi
    from conan_slam_amd.synth import noise_matrices

    LM, poses = _map(), _truth()
    QE = noise_matrices(F)[2]
    gen, gen2 = BatchSimulator(LM, 4, SEEDS), BatchSimulator(LM, 4, SEEDS)
    a = EKFBatch(4, 0, quirks=TEXTBOOK, max_landmarks=384)
    twin = EKFBatch(4, 0, quirks=TEXTBOOK, max_landmarks=384)
    other = EKFBatch(3, 0, quirks=TEXTBOOK, max_landmarks=384)
    fresh = EKFBatch(4, 0, quirks=TEXTBOOK, max_landmarks=384)
    sized = EKFBatch(4, 5, quirks=TEXTBOOK, max_landmarks=384)
    bad = _capi.ERR_BAD_ARG
    seen_both = 0
    for step, xv in enumerate(poses[:12], start=1):
        for e in (a, twin):
            e.predict(900.0, SWA, QE, 73.0, 0.01)
            e.observe_heading(float(xv[2]))
            e.predict(900.0, SWA, QE, 73.0, 0.01)  # (held: it rides inside the update's window)
        m, mf, mn = gen.scan(xv, RMAX, R, step)
        assert gen2.scan(xv, RMAX, R, step) == (m, mf, mn)
        _raises(bad, other.update_scan, gen, RE)  # instance counts differ
        _raises(bad, other.augment_scan, gen, RE)
        if step == 1:
            assert mf == 0 and mn > 0
            _raises(bad, sized.augment_scan, gen, RE)  # 5 features, the scan was split against 0
        if mf > 0:
            _raises(bad, fresh.update_scan, gen, RE)  # no features, the scan was split against nf > 0
            _raises(bad, a.augment_scan, gen, RE)  # augment before a non-empty update
        a.update_scan(gen, RE)
        _raises(bad, a.update_scan, gen, RE)  # consumed twice
        a.augment_scan(gen, RE)
        _raises(bad, a.augment_scan, gen, RE)
        _raises(bad, a.update_scan, gen, RE)
        twin.update_scan(gen2, RE)
        twin.augment_scan(gen2, RE)
        seen_both += (mf > 0 and mn > 0)
        assert a.n == twin.n
    assert seen_both >= 5
    for i in range(4):
        Xa, Pa = a.get_state(i)
        Xt, Pt = twin.get_state(i)
        assert np.array_equal(Xa, Xt) and np.array_equal(Pa, Pt), i
    assert a.factor_status() == twin.factor_status() == [0] * 4
    assert fresh.n == 3 and sized.n == 13 and other.n == 3
    with pytest.raises(Exception):
        EKFBatch(4, 0, quirks=TEXTBOOK, max_landmarks=8).update_scan(BatchSimulator(LM, 4, SEEDS), RE)  # no scan yet
    for h in (a, twin, other, fresh, sized, gen, gen2):
        h.close()
