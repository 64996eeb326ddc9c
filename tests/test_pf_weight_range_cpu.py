"""The inputs of test_pf_weight_range_gpu.py, proved on the CPU oracle alone (no GPU): particle weights at the ENDS of the
floating-point range.  The scaled exact cases are exact in their dtype; the oracle reproduces them wherever its own sum
stays finite (and demonstrably fails beyond, which is why the exact rational is the reference there); the normalisation
the device used before -- w * (T)(1 / ws) -- fails the new cases (the negative control); the degenerate sets give NaN and
no resample on the oracle; and the exponents of the scaled proposal cases are found and checked here."""
from fractions import Fraction

import numpy as np
import pytest

import pf_weight_range_ref as wr
from conan_slam_amd.pf import SingleComm, resample_particles, stratified_keep
from pyoracle import Oracle

NEFF_TOL = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-12}  # of test_pf_edges_cpu.test_exact_resample_inputs


def _frac(a):
    return [Fraction(float(x)) for x in np.asarray(a, dtype=np.float64)]


@pytest.mark.parametrize("key", wr.scaled_case_keys(), ids=lambda k: "-".join(map(str, k)))
def test_scaled_exact_cases_are_exact(key):
    """1. Weights, sum and select are the intended rationals in the case's dtype; the running sum in the dtype over the
    expected normalised weights is K / G."""
    case = wr.scaled_case(key)
    dt = case.dtype.type
    w = case.raw_weights()
    assert w.dtype == case.dtype and np.all(np.isfinite(w)), case
    unit = Fraction(2) ** case.unit_exp
    assert _frac(w) == [int(k) * unit for k in case.k], case
    assert sum(_frac(w)) == case.sum_fraction() == Fraction(2) ** (3 + case.e)
    assert _frac(case.select()) == [Fraction(int(t), case.G) for t in case.base.t]
    wn = case.norm_weights()
    assert _frac(wn) == [Fraction(int(k), case.G) for k in case.k]
    assert _frac(np.cumsum(wn, dtype=dt)) == [Fraction(int(K), case.G) for K in case.K]
    # the sum in double, as the device forms it, is exact too (a power of two; finite: f64 has no `beyond_max` case)
    assert Fraction(float(w.astype(np.float64).sum())) == case.sum_fraction()
    if case.name == "beyond_max":
        assert case.n == 257 and float(w.max()) <= float(np.finfo(dt).max) and float(w.astype(np.float64).sum()) > float(np.finfo(dt).max)
    # (n = 10: G = 2^7, so at a sum of 2^(emin+6) the unit is 2^(emin-1) and only a weight of k = 1 would be subnormal;
    # the case has none.  n = 257, G = 2^12, has them.)
    if (case.name == "some_subnormal" and case.n == 257) or case.name == "unit_tiny":
        assert np.any((w > 0) & (w < np.finfo(dt).tiny)), "no subnormal weight"
    if case.name == "unit_tiny":
        assert case.unit_exp == wr.tiny_exp(dt) and float(w[w > 0].min()) == int(case.k[case.k > 0].min()) * float(np.finfo(dt).smallest_subnormal)


@pytest.mark.parametrize("key", wr.scaled_case_keys(), ids=lambda k: "-".join(map(str, k)))
def test_oracle_on_scaled_exact_cases(key):
    """2. For sums at or below T's largest finite number the oracle (w / sum in T, PF.cpp:482-487) gives k / G and keep[]
    bit for bit.  Beyond it the oracle's own sum is +inf: every weight becomes 0 and nothing is resampled -- it FAILS the
    case, which is why the exact rational is the only reference there."""
    case = wr.scaled_case(key)
    o = Oracle(case.dtype.type)
    w = case.raw_weights()
    with np.errstate(all="ignore"):
        neff, did, keep = o.pf_normalize_resample(w, case.n + 1, True, case.select())
    if case.overflows_oracle:
        assert not did and not np.array_equal(keep, case.keep) and not w.any(), (case, neff, did)
        return
    assert did and np.array_equal(keep, case.keep), case
    assert np.all(w == case.dtype.type(1.0 / case.n))
    w = case.raw_weights()
    neff, did, _ = o.pf_normalize_resample(w, case.n + 1, False, case.select())
    assert not did and w.tobytes() == case.norm_weights().tobytes(), case
    assert abs(float(neff) - case.neff) <= NEFF_TOL[case.dtype] * case.neff
    assert np.array_equal(stratified_keep(w, case.select()), case.keep)


def test_negative_control_the_old_normalisation_on_the_new_cases():
    """3. The device's former normalisation w * (T)(1 / ws), restated in numpy, on the new cases; then the rule it follows
    now (wr.device_rule).  Measured here:
      old form, sums 2^(emin-2) and G * tiny, f32 and f64, n = 10 and 257: every positive weight inf, every zero NaN;
      old form, sum 2^(emin-1) (reciprocal 2^127 / 2^1023): still exact;
      old form, non-power-of-two sum in [2^133, 2^134), f32, n = 257: up to 23 ulp from the correctly rounded k / K -- the
        scale is a subnormal with 16 bits; in [2^1023, 2^1024), f64: 1 ulp (the double sum can go no higher; the scale keeps
        51 bits);
      old form, non-power-of-two sums in the subnormal range: inf;
      new rule: k / G bit for bit on every scaled exact case, the correctly rounded k / K (0 ulp) on the non-power-of-two
        sums."""
    for key in wr.scaled_case_keys():
        case = wr.scaled_case(key)
        old, new = wr.device_old_form(case.raw_weights(), case.dtype), wr.device_rule(case.raw_weights(), case.dtype)
        assert new.tobytes() == case.norm_weights().tobytes(), case
        if case.name in ("reciprocal_overflows", "unit_tiny"):
            assert np.all(np.isinf(old[case.k > 0])) and np.all(np.isnan(old[case.k == 0])) and (case.k == 0).any(), case
        else:
            assert old.tobytes() == case.norm_weights().tobytes(), case   # powers of two: a subnormal scale is still exact
    for key in wr.NONPOW2_KEYS:
        case = wr.nonpow2_case(key)
        want = case.expected()
        e_old = wr.ulps(wr.device_old_form(case.raw_weights(), case.dtype), want).max()
        e_new = wr.ulps(wr.device_rule(case.raw_weights(), case.dtype), want).max()
        print(f"{case}: old form {e_old:.3g} ulp, new rule {e_new:.3g} ulp")
        assert e_new <= 0.5, (case, e_new)
        if case.where == "sub":
            assert np.isinf(e_old), case
        elif case.dtype == np.float32:
            assert 2.0 < e_old < np.inf, (case, e_old)
        else:
            assert e_old <= 2.0, (case, e_old)


@pytest.mark.parametrize("key", wr.NONPOW2_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_non_power_of_two_cases_are_where_they_should_be(key):
    case = wr.nonpow2_case(key)
    w, em = case.raw_weights(), wr.emin(case.dtype)
    assert _frac(w) == [int(k) * Fraction(2) ** case.unit_exp for k in case.k]
    s = case.sum_fraction()
    assert Fraction(float(w.astype(np.float64).sum())) == s, "the double sum is not exact"
    if case.where == "sub":
        assert Fraction(2) ** (em - 4) <= s < Fraction(2) ** (em - 3)
    else:
        assert Fraction(2) ** (-em + 1) < s < Fraction(2) ** (-em + 8)
    assert case.k.min() >= 1 and case.k.max() <= 2 ** 12 and case.K & (case.K - 1)
    # the same-dtype oracle (one division in T) is within the derived 2 ulp wherever its sum is finite
    if s <= Fraction(float(np.finfo(case.dtype).max)):
        wo = w.copy()
        Oracle(case.dtype.type).pf_normalize_resample(wo, case.n + 1, False, np.zeros(case.n, case.dtype))
        assert wr.ulps(wo, case.expected()).max() <= 2.0, case


@pytest.mark.parametrize("key", wr.degenerate_keys(), ids=lambda k: "-".join(k))
def test_degenerate_sets_on_the_oracle(key):
    """4. All weights zero, one NaN: Neff NaN, nothing resampled, weights the IEEE w / sum w.  Recorded for one +inf: the
    same (finite / inf = 0, inf / inf = NaN, Neff NaN).  Recorded for the f64 set whose sum overflows: every weight 0,
    Neff NaN, nothing resampled.  This is the rule a handle follows under CSLAM_PF_REPORT
    (test_pf_weight_range_gpu.py::test_degenerate_sums_are_reported_not_resampled)."""
    kind, dtn = key
    dt = np.dtype(dtn).type
    case, w = wr.degenerate_weights(kind, dt)
    want = wr.ieee_quotients(w, dt)
    with np.errstate(all="ignore"):
        neff, did, _ = Oracle(dt).pf_normalize_resample(w, case.n + 1, True, case.select(dt))
    assert not did, key
    assert np.array_equal(w, want, equal_nan=True), (key, w, want)
    assert np.isnan(neff), (key, neff)
    assert {"zero": np.isnan(want).all(), "nan": np.isnan(want).all(), "inf": np.isnan(want).sum() == 1 and not np.nansum(want),
            "overflow": not want.any()}[kind]


class _Shard:
    """Numpy stand-in with ParticleShard's host-planned resample surface, arithmetic as the kernels do it."""

    def __init__(self, w):
        self.dtype, self.w, self.n_local, self.order = np.dtype(w.dtype), w.copy(), w.shape[0], np.arange(w.shape[0])
        self.calls = []

    def weight_sums(self):
        with np.errstate(all="ignore"):
            w = self.w.astype(np.float64)
            return float(w.sum()), float((w * w).sum())

    def scale_weights(self, s):
        self.calls.append("scale")
        self.w = (self.w * self.dtype.type(s)).astype(self.dtype)

    def divide_weights(self, ws):
        self.calls.append("divide")
        with np.errstate(all="ignore"):
            self.w = (self.w.astype(np.float64) / np.float64(ws)).astype(self.dtype)

    def get_weights(self):
        return self.w.copy()

    def gather_local(self, keep, w_new):
        self.order = self.order[keep]
        self.w[:] = self.dtype.type(w_new)


def test_host_planned_path_over_the_range():
    """conan_slam_amd.pf.resample_particles (the host-planned route) on a numpy stand-in: k / G and keep[] on every scaled
    exact case, the scale kept wherever it is a normal number of T; on a shard that reports degenerate sums, (nan, False) and
    the IEEE quotients on the degenerate sets, where the path otherwise raises ZeroDivisionError on a sum of 0."""
    for key in wr.scaled_case_keys():
        case = wr.scaled_case(key)
        sh = _Shard(case.raw_weights())
        neff, did = resample_particles(sh, SingleComm(), case.n + 1, False, select=case.select())
        assert not did and sh.w.tobytes() == case.norm_weights().tobytes(), case
        assert abs(neff - case.neff) <= 1e-12 * case.neff, (case, neff)
        scale_is_normal = wr.emin(case.dtype) <= -case.sum_exp <= -wr.emin(case.dtype) + 1
        assert sh.calls == (["scale"] if scale_is_normal else ["divide"]), (case, sh.calls)
        sh = _Shard(case.raw_weights())
        neff, did = resample_particles(sh, SingleComm(), case.n + 1, True, select=case.select())
        assert did and np.array_equal(sh.order, case.keep) and np.all(sh.w == case.dtype.type(1.0 / case.n)), case
    for kind, dtn in wr.degenerate_keys():
        case, w = wr.degenerate_weights(kind, np.dtype(dtn).type)
        sh = _Shard(w)
        sh.report_degenerate = True
        neff, did = resample_particles(sh, SingleComm(), case.n + 1, True, select=case.select(np.dtype(dtn).type))
        assert np.isnan(neff) and did is False, (kind, dtn, neff, did)
        assert np.array_equal(sh.w, wr.ieee_quotients(w, np.dtype(dtn).type), equal_nan=True) and np.array_equal(sh.order, np.arange(case.n))

@pytest.mark.parametrize("dtype", wr.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", wr.PROPOSAL_SHAPES, ids=lambda s: f"m{s[0]}-np{s[1]}")
@pytest.mark.parametrize("kernel", wr.KERNELS)
def test_proposal_scaling_exponents(kernel, shape, dtype):
    """5a. The largest |e| in each direction for which the same-dtype oracle's weights are bit for bit 2^e x its e = 0
    weights for every particle, found by search; wr.E_NORMAL records that |e| minus 2.  For the sibling the oracle is
    pf_assoc_ref.consumer_reference, searched in both orders of the miss factor (after the product, as it multiplies; inside
    the likelihood, as the device and cslam.h do: wr.oracle_weights) and the smaller |e| counts.  The recorded exponents,
    and the ones next to them, are re-checked directly."""
    case = wr.proposal_case(kernel, shape, dtype)
    found = wr.exact_exponents(kernel, case, 300 if dtype == np.float32 else 2200)
    rec = wr.E_NORMAL[(kernel, shape[0], np.dtype(dtype).name)]
    print(f"{kernel} m={shape[0]} {np.dtype(dtype).name}: exact for e in [-{found[0]}, +{found[1]}], recorded -{rec[0]} / +{rec[1]}")
    assert rec == (found[0] - 2, found[1] - 2), (kernel, shape, found, rec)
    for sign, r_ in zip((-1, +1), rec):
        for e in (r_, r_ + 1, r_ + 2, r_ // 2):
            for order in ((False, True) if kernel == "assoc" else (False,)):
                assert wr.scales_exactly(kernel, case, sign * e, miss_first=order), (kernel, shape, sign * e, order)
    if kernel == "assoc":   # the sibling's product holds the miss factor: somebody has no match for a used observation
        assert ((case.idf == 0) & (case.use[:, None] == 1)).any() and (case.idf != 0).any(), case


@pytest.mark.parametrize("shape", wr.PROPOSAL_SHAPES, ids=lambda s: f"m{s[0]}-np{s[1]}")
@pytest.mark.parametrize("kernel", wr.KERNELS)
def test_subnormal_exponents(kernel, shape):
    """5b (f32).  By the f64 oracle on the inputs as f32 holds them, over the exponents wr.E_SUB records: an e with a
    quarter of the particles in [2^-149, 2^-126) and one normal weight; for the sibling also an e with a quarter there and
    one weight below 2^-150.  The plain kernel cannot be given a weight below 2^-150 on these clouds -- asserted: its
    smallest likelihood * prior / proposal factor is above 1, and an f32 input weight is 0 or at least 2^-149."""
    case = wr.proposal_case(kernel, shape, np.float32)
    quarter = -(-case.np_ // 4)
    census = {}
    for e in wr.E_SUB[(kernel, shape[0])]:
        wh = wr.oracle_weights(kernel, case, np.float64, e)
        wc = wr.oracle_weights(kernel, case, np.float32, e)
        census[e] = wr.sub_census(wh)
        assert np.all(np.isfinite(wc)) and np.all(wc >= 0)
        print(f"{kernel} m={shape[0]} e={e}: (subnormal, normal, below 2^-150) = {census[e]}; f32 oracle max / median "
              f"error {wr.sub_errors(wc, wc, wh)[2]:.3e} / {wr.sub_errors(wc, wc, wh)[3]:.3e}")
        assert census[e][0] >= quarter, (kernel, shape, e, census[e])
    assert any(n >= 1 for _, n, _ in census.values()), census
    if kernel == "assoc":
        assert any(b >= 1 for _, _, b in census.values()), census
    else:
        w_in = np.array([p[0] for p in case.parts], dtype=np.float64)
        factor = wr.oracle_weights(kernel, case, np.float64, 0) / w_in
        assert factor.min() > 1.0, (kernel, shape, factor.min())
