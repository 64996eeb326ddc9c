"""Builders and references of the particle-weight tests at the ENDS of the floating-point range
(test_pf_weight_range_cpu.py, test_pf_weight_range_gpu.py).

Everything else in the suite keeps the weights in the middle of the format.  Here:
  * SCALED EXACT CASES: pf_builders.ExactResampleCase times 2^e.  The integer weights k[i] * 8 / G (G a power of two)
    stay exactly representable as long as the unit 2^(3 - log2 G + e) is at least the smallest subnormal of T, so the
    expected normalised weights k / G, the running sums and keep[] are the case's own for every e;
  * NON-POWER-OF-TWO SUMS: integer weights k[i] in [1, 2^12] times a power-of-two unit whose sum K is no power of two;
    the expected weights are k[i] / K computed exactly (fractions.Fraction) and rounded once to T;
  * DEGENERATE SETS: all weights zero, one NaN, one +inf (and, for f64, finite weights whose double sum is +inf);
  * SCALED PROPOSAL CASES: pf_builders.ProposalCase with every input weight times 2^e, for pf_sample_proposal_kernel and
    for its sibling pf_sample_proposal_assoc_kernel (per-particle correspondences, the `miss` factor in the product).
test_pf_weight_range_cpu.py proves the stated properties on the CPU oracle alone and finds the exponents recorded here.
"""
import copy
from fractions import Fraction

import numpy as np

import pf_assoc_ref as aref
from pf_builders import ExactResampleCase, ProposalCase, copy_parts, oracle_chain

DTYPES = [np.float32, np.float64]
EMIN = {np.dtype(np.float32): -126, np.dtype(np.float64): -1022}      # exponent of the smallest normal number
TINY_EXP = {np.dtype(np.float32): -149, np.dtype(np.float64): -1074}  # exponent of the smallest subnormal


def emin(dtype):
    return EMIN[np.dtype(dtype)]


def tiny_exp(dtype):
    return TINY_EXP[np.dtype(dtype)]


def scale2(a, e, dtype):
    """a * 2^e formed in f64 steps that cannot overflow before the end, cast to dtype (exact whenever the result is
    representable: the callers assert that)."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(a, e).astype(dtype)


def ulps(got, want):
    """|got - want| in units of the spacing of `want` (its own dtype); inf where got is not finite."""
    got, want = np.asarray(got), np.asarray(want)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    return np.where(np.isfinite(got), d, np.inf)


# ------------------------------------------------------------------------------------------------
# scaled exact cases
# ------------------------------------------------------------------------------------------------
SUM_NAMES = ("control", "some_subnormal", "last_finite_reciprocal", "reciprocal_overflows", "unit_tiny",
             "scale_smallest_normal", "scale_subnormal", "beyond_max")


class ScaledExactCase:
    """ExactResampleCase(n) with every weight times 2^e: sum w = 2^sum_exp.  keep[], k / G, K / G and Neff are the base
    case's.  `overflows_oracle`: the sum is beyond T's largest finite number (the same-dtype oracle's own sum is inf)."""

    def __init__(self, n, dtype, name, sum_exp):
        self.n, self.dtype, self.name, self.sum_exp = n, np.dtype(dtype), name, sum_exp
        self.base = ExactResampleCase(n)
        self.G, self.k, self.K, self.keep, self.neff = self.base.G, self.base.k, self.base.K, self.base.keep, self.base.neff
        self.e = sum_exp - 3
        self.unit_exp = sum_exp - int(np.log2(self.G))
        assert self.unit_exp >= tiny_exp(dtype), (self, "the unit weight is below the smallest subnormal")
        self.overflows_oracle = sum_exp > -emin(dtype) + 1

    def raw_weights(self):
        return scale2(self.k, self.unit_exp, self.dtype)

    def norm_weights(self):
        return self.base.norm_weights(self.dtype)

    def select(self):
        return self.base.select(self.dtype)

    def sum_fraction(self):
        return Fraction(2) ** self.sum_exp

    def __repr__(self):
        return f"ScaledExactCase({self.name}, n={self.n}, {self.dtype.name}, sum=2^{self.sum_exp})"


def sum_exponents(dtype, G):
    em = emin(dtype)
    return {"control": 3, "some_subnormal": em + 6, "last_finite_reciprocal": em - 1, "reciprocal_overflows": em - 2,
            "unit_tiny": int(np.log2(G)) + tiny_exp(dtype), "scale_smallest_normal": -em, "scale_subnormal": -em + 1,
            "beyond_max": -em + 4}


def scaled_case_keys(ns=(10, 257)):
    """(name, n, dtype name) of every scaled exact case.  `beyond_max` exists for f32 only (in f64 the DOUBLE sum is +inf:
    that is the degenerate set `overflow`) and only for an n whose largest weight is still finite in T."""
    keys = []
    for dt in DTYPES:
        for n in ns:
            base = ExactResampleCase(n)
            for name in SUM_NAMES:
                if name == "beyond_max":
                    top = float(base.k.max()) / base.G * 2.0 ** (-emin(dt) + 4) if dt == np.float32 else np.inf
                    if not top <= float(np.finfo(dt).max):
                        continue
                keys.append((name, n, np.dtype(dt).name))
    return keys


def scaled_case(key):
    name, n, dt = key
    return ScaledExactCase(n, np.dtype(dt).type, name, sum_exponents(np.dtype(dt), ExactResampleCase(n).G)[name])


# ------------------------------------------------------------------------------------------------
# sums that are no power of two
# ------------------------------------------------------------------------------------------------
class NonPow2Case:
    """n integer weights k[i] in [1, 2^12] times 2^unit_exp, sum K * 2^unit_exp with K no power of two.
    where = "sub": the sum lies in [2^(emin-4), 2^(emin-3)), inside the subnormal range of T and below the 2^(emin-2)
    from which the reciprocal overflows T.  where = "top": in [2^133, 2^134) for f32 (the scale (T)(1/ws) is a subnormal
    with 16 bits left), in [2^1023, 2^1024) for f64 (the double sum can go no further; the scale keeps 51 bits)."""

    def __init__(self, n, dtype, where):
        self.n, self.dtype, self.where = n, np.dtype(dtype), where
        rng = np.random.default_rng(77_000 + n + (1 if where == "top" else 0))
        self.k = rng.integers(1, 2 ** 12 + 1, size=n).astype(np.int64)
        self.K = int(self.k.sum())
        assert self.K & (self.K - 1), "K is a power of two"
        lg = self.K.bit_length() - 1
        if where == "sub":
            self.unit_exp = emin(dtype) - 4 - lg
        else:
            self.unit_exp = (133 if self.dtype == np.float32 else 1023) - lg
        assert self.unit_exp >= tiny_exp(dtype), self
        self.neff = float(Fraction(self.K * self.K, int((self.k * self.k).sum())))

    def raw_weights(self):
        w = scale2(self.k, self.unit_exp, self.dtype)
        assert np.all(np.isfinite(w)) and np.all(w > 0)
        return w

    def sum_fraction(self):
        return Fraction(self.K) * Fraction(2) ** self.unit_exp

    def expected(self):
        """k[i] / K exactly, rounded once to T (through f64 for f32: 53 >= 2 * 24 + 2 makes the double rounding innocuous;
        Fraction -> float is correctly rounded)."""
        return np.array([float(Fraction(int(ki), self.K)) for ki in self.k], dtype=np.float64).astype(self.dtype)

    def __repr__(self):
        return f"NonPow2Case({self.where}, n={self.n}, {self.dtype.name}, K={self.K}, unit=2^{self.unit_exp})"


NONPOW2_KEYS = [(where, n, np.dtype(dt).name) for dt in DTYPES for where, n in (("sub", 10), ("sub", 257), ("top", 257))]


def nonpow2_case(key):
    where, n, dt = key
    return NonPow2Case(n, np.dtype(dt).type, where)


def device_old_form(w, dtype):
    """The normalisation as the device did it: w * (T)(1 / ws) with ws the f64 sum.  The negative control."""
    t = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        ws = np.asarray(w, dtype=np.float64).sum()
        return (np.asarray(w, dtype=dtype) * t(np.float64(1.0) / ws)).astype(dtype)


def device_rule(w, dtype):
    """The rule the device follows now, restated: the scale where (T)(1 / ws) is a normal number of T, else the quotient
    (T)((double)w / ws), one rounding."""
    t, fi = np.dtype(dtype).type, np.finfo(dtype)
    with np.errstate(all="ignore"):
        w64 = np.asarray(w, dtype=np.float64)
        ws = w64.sum()
        scale = t(np.float64(1.0) / ws)
        if 0.0 < ws <= np.finfo(np.float64).max and fi.tiny <= scale <= fi.max:
            return (np.asarray(w, dtype=dtype) * scale).astype(dtype)
        return (w64 / ws).astype(dtype)


# ------------------------------------------------------------------------------------------------
# degenerate sets
# ------------------------------------------------------------------------------------------------
DEGENERATE_N = 16
DEGENERATE_KINDS = {np.dtype(np.float32): ("zero", "nan", "inf"), np.dtype(np.float64): ("zero", "nan", "inf", "overflow")}


def degenerate_keys():
    return [(kind, dt.name) for dt in DEGENERATE_KINDS for kind in DEGENERATE_KINDS[dt]]


def degenerate_weights(kind, dtype):
    """Raw weights of a healthy ExactResampleCase(16) made degenerate.  `overflow` (f64): every weight finite, their sum
    in double +inf."""
    case = ExactResampleCase(DEGENERATE_N)
    w = case.raw_weights(dtype)
    j = int(np.argmax(case.k))
    if kind == "zero":
        w[:] = 0
    elif kind == "nan":
        w[j] = np.nan
    elif kind == "inf":
        w[j] = np.inf
    else:
        assert kind == "overflow" and np.dtype(dtype) == np.float64
        w = scale2(case.k, 1026 - int(np.log2(case.G)), dtype)
        assert np.all(np.isfinite(w))
    return case, w


def ieee_quotients(w, dtype):
    """w / sum w as IEEE arithmetic gives it with the sum formed in double: the weights a degenerate set is left with."""
    with np.errstate(all="ignore"):
        w64 = np.asarray(w, dtype=np.float64)
        return (w64 / w64.sum()).astype(dtype)


# ------------------------------------------------------------------------------------------------
# scaled proposal cases
# ------------------------------------------------------------------------------------------------
PROPOSAL_SHAPES = [(1, 65), (9, 65)]
MISS = 1e-3
KERNELS = ("proposal", "assoc")
_CASES = {}


def scaled_parts(parts, e, dtype):
    ps = copy_parts(parts, np.dtype(dtype).type)
    for p in ps:
        p[0] = scale2(p[0], e, dtype)[()]
    return ps


def make_proposal_case(m, np_, dtype):
    """ProposalCase(m, np); m = 1 (below what its shuffled feature list can build): the first observation of the m = 2
    case on the same cloud."""
    if m >= 2:
        return ProposalCase(m, np_, dtype)
    case = ProposalCase(2, np_, dtype)
    case.m, case.idf, case.Z = 1, case.idf[:1].copy(), np.asfortranarray(case.Z[:, :1])
    return case


class AssocProposalCase:
    """ProposalCase(m, np) for pf_sample_proposal_assoc_kernel: every particle takes its correspondences from a table.
    gate1 is the median over the particles of the smallest nis of observation 0 (f64 restatement of EKF.cpp:131-144), so
    about half the particles have no match for it and pay MISS: the `miss` factor is in the product.  `idf`: the f64
    reference's table [m, np] (the GPU test feeds the oracle with the table the device returned)."""

    def __init__(self, m, np_, dtype):
        self.case = make_proposal_case(m, np_, dtype)
        self.m, self.np_, self.dtype, self.nf = m, np_, np.dtype(dtype), self.case.nf
        self.parts, self.Z, self.R, self.normals = self.case.parts, self.case.Z, self.case.R, self.case.normals
        ac = aref.Case("weight-range", dtype, self.parts, self.Z, R=self.R.astype(np.float64))
        nis, _ = ac.ref()
        g1 = float(np.median(nis[:, 0, :].min(axis=1)))
        self.gates = (g1, 4.0 * g1)
        ac.gates = (self.gates,)
        self.idf = ac.decisions(self.gates)[0]
        self.use = np.ones(m, np.int32)

    def __repr__(self):
        return f"AssocProposalCase(m={self.m}, np={self.np_}, {self.dtype.name}, gates={self.gates})"


def proposal_case(kernel, shape, dtype):
    key = (kernel, shape, np.dtype(dtype).name)
    if key not in _CASES:
        _CASES[key] = make_proposal_case(*shape, dtype) if kernel == "proposal" else AssocProposalCase(*shape, dtype)
    return _CASES[key]


def oracle_weights(kernel, case, dt, e, idf=None, miss_first=False):
    """The weights after the proposal of `case` with every input weight times 2^e, on the CPU oracle in precision dt (the
    inputs are the case's own-dtype values, scaled in the case's dtype, then converted).  assoc: `idf` is the table to
    take the correspondences from (default: the case's f64 reference table).
    miss_first (assoc): pf_assoc_ref.consumer_reference multiplies the finished weight w * like * prior / prop by
    miss_likelihood once per unmatched observation; the device -- and include/cslam.h -- put that factor INTO the
    likelihood product, ahead of prior and proposal.  The values agree to rounding, but the intermediate w * like * prior
    is smaller on the device by miss^k, which matters for where exact scaling ends.  miss_first restates that order with
    the oracle: the input weight takes the factors (in dt, before the scaling), consumer_reference runs with a factor 1."""
    if kernel == "proposal":
        c = copy.copy(case)
        c.parts = scaled_parts(case.parts, e, case.dtype)
        return np.array([p[0] for p in oracle_chain(c, dt)], dtype=dt)
    idf = case.idf if idf is None else idf
    if not miss_first:
        parts = scaled_parts(case.parts, e, case.dtype)
        ps = aref.consumer_reference(parts, dt, case.Z, case.R, idf, case.use, case.normals, MISS)
        return np.array([p[0] for p in ps], dtype=dt)
    parts = copy_parts(case.parts, dt)
    misses = ((idf == 0) & (case.use[:, None] == 1)).sum(axis=0)
    for p, k in zip(parts, misses):
        w = dt(p[0])
        for _ in range(int(k)):
            w = dt(w * dt(MISS))
        p[0] = scale2(w, e, dt)[()]
    ps = aref.consumer_reference(parts, dt, case.Z, case.R, idf, case.use, case.normals, 1.0)
    return np.array([p[0] for p in ps], dtype=dt)


def scales_exactly(kernel, case, e, w0=None, miss_first=False):
    """Are the same-dtype oracle's weights at 2^e bit for bit 2^e x its weights at e = 0, for every particle?"""
    dt = case.dtype.type if isinstance(case.dtype, np.dtype) else case.dtype
    w0 = oracle_weights(kernel, case, dt, 0, miss_first=miss_first) if w0 is None else w0
    we = oracle_weights(kernel, case, dt, e, miss_first=miss_first)
    want = scale2(w0, e, dt)
    return bool(np.all(np.isfinite(we)) and np.array_equal(we, want) and np.all(want > 0))


def largest_exact_exponent(kernel, case, sign, limit, window=24, miss_first=False):
    """The largest |e| <= limit, in direction `sign`, such that scales_exactly holds there AND at the `window` exponents
    before it.  Bisection finds a boundary; near the edge exactness is not monotone (a product that has just become
    subnormal can still be exact when its low bits happen to be zero), so the exponents under the answer are checked one
    by one and the search repeated below the first that fails."""
    dt = case.dtype.type if isinstance(case.dtype, np.dtype) else case.dtype
    w0 = oracle_weights(kernel, case, dt, 0, miss_first=miss_first)

    def ok(e):
        return scales_exactly(kernel, case, sign * e, w0, miss_first)
    assert not ok(limit), "the search limit is inside the exact range"
    hi = limit
    while True:
        lo = 0                     # exact at lo, not exact at hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if ok(mid) else (lo, mid)
        bad = [e for e in range(max(lo - window, 1), lo) if not ok(e)]
        if not bad:
            return lo
        hi = min(bad)


def exact_exponents(kernel, case, limit):
    """(|e| down, |e| up) of the largest exact scaling; for the sibling the smaller of the two orders of the miss factor."""
    orders = (False, True) if kernel == "assoc" else (False,)
    return tuple(min(largest_exact_exponent(kernel, case, sign, limit, miss_first=o) for o in orders) for sign in (-1, +1))


# |e| of the largest exact scaling found by test_pf_weight_range_cpu.py::test_proposal_scaling_exponents, minus 2:
# (kernel, m, dtype name) -> (E_NORMAL-, E_NORMAL+), both given as positive numbers
E_NORMAL = {
    ("proposal", 1, "float32"): (114, 126), ("proposal", 1, "float64"): (1009, 1022),
    ("proposal", 9, "float32"): (117, 110), ("proposal", 9, "float64"): (1018, 1006),
    ("assoc", 1, "float32"): (100, 126), ("assoc", 1, "float64"): (996, 1022),
    ("assoc", 9, "float32"): (58, 113), ("assoc", 9, "float64"): (954, 1009),
}

# f32: the exponents that put the weights across the bottom of the range, (kernel, m) -> tuple of e.  By the f64 oracle on
# the inputs as f32 holds them (an input weight of 2^e / 65 is itself a subnormal below e = -120 and loses bits: device and
# oracles are given the same rounded value), test_pf_weight_range_cpu.py::test_subnormal_exponents asserts:
#   assoc     over the tuple, an e with a quarter of the particles in [2^-149, 2^-126) and one normal weight, and an e
#             with a quarter there and one below 2^-150 (m = 9: one e does both; m = 1: two);
#   proposal  a quarter subnormal and one normal.  NO exponent gives the plain kernel a weight below 2^-150: on these
#             clouds every particle's likelihood * prior / proposal is above 1 (the densities of a 0.3 m cloud are
#             large), so the weight leaves the call larger than it came, and an f32 input is 0 or at least 2^-149.  The
#             sibling has the factor miss_likelihood = 1e-3 per unmatched observation and does get there.
E_SUB = {("proposal", 1): (-122,), ("proposal", 9): (-135,), ("assoc", 1): (-122, -135), ("assoc", 9): (-90,)}


def sub_census(wh):
    """(subnormal, normal, below 2^-150) counts of f64-oracle weights against the f32 format."""
    wh = np.asarray(wh, dtype=np.float64)
    return (int(((wh >= 2.0 ** -149) & (wh < 2.0 ** -126)).sum()), int((wh >= 2.0 ** -126).sum()),
            int((wh < 2.0 ** -150).sum()))


def sub_errors(g, wc, wh):
    """The E_SUB measure |x - wh| / max(wh, 2^-126) against the f64 oracle's weights wh (one step of the subnormal grid
    is one ulp in it) -> (device max, device median, CPU max, CPU median)."""
    g, wc, wh = (np.asarray(a, dtype=np.float64) for a in (g, wc, wh))
    den = np.maximum(wh, 2.0 ** -126)
    eg, ec = np.abs(g - wh) / den, np.abs(wc - wh) / den
    return float(eg.max()), float(np.median(eg)), float(ec.max()), float(np.median(ec))
