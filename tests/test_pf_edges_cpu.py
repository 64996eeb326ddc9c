"""The input conditions of test_pf_edges_gpu.py, proved on the CPU oracle alone (no GPU):
  * tight cloud: for every (m, np, dtype) the GPU file gives to pf_sample_proposal_kernel, EVERY particle's weight is
    far inside the range of f32, so no particle has to be left out of a comparison;
  * exact resample inputs: the normalised weights and running sums are their exact rational values in f32 and f64, the
    cases hold ties select[c] == cum[i] and positions beyond cum[np-1], the oracle's keep[] equals stratified_keep and
    the integer reference, and a `<=` search would give a different keep[] (the cases can catch a wrong comparison)."""
import numpy as np
import pytest

from conan_slam_amd.pf import stratified_keep, stratified_random
from pf_builders import (DECISION_NP, DTYPES, ExactResampleCase, oracle_chain, proposal_case, proposal_case_keys,
                         resample_case_keys)
from pyoracle import Oracle


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", proposal_case_keys(), ids=lambda k: f"m{k[0]}-np{k[1]}-nf{k[2]}-pred{int(k[3])}")
def test_tight_cloud_weights_stay_in_range(key, dtype):
    """Every particle's f64-oracle weight in [1e-20, 1e20] and its f32-oracle weight finite and positive, for every
    proposal case of the GPU file built in this dtype (a cloud spread by 2 m underflows from about 12 factors on)."""
    case = proposal_case(key, dtype)
    assert len(set(case.idf.tolist())) == case.m and 1 in case.idf and case.nf in case.idf
    wh = np.array([p[0] for p in oracle_chain(case, np.float64)], dtype=np.float64)
    wc = np.array([p[0] for p in oracle_chain(case, np.float32)], dtype=np.float64)
    assert wh.shape == (case.np_,)
    assert np.all(wh >= 1e-20) and np.all(wh <= 1e20), (case, wh.min(), wh.max())
    assert np.all(np.isfinite(wc)) and np.all(wc > 0), (case, wc.min(), wc.max())
    print(f"{case}: f64 weights [{wh.min():.3e}, {wh.max():.3e}], f32 oracle within "
          f"{(np.abs(wc - wh) / wh).max():.1e} relative")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", resample_case_keys(), ids=lambda k: f"np{k[0]}-{'end' if k[1] else 'in'}")
def test_exact_resample_inputs(key, dtype):
    n, end = key
    case = ExactResampleCase(n, end=end)
    t = np.dtype(dtype).type
    o = Oracle(dtype)
    G = case.G
    w_raw, sel = case.raw_weights(dtype), case.select(dtype)
    # the inputs are exact in this dtype, zeros and a run of zeros among the weights
    assert np.array_equal(w_raw.astype(np.float64) * G, case.k * 8.0)
    assert np.array_equal(sel.astype(np.float64) * G, case.t.astype(np.float64))
    assert np.all(np.diff(sel) > 0)
    if n >= 16:
        z = case.k == 0
        assert z.sum() >= 2 and np.any(z[1:] & z[:-1]), "no run of zero weights"
    # the oracle's normalisation (w / sum in the dtype) and the device's (w * (T)(1 / sum_double)) give k / G exactly
    w = w_raw.copy()
    neff_o, did, keep_o = o.pf_normalize_resample(w, n + 1, False, sel)
    assert not did
    assert np.array_equal(w.astype(np.float64) * G, case.k.astype(np.float64))
    ws = float(w_raw.astype(np.float64).sum())
    assert ws == 8.0
    assert np.array_equal(w_raw * t(1.0 / ws), w)
    assert np.array_equal(w, case.norm_weights(dtype))
    # every running sum, summed sequentially in the dtype, is K / G exactly
    cum = np.cumsum(w, dtype=dtype)
    assert np.array_equal(cum.astype(np.float64) * G, case.K.astype(np.float64))
    assert cum[-1] == t(1)
    # ties, and the three references agree on keep[]
    assert case.ties >= (1 if n <= 16 else 8), case
    assert np.array_equal(keep_o, case.keep)
    assert np.array_equal(stratified_keep(w, sel), case.keep)
    w2 = w_raw.copy()
    _, did2, keep2 = o.pf_normalize_resample(w2, n + 1, True, sel)
    assert did2 and np.array_equal(keep2, case.keep) and np.all(w2 == t(1) / t(n))
    # a `<=` search decides at least one slot differently (with ONE particle keep[0] can only be 0: nothing to differ)
    left = np.searchsorted(cum, sel, side="left")
    left[left >= n] = 0
    if n > 1:
        assert np.any(left != case.keep), case
    # Neff: the oracle's value in the dtype against the exact rational one
    assert abs(float(neff_o) - case.neff) <= (1e-4 if dtype == np.float32 else 1e-12) * case.neff
    if end:
        # the last position is 1.0, not below cum[np-1] = 1.0: the search runs off the end and the slot keeps 0
        assert sel[-1] == t(1) and case.beyond[-1] and case.keep[-1] == 0 and case.k[0] >= 0
        assert np.searchsorted(cum, sel, side="right")[-1] == n
    else:
        assert case.keep[-1] == n - 1 or n == 1  # the last slot keeps the last particle: it reads the last running sums
    if case.pow2 and n > 1:
        # strata offsets in multiples of 1/8 (nextafter(1, 0) for the position 1.0): stratified_random is exact too
        u = case.uniforms(dtype)
        assert np.all(u < 1) and np.array_equal(u[u < 0.95] * 8, np.round(u[u < 0.95] * 8))
        assert np.array_equal(stratified_random(n, u, dtype), sel)
        assert np.array_equal(o.pf_stratified_random(n, u, ref_exact=False), sel)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", DECISION_NP)
def test_uniform_exact_weights_have_neff_equal_to_np(n, dtype):
    """The decision edge of the GPU file: uniform weights of 8/np normalise to exactly 1/np and Neff is exactly np, in the
    oracle's dtype arithmetic and in the device's double sums, so n_effective = np must not resample and np + 1 must."""
    case = ExactResampleCase(n, uniform=True)
    o = Oracle(dtype)
    t = np.dtype(dtype).type
    assert case.neff == float(n) and np.array_equal(case.keep, np.arange(n))
    for nmin, expect in ((n, False), (n + 1, True)):
        w = case.raw_weights(dtype)
        ws, ws2 = float(w.astype(np.float64).sum()), float((w.astype(np.float64) ** 2).sum())
        assert (ws * ws) / ws2 == float(n)
        neff, did, keep = o.pf_normalize_resample(w, nmin, True, case.select(dtype))
        assert float(neff) == float(n) and did == expect
        assert np.all(w == t(1) / t(n)) and np.array_equal(keep, case.keep)
