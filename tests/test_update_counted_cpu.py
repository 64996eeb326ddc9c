"""cslam_ekf_update_counted without a device: the new entry points are declared and bound, and the oracle-side statement
the GPU tests rest on -- an update with c observations is the update with m_cap observations whose last m_cap - c rows
of H and innovations are zero (the zero-column argument: those rows give zero columns of P H^T, S is block diagonal, so
is the gain factor, and the last 2 (m_cap - c) columns of W1 are exact zeros that move neither X nor P)."""
import numpy as np
import pytest

from helpers import P_RTOL, X_RTOL, assert_close, make_obs, make_scenario
from np_restatement import REF_EXACT, TEXTBOOK, NpSlam

N = 70
R22 = np.diag([0.08, 0.0024])


def test_prototypes_are_declared_and_bound():
    from conan_slam_amd import EKF, _capi

    names = _capi.declared_symbols()
    for s in _capi.EKF_COUNTED_SYMBOLS:
        assert s in names and s in _capi._PROTOTYPES, s
    assert _capi.FACTOR_COUNT_CLAMPED == 64
    header = open(_capi.HEADER_PATH).read()
    assert "#define CSLAM_FACTOR_COUNT_CLAMPED 64" in header
    for meth in ("update_counted", "associate_deferred_async", "association_wait", "associate_update_counted"):
        assert callable(getattr(EKF, meth))


def _padded_update(s, X, P, Z, R, idf, c):
    """slam.h:235-266 on m_cap observations of which only the first c have their rows of H and V; -> X, P, W1"""
    m, n = Z.shape[1], X.shape[0]
    H = np.zeros((2 * m, n), dtype=s.dtype)
    V = np.zeros(2 * m, dtype=s.dtype)
    RR = np.zeros((2 * m, 2 * m), dtype=s.dtype)
    for i in range(m):
        RR[2 * i:2 * i + 2, 2 * i:2 * i + 2] = R
        if i < c:
            Zp, HT = s.observe_model(X, int(idf[i]))
            H[2 * i:2 * i + 2, :] = HT
            V[2 * i] = Z[0, i] - Zp[0]
            V[2 * i + 1] = s.pi2pi(Z[1, i] - Zp[1])
    PHT = P @ H.T
    G = s.gain_factor(s.make_symmetric(H @ PHT + RR))
    Xn, Pn = s.cholesky_update(X, P, V, RR, H)
    return Xn, Pn, PHT @ G


@pytest.mark.parametrize("quirks", [TEXTBOOK, REF_EXACT], ids=["textbook", "ref_exact"])
@pytest.mark.parametrize("m_cap,c", [(2, 1), (9, 1), (9, 8), (17, 8), (32, 1), (32, 31), (64, 33)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_zero_column_argument(dtype, m_cap, c, quirks):
    s = NpSlam(dtype, quirks)
    X, P = make_scenario(N, dtype, seed=100 + m_cap, corr=0.1)
    idf = (np.random.default_rng(m_cap).permutation(N) + 1)[:m_cap].astype(np.int32)
    Z = make_obs(X, idf, dtype, seed=m_cap)
    R = R22.astype(dtype)
    Xc, Pc = s.batch_update(X, P, np.asfortranarray(Z[:, :c]), R, idf[:c])
    Xp, Pp, W1 = _padded_update(s, X, P, Z, R, idf, c)
    assert np.all(W1[:, 2 * c:] == 0), "the padded columns of W1 are exact zeros"
    assert np.abs(W1[:, :2 * c]).max() > 0
    dt = np.dtype(dtype)
    assert_close("X", Xp, Xc, X_RTOL[dt])
    assert_close("P", Pp, Pc, P_RTOL[dt])
    assert not np.array_equal(Xc, X)  # (the update moved the state)
