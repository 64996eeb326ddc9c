"""cslam_ekf_augment_device without a device: the new entry points are declared and bound; the fused form the kernel
implements (ekf_augment_kernels.hpp: every feature of a call built from pre-call data, the stripe rows of the earlier new
features RECOMPUTED from Gv and the 3 x 3 pose block) is EKF::addOneNewFeature applied q times; and the loop fixture of
test_augment_device_gpu.py (augment_loop.py) is decisive for every observation of every step on the CPU oracle alone."""
import numpy as np
import pytest

from augment_loop import N_NEW, NF0, NF_END, STEPS, get_loop
from helpers import make_scenario
from np_restatement import TEXTBOOK, NpSlam

R22 = np.array([[0.08, 0.004], [0.004, 0.0024]])


def test_prototypes_are_declared_and_bound():
    from conan_slam_amd import EKF, _capi

    names = _capi.declared_symbols()
    assert _capi.EKF_AUGMENT_DEVICE_SYMBOLS == ("cslam_ekf_augment_device", "cslam_ekf_augment_launches")
    for s in _capi.EKF_AUGMENT_DEVICE_SYMBOLS:
        assert s in names and s in _capi._PROTOTYPES, s
    assert _capi.EKF_AUGMENT_CHUNK >= 64
    src = open(_capi.HEADER_PATH.replace("include/cslam.h", "conan_slam_amd/csrc/ekf_augment_kernels.hpp")).read()
    assert f"constexpr int kAugChunk = {_capi.EKF_AUGMENT_CHUNK};" in src
    header = open(_capi.HEADER_PATH).read()
    for cite in ("test/main.cpp:188-189", "slam.h:190-191", "EKF.cpp:28-91"):
        assert cite in header, cite
    for meth in ("augment_device", "augment_launches", "associate_update_augment"):
        assert callable(getattr(EKF, meth))
    adapter = open(_capi.HEADER_PATH.replace("cslam.h", "cslam_adapter.hpp")).read()
    assert "augmentDevice(const void* dZ, int q, const Eigen::MatrixXf& R)" in adapter and "augmentAssociated(" in adapter


def jacobians(t, X, z):
    r, b = t(z[0]), t(z[1])
    s, c = t(np.sin(t(X[2] + b))), t(np.cos(t(X[2] + b)))
    Gv = np.array([[1, 0, -r * s], [0, 1, r * c]], dtype=t)
    Gz = np.array([[c, -r * s], [s, r * c]], dtype=t)
    return r, s, c, Gv, Gz


def fused_augment(dtype, X, P, Z, R, recompute=True):
    """The kernel's form: everything from X[0:3], the stripe P[0:3, 0:len0] with its 3 x 3 block, R and Z.  recompute=False
    is the negative control: the rows of the earlier new features are taken as they stand before the call (zero)."""
    t = np.dtype(dtype).type
    len0, q = X.shape[0], Z.shape[1]
    Xn = np.zeros(len0 + 2 * q, dtype=dtype)
    Pn = np.zeros((len0 + 2 * q, len0 + 2 * q), dtype=dtype)
    Xn[:len0], Pn[:len0, :len0] = X, P
    stripe, Pvv = P[0:3, 0:len0], P[0:3, 0:3]
    J = [jacobians(t, X, Z[:, f]) for f in range(q)]
    for f, (r, s, c, Gv, Gz) in enumerate(J):
        a = len0 + 2 * f
        Xn[a], Xn[a + 1] = X[0] + r * c, X[1] + r * s
        Pn[a:a + 2, a:a + 2] = Gv @ Pvv @ Gv.T + Gz @ R @ Gz.T          # EKF.cpp:74
        Pn[a:a + 2, 0:len0] = Gv @ stripe                              # EKF.cpp:77-78, 83-84
        Pn[0:len0, a:a + 2] = Pn[a:a + 2, 0:len0].T
        for g in range(f):                                              # the rows an earlier feature of the call added
            Gg = J[g][3]
            col = (Gg @ Pvv).T if recompute else np.zeros((3, 2), dtype=dtype)  # P[0:3, rows of g] after g's augment
            b = len0 + 2 * g
            Pn[a:a + 2, b:b + 2] = Gv @ col
            Pn[b:b + 2, a:a + 2] = Pn[a:a + 2, b:b + 2].T
    return Xn, Pn


@pytest.mark.parametrize("N0,q", [(0, 1), (0, 3), (4, 2), (20, 40)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_fused_form_is_add_one_new_feature_q_times(dtype, N0, q):
    s = NpSlam(dtype, TEXTBOOK)
    X, P = make_scenario(N0, dtype, seed=300 + N0 + q)
    rng = np.random.default_rng(N0 + 7 * q)
    Z = np.asfortranarray(np.stack([rng.uniform(5.0, 40.0, q), rng.uniform(-3.0, 3.0, q)]).astype(dtype))
    R = R22.astype(dtype)
    Xr, Pr = s.augment(X, P, Z, R)
    Xf, Pf = fused_augment(dtype, X, P, Z, R)
    assert Xf.shape == Xr.shape == (3 + 2 * (N0 + q),)
    assert np.array_equal(Xf, Xr)
    # Every entry is one or two nested products of at most three terms with |Gv| <= 1 + r: two orders of evaluation differ
    # by a few roundings of the sum of the absolute terms, which 9 (1 + r)^2 max|P| + 4 (1 + r)^2 max|R| bounds.
    g = (1.0 + float(np.abs(Z[0]).max())) ** 2
    bound = 8.0 * float(np.finfo(dtype).eps) * g * (9.0 * float(np.abs(P).max()) + 4.0 * float(np.abs(R).max()))
    assert float(np.abs(Pf.astype(np.float64) - Pr.astype(np.float64)).max()) <= bound
    assert np.array_equal(Pf[: X.shape[0], : X.shape[0]], P)
    if q > 1:   # negative control: without the recomputed stripe the new x new cross blocks are wrong
        Pz = fused_augment(dtype, X, P, Z, R, recompute=False)[1]
        assert float(np.abs(Pz.astype(np.float64) - Pr.astype(np.float64)).max()) > 10.0 * bound


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_every_observation_of_every_step_of_the_loop_is_decisive(dtype):
    steps, X_end, P_end = get_loop(dtype)
    assert len(steps) == STEPS == 8
    n, seen_new = 3 + 2 * NF0, 0
    for t, s in enumerate(steps):
        assert s["n"] == n, (t, s["n"], n)
        assert s["Z"].shape == (2, 7 + N_NEW[t]) and s["Z"].dtype == np.dtype(dtype)
        assert s["margin"] >= s["tau"] > 0, (t, s["margin"], s["tau"])          # every observation: the minimum
        assert np.array_equal(s["kind"], s["intended"]), (t, s["kind"], s["intended"])
        assert [int((s["kind"] == k).sum()) for k in (1, 2, 0)] == [5, N_NEW[t], 2], t
        own = s["idf"][s["kind"] == 1]
        assert np.all(own > 0) and np.all(s["idf"][s["kind"] != 1] == 0) and len(set(own)) == 5
        # features that an earlier step augmented are re-observed and associate
        assert int((own > NF0).sum()) == min(seen_new, 2), (t, own)
        assert np.all(own <= NF0 + seen_new)
        seen_new += N_NEW[t]
        n += 2 * N_NEW[t]
    assert X_end.shape == (3 + 2 * NF_END,) and P_end.shape == (3 + 2 * NF_END,) * 2
    assert 3 + 2 * NF0 < 128 < 3 + 2 * NF_END      # the map grows across the 128-row tile boundary
    assert np.all(np.isfinite(P_end)) and np.all(np.diag(P_end)[3 + 2 * NF0:] > 0)
