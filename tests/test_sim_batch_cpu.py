"""CPU side of the batched scan generator: the C ABI declares its eight entry points, and synth.control_noise is the
harness's control noise (oracle/sim_driver.run_demo, slam.h:149-159) bit for bit."""
import numpy as np

from conan_slam_amd import _capi

SIM_BATCH = ("cslam_sim_batch_create", "cslam_sim_batch_destroy", "cslam_sim_batch_scan", "cslam_sim_batch_get_scan",
             "cslam_sim_batch_get_table", "cslam_sim_batch_set_table", "cslam_ekf_batch_update_scan",
             "cslam_ekf_batch_augment_scan")


def test_header_declares_the_batched_generator():
    import ctypes

    names = _capi.declared_symbols()
    for need in SIM_BATCH:
        assert need in names, need
    assert set(SIM_BATCH) == set(_capi.SIM_BATCH_SYMBOLS)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert not [s for s in SIM_BATCH if not hasattr(lib, s)]
    lib.cslam_version.restype = ctypes.c_int
    assert lib.cslam_version() == 100


def test_python_surface():
    import conan_slam_amd

    assert hasattr(conan_slam_amd, "BatchSimulator") and "BatchSimulator" in conan_slam_amd.__all__
    assert hasattr(conan_slam_amd.EKFBatch, "update_scan") and hasattr(conan_slam_amd.EKFBatch, "augment_scan")


class _Controls:
    """run_demo back-end without a filter: keeps the (vn, swan) of every predict."""

    def __init__(self):
        self.vn, self.swan, self.nf = [], [], 0

    @property
    def n(self):
        return 3 + 2 * self.nf

    def predict(self, v, swa, Q, wb, dt):
        self.vn.append(np.float32(v))
        self.swan.append(np.float32(swa))

    def observe_heading(self, *a):
        pass

    def update(self, *a):
        return 0

    def augment(self, Z, R):
        self.nf += Z.shape[1] if Z.size else 0

    def get_x(self):
        return np.zeros(self.n, np.float32)

    def get_p(self):
        return np.zeros((self.n, self.n), np.float32)


def test_control_noise_is_the_harness_control_noise():
    """Seeds 1000..1003, the first 2 400 control steps of the demo: one vectorised call and step by step, bitwise."""
    from sim_driver import SlamConfig, load_demo_map, run_demo

    from conan_slam_amd.synth import control_noise, noise_matrices

    STEPS, seeds = 2400, [1000, 1001, 1002, 1003]
    LM, WP = load_demo_map()
    rec = []
    for s in seeds:
        c = _Controls()
        run_demo(c, LM, WP, noise_seed=s, max_steps=STEPS)
        assert len(c.vn) == STEPS
        rec.append(c)
    # the noise-free controls: the commanded speed, and the steering angle of a run without noise
    c0 = _Controls()
    run_demo(c0, LM, WP, noise_seed=None, max_steps=STEPS)
    swa = np.array(c0.swan, dtype=np.float32)
    v = SlamConfig().velocity
    assert all(x == v for x in c0.vn)
    Q = noise_matrices(np.float32)[0]
    want_v = np.array([r.vn for r in rec], dtype=np.float32).T
    want_s = np.array([r.swan for r in rec], dtype=np.float32).T
    steps = np.arange(1, STEPS + 1)
    vn, swan = control_noise(seeds, steps, v, swa, Q)
    assert vn.dtype == np.float32 and swan.dtype == np.float32 and vn.shape == (STEPS, 4)
    assert np.array_equal(vn.view(np.uint32), want_v.view(np.uint32))
    assert np.array_equal(swan.view(np.uint32), want_s.view(np.uint32))
    assert np.any(vn[:, 0] != vn[:, 1])
    for t in range(STEPS):
        a, b = control_noise(seeds, t + 1, v, swa[t], Q)
        assert a.shape == (4,) and b.shape == (4,)
        assert np.array_equal(a.view(np.uint32), want_v[t].view(np.uint32)), t
        assert np.array_equal(b.view(np.uint32), want_s[t].view(np.uint32)), t
