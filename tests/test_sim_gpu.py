"""Device-side observation generator and known-association table against the oracle's restatement
of Slam::getObservations (slam.h:575-683, 339-368) and EKF::dataAssociateTable (EKF.cpp:146-233)."""
import numpy as np
import pytest

from pyoracle import Oracle, TEXTBOOK

pytestmark = pytest.mark.gpu


def _random_map(N, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.uniform(-400.0, 400.0, size=(2, N)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [0, 1, 35, 1500, 5000])
def test_get_observations_matches_the_oracle(gpu_required, dtype, N):
    from conan_slam_amd import Simulator

    LM = _random_map(N, 3 + N).astype(dtype)
    o = Oracle(dtype)
    sim = Simulator(LM, dtype=dtype)
    rng = np.random.default_rng(N)
    for trial in range(4):
        xv = np.array([rng.uniform(-300, 300), rng.uniform(-300, 300), rng.uniform(-3.1, 3.1)], dtype=dtype)
        rmax = [30.0, 120.0, 400.0, 2000.0][trial]
        Z, tags = sim.get_observations(xv, rmax)
        Zo, tags_o = o.get_observations(xv, LM, rmax)
        assert np.array_equal(tags, tags_o), (N, trial)          # integer output: exact, ascending tag order
        assert Z.shape == Zo.shape
        tol = 2e-6 if dtype == np.float32 else 1e-13
        assert np.all(np.abs(Z.astype(np.float64) - Zo.astype(np.float64)) <= tol * np.maximum(1.0, np.abs(Zo)))
    sim.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_table_association_and_noise_follow_the_reference_over_a_run(gpu_required, dtype):
    """A drive through a 300-landmark map: every scan is split by the device table exactly as the oracle's sequential
    loop does it (ZF/idf/ZN and the table itself), noise included, and the known part feeds the engine from HBM."""
    from conan_slam_amd import EKF, Simulator
    from conan_slam_amd.synth import normal

    N = 300
    LM = _random_map(N, 11).astype(dtype)
    o = Oracle(dtype)
    sim = Simulator(LM, dtype=dtype)
    table = np.zeros(N, dtype=np.int32)
    R = np.diag([0.08, 0.0024]).astype(dtype)
    nf = 0
    xv = np.array([0.0, 0.0, 0.3], dtype=dtype)
    for step in range(25):
        xv = (xv + np.array([9.0 * np.cos(xv[2]), 9.0 * np.sin(xv[2]), 0.11], dtype=np.float64)).astype(dtype)
        Z, tags = sim.get_observations(xv, 150.0)
        Zo, tags_o = o.get_observations(xv, LM, 150.0)
        assert np.array_equal(tags, tags_o)
        m = len(tags)
        nz = np.array([normal(77, 1000 * step + j) for j in range(2 * max(m, 1))], dtype=dtype)
        sim.add_observation_noise(R, nz)
        Zn = Zo.copy()
        for c in range(m):  # slam.h:168-178
            Zn[0, c] = dtype(Zn[0, c] + dtype(nz[2 * c]) * dtype(np.sqrt(R[0, 0])))
            Zn[1, c] = dtype(Zn[1, c] + dtype(nz[2 * c + 1]) * dtype(np.sqrt(R[1, 1])))
        ZF, ZN, idf = sim.data_associate_table(nf)
        ZFo, ZNo, idfo = o.data_associate_table(Zn, tags_o, table, nf)
        assert np.array_equal(idf, idfo) and ZF.shape == ZFo.shape and ZN.shape == ZNo.shape
        tol = 4e-6 if dtype == np.float32 else 1e-12
        for A, B in ((ZF, ZFo), (ZN, ZNo)):
            assert np.all(np.abs(A.astype(np.float64) - B.astype(np.float64)) <= tol * np.maximum(1.0, np.abs(B)))
        assert np.array_equal(sim.table, table)
        nf += ZN.shape[1]
    assert nf > 20 and (table > 0).sum() == nf
    sim.close()


def test_device_resident_scan_feeds_the_engine(gpu_required):
    """ZF / idf of the device-side split go into cslam_ekf_update_device without touching the host: same state as the
    host-pointer entry."""
    from conan_slam_amd import EKF, Simulator
    from helpers import make_scenario

    N = 60
    X, P = make_scenario(N, np.float32, seed=21, corr=0.2)
    LM = np.asfortranarray(X[3:].reshape(2, N, order="F").astype(np.float32))  # the map is where the filter thinks it is
    sim = Simulator(LM)
    sim.table = np.arange(1, N + 1, dtype=np.int32)                              # every landmark already known
    Z, tags = sim.get_observations(X[:3].astype(np.float32), 1e6)
    ZF, ZN, idf = sim.data_associate_table(N)
    assert ZN.shape[1] == 0 and len(idf) == len(tags) > 0
    R = np.diag([0.08, 0.0024]).astype(np.float32)
    a = EKF(N, dtype=np.float32, quirks=TEXTBOOK)
    b = EKF(N, dtype=np.float32, quirks=TEXTBOOK)
    for e in (a, b):
        e.set_state(X, P)
    a.update(ZF, R, idf, batch=True)
    p = sim.device_ptrs()
    b.update_device(p["ZF"], len(idf), R, p["idf"], batch=True)
    Xa, Pa = a.get_state()
    Xb, Pb = b.get_state()
    assert np.array_equal(Xa, Xb) and np.array_equal(Pa, Pb)
    a.close()
    b.close()
    sim.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [1023, 1024, 1025, 2049])
def test_table_association_beyond_one_pass_of_the_workgroup(gpu_required, dtype, N):
    """sim_associate_table_body walks the scan in passes of 1024 threads with two workgroup-wide scans per pass.  Every
    landmark is in front of the pose and inside rmax, so scan position i holds tag i + 1; the preset table makes known
    and new tags alternate in runs of 7 of which one covers positions 1018 .. 1024 and one starts at 2047 (the counts
    carried from pass to pass change inside a run), with a shuffled state position for every known tag.  ZF, ZN, idf and
    the table are copies and integers: bit for bit the oracle's sequential loop.  Then a second scan from another pose,
    on the table the first one left."""
    from conan_slam_amd import Simulator

    rng = np.random.default_rng(N)
    LM = np.asfortranarray(np.stack([rng.uniform(10.0, 300.0, size=N), rng.uniform(-200.0, 200.0, size=N)]).astype(dtype))
    run = ((np.arange(2049) + 4) // 7) % 2 == 0              # the pattern at its full length, whatever N cuts off
    assert len(set(run[1018:1025])) == 1 and run[1017] != run[1018] and run[2046] != run[2047] == run[2048]
    known = run[:N]
    table = np.zeros(N, dtype=np.int32)
    nf = int(known.sum())
    table[known] = rng.permutation(nf) + 1
    o = Oracle(dtype)
    sim = Simulator(LM, dtype=dtype)
    sim.table = table
    for xv in ([0.0, 0.0, 0.0], [-5.0, 3.0, 0.05]):
        xv = np.array(xv, dtype=dtype)
        Z, tags = sim.get_observations(xv, 1000.0)
        assert np.array_equal(tags, np.arange(1, N + 1))
        ZF, ZN, idf = sim.data_associate_table(nf)
        ZFo, ZNo, idfo = o.data_associate_table(Z, tags, table, nf)     # (advances `table` in place)
        assert np.array_equal(idf, idfo), (N, np.nonzero(idf != idfo)[0][:5] if idf.shape == idfo.shape else (idf.shape, idfo.shape))
        assert ZF.shape == ZFo.shape and ZN.shape == ZNo.shape
        assert np.array_equal(ZF, ZFo) and np.array_equal(ZN, ZNo)
        assert np.array_equal(sim.table, table)
        nf += ZN.shape[1]
    assert nf == N and ZN.shape[1] == 0 and np.array_equal(np.sort(table), np.arange(1, N + 1))
    sim.close()
