"""The tail phase of the f32 P-GEMM ekf_downdate_psym4_f32 (CSLAM_PGEMM_TAIL; csrc/ekf_pgemm_tiles.hpp): the tiles at the
end of the work list are handed out as 32-row strips, and strips wholly beyond row n are dropped.

A strip element is the same MFMA on the same operand pairs in the same order as in a whole tile, so get_state() must be
BITWISE equal whatever the switch says: 0 (no strips), 1 (one tile), a number beyond the tile count (every tile but the
first, which the engine keeps whole: a workgroup enters the tail phase from the whole-tile loop), unset (the rule).
pgemm_split() reports the whole tiles and strips of the last launch, which shows that the strip path ran.
With all those tiles split P_map is also checked element by element against P0 - W1 W1^T in f64 (immediate updates, whose
panel debug_last_update returns; bound: that of test_kernel_edges_gpu.py::_pgemm_case).

Grids (set_pgemm_workgroups): 0 -- one workgroup per tile, every list index is a static one; 1 -- one workgroup draws
every tile and strip by ticket; 3 -- several workgroups contend for the strips.  One handle is alive at a time.
"""
import numpy as np
import pytest

from helpers import make_obs, make_scenario
from pyoracle import TEXTBOOK

pytestmark = pytest.mark.gpu

R22 = np.diag([0.08, 0.0024])
ALL = "100000"  # more than any tile count here: every tile but the first is split
U32 = float(np.finfo(np.float32).eps) / 2


def _tiles(N):
    rows = (3 + 2 * N + 127) // 128
    return rows, rows * (rows + 1) // 2


def _valid(N):
    rows, _ = _tiles(N)
    return (3 + 2 * N - (rows - 1) * 128 + 31) // 32


def _expected_split(N, G, tail):
    """(whole tiles, strips) by the rules of ekf_pgemm_tiles.hpp"""
    rows, T = _tiles(N)
    valid = _valid(N)
    last_row = rows if valid < 4 else 0
    if tail is None:
        S = 0 if T <= 2 * G else last_row
    else:
        S = min(int(tail), T - 1)  # (the engine keeps one tile whole)
    in_last = min(S, last_row)
    strips = in_last * valid + (S - in_last) * 4
    return (T - S, strips) if strips else (T, 0)


def _landmarks(N, m, seed):
    """m distinct landmarks, the last one and the tile-straddling ones (f = 63 mod 64) among them"""
    rng = np.random.default_rng(seed)
    special = list(dict.fromkeys([f for f in range(63, N + 1, 64)] + [N]))[:m]
    rest = [f for f in rng.permutation(N) + 1 if f not in special]
    return np.array(special + rest[: m - len(special)], dtype=np.int32)


def _run(monkeypatch, N, k, grid, tail, extra_env=None):
    """one (shape, panel width, grid) under one value of the switch: state, split, W1 of an immediate update"""
    from conan_slam_amd import EKF

    if tail is None:
        monkeypatch.delenv("CSLAM_PGEMM_TAIL", raising=False)
    else:
        monkeypatch.setenv("CSLAM_PGEMM_TAIL", tail)
    for key, val in (extra_env or {}).items():
        monkeypatch.setenv(key, val)
    X, P = make_scenario(N, np.float32, seed=900 + N + k, corr=0.1, pose_scale=1e-4)
    e = EKF(N, dtype=np.float32, quirks=TEXTBOOK)
    try:
        e.set_pgemm_workgroups(grid)
        e.set_state(X, P)
        W1 = None
        if k == 128:
            e.set_deferred(128)
            for t in range(2):
                idf = _landmarks(N, 32, seed=10 * N + t)
                e.update(make_obs(X, idf, np.float32, seed=t), R22.astype(np.float32), idf, batch=True)
            e.flush()
        else:
            idf = _landmarks(N, k // 2, seed=10 * N + k)
            e.update(make_obs(X, idf, np.float32, seed=k), R22.astype(np.float32), idf, batch=True)
            W1 = e.debug_last_update()["W1"].astype(np.float64)[3:, :]
        Xg, Pg = e.get_state()
        split = e.pgemm_split()
        assert e.factor_status() == 0
    finally:
        e.close()
    return Xg, Pg, split, W1, P


@pytest.mark.parametrize("grid", [0, 1, 3])
@pytest.mark.parametrize("k", [64, 66, 128])
@pytest.mark.parametrize("N", [63, 127, 600])
def test_state_is_bitwise_the_same_for_every_value_of_the_switch(gpu_required, monkeypatch, N, k, grid):
    _, T = _tiles(N)
    G = T if grid == 0 else grid
    ref = None
    for tail in ("0", "1", ALL, None):
        Xg, Pg, split, W1, P0 = _run(monkeypatch, N, k, grid, tail)
        assert split == _expected_split(N, G, tail), (tail, split)
        if ref is None:
            ref = (Xg, Pg)
            assert split[1] == 0
        else:
            assert np.array_equal(Xg, ref[0]), f"X differs with CSLAM_PGEMM_TAIL={tail}"
            assert np.array_equal(Pg, ref[1]), f"P differs with CSLAM_PGEMM_TAIL={tail}"
        if tail == ALL:
            assert split[0] == 1 and split[1] > 0
            if W1 is not None:
                # element by element against f64 from the same panel: the subtraction rounds at the size of its
                # operands, the dot product of length k at (k + 1) u of sum |w_ik w_jk|
                Pm = P0[3:, 3:].astype(np.float64)
                expected = Pm - W1 @ W1.T
                bound = U32 * (np.abs(Pm) + np.abs(expected)) + (k + 1) * U32 * (np.abs(W1) @ np.abs(W1).T) + 1e-300
                err = np.abs(Pg[3:, 3:].astype(np.float64) - expected)
                worst = float((err / bound).max())
                print(f"N={N} k={k} grid={grid}: error / bound = {worst:.3g}")
                assert worst <= 1.0, f"error / bound = {worst:.3g}"


def test_per_xcd_queues_take_no_strips(gpu_required, monkeypatch):
    """CSLAM_XCD_QUEUES=1 (66 tiles: the grid is large enough for the eight queues): today's behaviour, no strips"""
    N = 640
    a = _run(monkeypatch, N, 64, 0, "0", {"CSLAM_XCD_QUEUES": "1"})
    b = _run(monkeypatch, N, 64, 0, ALL, {"CSLAM_XCD_QUEUES": "1"})
    assert b[2] == (_tiles(N)[1], 0) and a[2] == b[2]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_lookahead_windows_with_the_tail_forced(gpu_required, monkeypatch):
    """N = 70, eight m = 32 updates in look-ahead windows: the tail forced on all tiles against the switch at 0"""
    from conan_slam_amd import EKF

    N = 70
    X0, P0 = make_scenario(N, np.float32, seed=77, corr=0.1, pose_scale=1e-4)
    Q = np.diag([0.18, 6e-4]).astype(np.float32)
    R = R22.astype(np.float32)
    plan = [_landmarks(N, 32, seed=50 + t) for t in range(8)]
    obs = [make_obs(X0, idf, np.float32, seed=t) for t, idf in enumerate(plan)]
    out = {}
    monkeypatch.setenv("CSLAM_LOOKAHEAD", "1")
    for tail in ("0", ALL):
        monkeypatch.setenv("CSLAM_PGEMM_TAIL", tail)
        e = EKF(N, dtype=np.float32, quirks=TEXTBOOK, sync_mode=False)
        try:
            e.set_state(X0, P0)
            e.set_deferred(128)
            for t, idf in enumerate(plan):
                e.predict(83.33, 0.01 * (t % 5), Q, 73.0, 0.01)
                e.update(obs[t], R, idf, True)
            out[tail] = e.get_state()
            assert e.factor_status() == 0
            assert e.lookahead_windows() > 0
            split = e.pgemm_split()
            assert (split[1] > 0) == (tail == ALL), split
        finally:
            e.close()
    assert np.array_equal(out["0"][0], out[ALL][0]) and np.array_equal(out["0"][1], out[ALL][1])


def test_batched_engine_with_the_tail_forced(gpu_required, monkeypatch):
    """2 instances x N = 600, two windows of two m = 32 updates: the tail forced on all tiles against off, bitwise per instance"""
    import torch

    from conan_slam_amd import EKFBatch
    from conan_slam_amd.synth import Workload

    N, m, steps = 600, 32, 4
    loads = [Workload(N, m, np.float32, seed=700 + r) for r in range(2)]
    ctrl = [Workload(N, m, np.float32, seed=0, build_p=False).controls(t) for t in range(steps)]
    inputs = []
    for w in loads:
        Zh = np.zeros((steps, 2 * m), dtype=np.float32)
        Ih = np.zeros((steps, m), dtype=np.int32)
        for t in range(steps):
            w.controls(t)
            Z, idf = w.observations(t)
            Zh[t] = Z.reshape(-1, order="F")
            Ih[t] = idf
        inputs.append((torch.from_numpy(Zh).cuda(), torch.from_numpy(Ih).cuda()))
    torch.cuda.synchronize()
    w0 = loads[0]
    out = {}
    for tail in ("0", ALL):
        monkeypatch.setenv("CSLAM_PGEMM_TAIL", tail)
        b = EKFBatch(2, N, quirks=TEXTBOOK)
        try:
            for i, w in enumerate(loads):
                b.set_state(i, w.X0, w.P0)
            b.run(steps, np.array([c[0] for c in ctrl], dtype=np.float64), np.array([c[1] for c in ctrl], dtype=np.float64),
                  w0.QE, w0.wb, w0.dt, [inp[0].data_ptr() for inp in inputs], [inp[1].data_ptr() for inp in inputs], m, w0.RE)
            out[tail] = [b.get_state(i) for i in range(2)]
            assert all(f == 0 for f in b.factor_status())
            assert b.windows() == 2
            split = b.pgemm_split()
            _, T = _tiles(N)
            assert split == ((2 * T, 0) if tail == "0" else (2, 2 * _expected_split(N, 1, ALL)[1])), split
        finally:
            b.close()
    for i in range(2):
        assert np.array_equal(out["0"][i][0], out[ALL][i][0]), f"X of instance {i}"
        assert np.array_equal(out["0"][i][1], out[ALL][i][1]), f"P of instance {i}"
