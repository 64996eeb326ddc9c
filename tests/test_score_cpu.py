"""CPU checks of the score of a Monte-Carlo study (cslam_ekf_batch_score_*): the numpy restatement the GPU tests compare
with (tests/score_ref.py) against hand-worked cases, and the surface -- header, exports, bindings, EKFBatch methods."""
import ctypes
import os
import re

import numpy as np

import score_ref as sr
from conan_slam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cslam_ekf_batch_score_reset", "cslam_ekf_batch_score_set_truth", "cslam_ekf_batch_score",
                "cslam_ekf_batch_score_scan", "cslam_ekf_batch_get_scores")


def _one(x, A, xl, pll, truth, xt, **kw):
    return sr.score_call(np.array([x], np.float32), np.array([A], np.float32), np.array([xl], np.float32).reshape(1, -1, 2),
                         np.array([pll], np.float32).reshape(1, -1, 2, 2), truth, xt, **kw)


def test_unit_pose_block():
    """Pvv = I, e = (1, 0, 0): NEES 1, err^2 1, heading error 0, inside the gate."""
    T, B, rec, rb = _one([1, 0, 0], np.eye(3), [], [], np.zeros((0, 2)), [0, 0, 0])
    assert T[0, sr.POSE_N] == 1 and T[0, sr.POSE_BAD] == 0 and T[0, sr.POSE_IN] == 1
    assert T[0, sr.POSE_NEES] == 1.0 and T[0, sr.POSE_ERR2] == 1.0 and T[0, sr.POSE_EPHI2] == 0.0
    assert rec[0, 0] == 1.0 and rec[0, 1] == 1.0
    assert 0 < B[0, sr.POSE_NEES] < 1e-13


def test_pose_nees_against_a_solve():
    rng = np.random.default_rng(0)
    M = rng.normal(size=(3, 3))
    A = (M @ M.T + 0.1 * np.eye(3)).astype(np.float32)
    x, xt = np.array([3.0, -1.0, 0.4], np.float32), np.array([2.5, -1.2, 0.1], np.float32)
    T, B, _, _ = _one(x, A, [], [], np.zeros((0, 2)), xt)
    e = x.astype(np.float64) - xt
    want = e @ np.linalg.solve(A.astype(np.float64), e)
    assert abs(T[0, sr.POSE_NEES] - want) <= 1e-12 * want
    # gate: outside a tiny gate, inside the default one
    T2, _, _, _ = _one(x, A, [], [], np.zeros((0, 2)), xt, gate_pose=1e-9)
    assert T2[0, sr.POSE_IN] == 0 and T[0, sr.POSE_IN] == float(want <= sr.GATE_POSE)


def test_heading_error_wraps_across_pi():
    """True phi = pi - 0.01, estimate -pi + 0.01: the error is 0.02, not 2 pi - 0.02."""
    xt = np.array([0, 0, np.pi - 0.01], np.float32)
    x = np.array([0, 0, -np.pi + 0.01], np.float32)
    T, _, _, _ = _one(x, np.eye(3), [], [], np.zeros((0, 2)), xt)
    assert abs(np.sqrt(T[0, sr.POSE_EPHI2]) - 0.02) < 1e-6
    assert sr.wrap(np.pi) == np.pi and sr.wrap(-np.pi) == np.pi and abs(sr.wrap(7.0) - (7.0 - 2 * np.pi)) < 1e-15
    assert abs(sr.wrap(-np.pi + 1e-9) - (-np.pi + 1e-9)) < 1e-15


def test_bad_pose_blocks():
    for A in (np.zeros((3, 3)), np.diag([1.0, -1.0, 1.0]), np.diag([1.0, np.nan, 1.0])):
        T, _, rec, _ = _one([1, 2, 3], A, [], [], np.zeros((0, 2)), [0, 0, 0])
        assert T[0, sr.POSE_BAD] == 1 and T[0, sr.POSE_N] == 0 and np.all(T[0, [sr.POSE_ERR2, sr.POSE_NEES]] == 0)
        assert np.isnan(rec[0, 0]) and np.isnan(rec[0, 1]) and np.all(np.isfinite(T))
    T, _, _, _ = _one([np.inf, 2, 3], np.eye(3), [], [], np.zeros((0, 2)), [0, 0, 0])
    assert T[0, sr.POSE_BAD] == 1


def test_landmark_closed_form_and_bad_blocks():
    xl = [[1.0, 2.0], [5.0, 5.0], [0.0, 0.0], [1.0, 1.0]]
    pll = [np.diag([4.0, 1.0]), [[1.0, 2.0], [2.0, 1.0]], [[0.0, 0.0], [0.0, 1.0]], [[2.0, 0.5], [0.5, 1.0]]]
    truth = np.array([[0.0, 0.0], [4.0, 4.0], [1.0, 1.0], [0.0, 3.0]])
    T, B, rec, _ = _one([0, 0, 0], np.eye(3), xl, pll, truth, [0, 0, 0])
    # feature 1: 1/4 + 4 = 4.25; feature 2: det = -3 -> BAD; feature 3: p00 = 0 -> BAD; feature 4: e = (1, -2)
    e = np.array([1.0, -2.0])
    q4 = e @ np.linalg.solve(np.array(pll[3]), e)
    assert T[0, sr.LM_N] == 2 and T[0, sr.LM_BAD] == 2
    assert abs(T[0, sr.LM_NEES] - (4.25 + q4)) < 1e-13 and T[0, sr.LM_ERR2] == 5.0 + 5.0
    assert T[0, sr.LM_IN] == float(4.25 <= sr.GATE_LM) + float(q4 <= sr.GATE_LM)
    assert abs(rec[0, 3] - (4.25 + q4) / 2) < 1e-13 and rec[0, 2] == 5.0
    # features beyond the truth rows are not scored; a NaN truth row is a bad block
    T, _, _, _ = _one([0, 0, 0], np.eye(3), xl, pll, truth[:1], [0, 0, 0])
    assert T[0, sr.LM_N] == 1 and T[0, sr.LM_BAD] == 0
    tn = truth.copy()
    tn[0, 1] = np.nan
    T, _, _, _ = _one([0, 0, 0], np.eye(3), xl, pll, tn, [0, 0, 0])
    assert T[0, sr.LM_N] == 1 and T[0, sr.LM_BAD] == 3 and np.all(np.isfinite(T))


def test_empty_map_gives_nan_means():
    T, _, rec, _ = _one([1, 0, 0], np.eye(3), [], [], np.zeros((0, 2)), [0, 0, 0])
    assert T[0, sr.LM_N] == 0 and T[0, sr.LM_BAD] == 0
    assert np.isnan(rec[0, 2]) and np.isnan(rec[0, 3]) and not np.isnan(rec[0, 0])


def test_accumulator_rejects_a_relative_error_of_1e_6():
    rng = np.random.default_rng(3)
    acc = sr.Accumulator(2, series_capacity=1)
    x = rng.normal(size=(2, 3)).astype(np.float32)
    A = np.stack([np.eye(3, dtype=np.float32) * (1 + i) for i in range(2)])
    xl = rng.normal(size=(2, 7, 2)).astype(np.float32)
    pll = np.stack([[np.diag([1.0 + j, 2.0]) for j in range(7)]] * 2).astype(np.float32)
    acc.add(x, A, xl, pll, np.zeros((7, 2)), np.zeros(3))
    acc.add(x, A, xl, pll, np.zeros((7, 2)), np.zeros(3))
    series = np.stack(acc.series).astype(np.float32)
    acc.check(acc.T.copy(), series, 2)
    for f in (sr.POSE_ERR2, sr.POSE_NEES, sr.LM_ERR2, sr.LM_NEES):
        bad = acc.T.copy()
        bad[:, f] *= 1 + 1e-6
        try:
            acc.check(bad, series, 2)
        except AssertionError:
            continue
        raise AssertionError(f"the bound accepts a relative error of 1e-6 in {sr.FIELDS[f]}")


def test_header_declares_the_score():
    names = _capi.declared_symbols()
    for s in ENTRY_POINTS:
        assert s in names, s
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    m = re.search(r"enum\s*\{([^}]*CSLAM_SCORE_FIELDS[^}]*)\}", text)
    assert m, "the enum of the totals' fields"
    fields = re.findall(r"CSLAM_SCORE_[A-Z0-9_]+", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["CSLAM_SCORE_" + f for f in sr.FIELDS] + ["CSLAM_SCORE_FIELDS"]
    assert _capi.SCORE_FIELD_NAMES == sr.FIELDS and _capi.SCORE_FIELDS == len(sr.FIELDS)
    for cite in ("test/main.cpp:136", "EKF.cpp:131-144"):
        assert cite in text, cite


def test_library_exports_the_score_and_the_binding_has_it():
    assert os.path.exists(_capi.LIB_PATH), "build the engine first: python -m conan_slam_amd.build"
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for s in ENTRY_POINTS:
        assert hasattr(lib, s), s
        assert s in _capi._PROTOTYPES, s
    from conan_slam_amd import EKFBatch

    for m in ("score_reset", "score_set_truth", "score", "score_scan", "scores"):
        assert callable(getattr(EKFBatch, m, None)), m
