"""The particle filter's device-side score without a GPU: the C ABI declares it and cites the reference, and the inputs
of the "values" cases of tests/test_pf_score_gpu.py are well chosen -- no bad block, and every NEES further from its gate
than its own rounding bound, so that the exact count comparison on the device cannot flip on rounding."""
import os
import re

import numpy as np
import pytest

import score_ref
from pf_builders import DTYPES, random_particles
from pf_estimate_ref import Moments, estimate_ref, stack
from pf_score_ref import (PfScoreRef, VALUES_NF, VALUES_NP, call, reads, reference_estimate, truth_count, values_case)
from score_ref import GATE_LM, GATE_POSE, LM_BAD, LM_IN, LM_N, POSE_BAD, POSE_IN, POSE_N

from conan_slam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cslam_pf_score_reset", "cslam_pf_score_set_truth", "cslam_pf_score", "cslam_pf_score_sharded",
       "cslam_pf_get_scores")


def test_header_declares_the_score_calls_and_cites_the_reference():
    names = _capi.declared_symbols()
    assert set(NEW) <= set(names) and tuple(_capi.PF_SCORE_SYMBOLS) == NEW
    text = open(os.path.join(ROOT, "include", "cslam.h")).read()
    for name in NEW:
        at = text.index("int " + name + "(")
        comment = text[text.rindex("/*", 0, at):at]
        assert "test/main.cpp:330" in comment and "slam.h:493-511" in comment, name
        assert re.search(r"\*/\s*$", comment), (name, "the comment must end right above the declaration")
    assert "slam.h:513-539" in text[text.index("cslam_pf_score_reset"):text.index("cslam_pf_get_scores")]
    assert "#define CSLAM_PF_SCORE_MEAN 0" in text and "#define CSLAM_PF_SCORE_BEST 1" in text
    assert "the particle filter have no scorer" not in text
    for name in NEW:
        assert name in _capi._PROTOTYPES, name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("estimator", ["mean", "best"])
@pytest.mark.parametrize("nf", VALUES_NF)
@pytest.mark.parametrize("npart", VALUES_NP)
def test_values_cases_are_well_chosen(npart, nf, estimator, dtype):
    case = values_case(npart, nf, dtype, estimator)
    c = truth_count(nf)
    assert case.truth.shape == (c, 2) and len(case.xv_trues) == 3
    inside = []
    for xv_true in case.xv_trues:
        T, B, rec, rb = call(case.ref, dtype, case.truth, xv_true)
        assert T[POSE_BAD] == 0 and T[LM_BAD] == 0 and T[POSE_N] == 1 and T[LM_N] == c, T
        # every NEES against its gate, with its own bound
        x, pvv, xl, pll = reads(case.ref, dtype)
        ok, e, q, b = score_ref.pose_score(x[0], pvv[0], xv_true)
        assert ok and abs(q - GATE_POSE) > b[2], (q, b)
        inside.append(q <= GATE_POSE)
        lok, _, lq, _, bq = score_ref.landmark_scores(xl[0, :c], pll[0, :c], case.truth)
        assert lok.all() and np.all(np.abs(lq - GATE_LM) > bq), (npart, nf, float(np.min(np.abs(lq - GATE_LM) - bq)))
        if c >= 5:
            assert 0 < T[LM_IN] < c, "the landmark gate must split the features"
    assert inside == [True, True, False], inside


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_weights_zero_is_one_bad_pose_and_c_bad_landmarks(dtype):
    """A degenerate weight sum makes every moment NaN: the wrapper counts POSE_BAD = 1 and LM_BAD = c, nothing else."""
    nf, c = 5, 3
    parts = random_particles(9, nf, dtype, seed=3)
    ref = estimate_ref(*stack(parts))
    # what cslam_pf_estimate returns for W = 0: W as computed, Neff and every moment NaN
    est = Moments(0.0, np.nan, *(np.full_like(a, np.nan) for a in ref[2:]))
    ref = PfScoreRef(dtype, "mean", series_capacity=2)
    ref.add(est, np.zeros((c, 2)), np.zeros(3))
    want = np.zeros(len(score_ref.FIELDS))
    want[POSE_BAD], want[LM_BAD] = 1, c
    assert np.array_equal(ref.totals, want), ref.totals
    assert np.isnan(ref.acc.series[0]).all() and np.isnan(ref.expected_track()[0, [0, 1, 2, 4]]).all()
    assert ref.expected_track()[0, 3] == 0.0


def test_wrapper_adds_no_arithmetic():
    """The wrapper's single call IS score_ref.score_call on the reshaped estimate, and without the map it scores none."""
    dtype = np.float32
    case = values_case(65, 1, dtype, "best")
    T, B, rec, rb = call(case.ref, dtype, case.truth, case.xv_trues[0])
    T2, B2, rec2, rb2 = score_ref.score_call(*reads(case.ref, dtype), case.truth, case.xv_trues[0])
    assert np.array_equal(T, T2[0]) and np.array_equal(B, B2[0]) and np.array_equal(rec, rec2[0], equal_nan=True)
    T3, _, rec3, _ = call(case.ref, dtype, case.truth, case.xv_trues[0], with_map=False)
    assert T3[LM_N] == 0 and T3[LM_BAD] == 0 and T3[POSE_N] == 1 and np.isnan(rec3[2:]).all()
    assert reference_estimate(case.parts, dtype, "best").index == case.ref.index
