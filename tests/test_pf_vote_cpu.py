"""CPU side of the vote on new features kept on the device: PfVoteMemo as a stand-alone program (plain and under the
address and undefined-behaviour sanitizers), the numpy restatement of the vote kernel (tests/pf_vote_ref.py) against
pf.new_feature_votes, the edge rows of the rule, and the new entry points declared, cited, bound, exported and mirrored."""
import ctypes
import os

import numpy as np
import pytest

import pf_vote_ref as V
from test_host_parts_cpu import build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEED = ("cslam_pf_associate_vote", "cslam_pf_associate_vote_sharded", "cslam_pf_vote_wait", "cslam_pf_get_vote",
        "cslam_pf_sample_proposal_voted", "cslam_pf_sample_proposal_voted_drawn", "cslam_pf_feature_update_voted",
        "cslam_pf_add_features_voted", "cslam_pf_assoc_scan_step_drawn")


def test_vote_memo_check_builds_and_passes(tmp_path):
    build_and_run("pf_vote_memo_check", tmp_path)


@pytest.mark.parametrize("fraction", V.FRACTIONS)
def test_the_restatement_is_the_host_policy(fraction):
    """Random summaries, m up to 600 (tile edges 255 / 256 / 257 among them): rule, ordered compaction and counts of the
    restatement against what pf.data_associate derives from pf.new_feature_votes, bit for bit, in f32 and f64."""
    rng = np.random.default_rng(int(fraction * 10) + 7)
    for m in (0, 1, 8, 9, 33, 64, 65, 255, 256, 257, 511, 513, 600):
        for dtype in (np.float32, np.float64):
            s = V.random_summaries(rng, m)
            Z = np.asfortranarray(rng.normal(size=(2, m)).astype(dtype))
            got, want = V.vote(s, Z, fraction), V.host_policy(s, Z, fraction)
            assert V.same(got, want), (m, fraction, np.dtype(dtype).name)
            assert got.count == (got.q, m) and got.q == int((got.use == 0).sum())
            assert np.all(np.diff(got.new_idx) > 0)  # observation order


def test_the_three_term_sum_is_sequential():
    """numpy's row sum of three terms adds them in order: (s0 + s1) + s2, which is what the kernel is written to do."""
    from conan_slam_amd.pf import new_feature_votes

    rng = np.random.default_rng(3)
    s = np.zeros((20000, 4))
    s[:, :3] = rng.random((20000, 3)) * 10.0 ** rng.integers(-8, 8, (20000, 3))
    seq = (s[:, 0] + s[:, 1]) + s[:, 2]
    assert np.array_equal(s[:, :3].sum(axis=1), seq)
    assert np.any(seq != s[:, 0] + (s[:, 1] + s[:, 2]))  # (the order matters on these rows)
    for f in V.FRACTIONS:
        assert np.array_equal(V.is_new(s, f), new_feature_votes(s, f))


def test_edge_rows():
    from conan_slam_amd.pf import new_feature_votes

    for row, answers in V.EDGE_ROWS:
        s = np.array([list(row) + [0.0]])
        for f, want in answers.items():
            assert bool(new_feature_votes(s, f)[0]) is want, (row, f)
            assert bool(V.is_new(s, f)[0]) is want, (row, f)
    # a NaN takes part in no comparison
    assert not V.is_new(np.array([[np.nan, 1.0, 0.0, 0.0], [0.5, np.nan, 0.0, 0.0]]), 0.5).any()
    # all rows at once through the compaction: observation order, untouched tail
    rows = np.array([list(r) + [0.0] for r, _ in V.EDGE_ROWS])
    Z = np.asfortranarray(np.arange(10, dtype=np.float32).reshape(2, 5, order="F"))
    got = V.vote(rows, Z, 0.5)
    assert got.use.tolist() == [0, 1, 1, 1, 0] and got.new_idx.tolist() == [0, 4] and got.q == 2
    assert np.array_equal(got.ZN, Z[:, [0, 4]])


def test_new_symbols_are_declared_cited_bound_and_exported():
    from conan_slam_amd import _capi

    names = _capi.declared_symbols()
    assert set(NEED) == set(_capi.PF_VOTE_SYMBOLS)
    for s in NEED:
        assert s in names, s
        assert s in _capi._PROTOTYPES, s
    assert os.path.exists(_capi.LIB_PATH), "build the engine first: python -m conan_slam_amd.build"
    lib = ctypes.CDLL(_capi.LIB_PATH)
    assert not [s for s in NEED if not hasattr(lib, s)]
    text = open(_capi.HEADER_PATH).read()
    block = text[text.index("---- the vote on new features"):text.index("int cslam_pf_assoc_scan_step_drawn")]
    for cite in ("EKF.cpp:131-144, 235-326", "PF.cpp:502-544", "PF.cpp:222-277", "PF.cpp:9-60", "PF.cpp:419-471",
                 "PF.cpp:473-500", "test/main.cpp:279-328"):
        assert cite in block, cite
    src = open(os.path.join(ROOT, "conan_slam_amd", "csrc", "pf_vote_kernels.hpp")).read()
    assert f"kPfVoteLanes = {_capi.PF_VOTE_LANES};" in src and V.TILE == _capi.PF_VOTE_LANES
    assert "pf_assoc_vote_kernel" in src and "fp contract(off)" in src and "atomic" not in src.replace("no atomics", "")


def test_the_wrappers_mirror_the_calls():
    from conan_slam_amd.pf import ParticleShard

    for name in ("associate_vote", "vote_wait", "vote", "sample_proposal_voted", "sample_proposal_voted_drawn",
                 "feature_update_voted", "add_features_voted", "assoc_scan_step_drawn"):
        assert callable(getattr(ParticleShard, name, None)), name
    adapter = open(os.path.join(ROOT, "include", "cslam_adapter.hpp")).read()
    for name in ("associateVoteAll", "sampleProposalVotedAll", "addVotedFeaturesAll", "scanStepUnknownAll",
                 "cslam_pf_assoc_scan_step_drawn"):
        assert name in adapter, name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("associateVoteAll", "sampleProposalVotedAll", "addVotedFeaturesAll", "scanStepUnknownAll"):
        assert name in doc, name
