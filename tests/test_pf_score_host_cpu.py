"""The host-side bookkeeping of the particle filter's device-side score (PfScoreBook of
conan_slam_amd/csrc/pf_host_parts.hpp: call count, capacity, records = min(calls, capacity), gates, scored features and
workgroups): a C++ check with its own main, built with plain g++ and run here -- once as it is, once as a stand-alone
program under the address and undefined-behaviour sanitizers, the way tests/test_host_parts_cpu.py drives its checks."""
from test_host_parts_cpu import build_and_run


def test_pf_score_book_check_builds_and_passes(tmp_path):
    build_and_run("pf_score_book_check", tmp_path)
