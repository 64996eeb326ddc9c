// pf_score_book_check.cpp -- host-only check of PfScoreBook (conan_slam_amd/csrc/pf_host_parts.hpp), the bookkeeping of
// the particle filter's device-side score: argument rules, default gates, the call count, which record the next call
// writes, records = min(calls, capacity), how many a read copies, how many features a call scores and in how many
// workgroups, and whether an allocated log serves a reset.  Built and run by tests/test_pf_score_host_cpu.py with plain
// g++ and once more under the address and undefined-behaviour sanitizers.  No HIP.
#include <cmath>
#include <cstdio>
#include <limits>

#include "pf_host_parts.hpp"

using namespace cslam;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do                                                                    \
    {                                                                     \
        if (!(cond))                                                      \
        {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

static void check_arguments()
{
    CHECK(PfScoreBook::reset_args_ok(0, 0) && PfScoreBook::reset_args_ok(1, 0) && PfScoreBook::reset_args_ok(1, 1 << 20));
    CHECK(!PfScoreBook::reset_args_ok(2, 0) && !PfScoreBook::reset_args_ok(-1, 0) && !PfScoreBook::reset_args_ok(0, -1));
    CHECK(PfScoreBook::truth_args_ok(0, 0) && PfScoreBook::truth_args_ok(5, 5) && PfScoreBook::truth_args_ok(0, 5));
    CHECK(!PfScoreBook::truth_args_ok(-1, 5) && !PfScoreBook::truth_args_ok(6, 5) && !PfScoreBook::truth_args_ok(1, 0));
}

static void check_defaults_and_gates()
{
    PfScoreBook b; // never reset: as after reset(0, 0, 0, 0)
    PfScoreBook r;
    r.reset(0, 0, 0.0, 0.0);
    for (const PfScoreBook* p : {&b, &r})
    {
        CHECK(p->estimator() == 0 && p->capacity() == 0 && p->calls() == 0 && p->truth_count() == 0);
        CHECK(p->gate_pose() == 7.8147 && p->gate_lm() == 5.9915);
        CHECK(p->next_record() == -1 && p->records() == 0);
    }
    b.reset(1, 3, -1.0, std::numeric_limits<double>::quiet_NaN());
    CHECK(b.estimator() == 1 && b.capacity() == 3 && b.gate_pose() == 7.8147 && b.gate_lm() == 5.9915);
    b.reset(0, 3, 2.5, 1e-300);
    CHECK(b.gate_pose() == 2.5 && b.gate_lm() == 1e-300);
    b.reset(0, 3, std::numeric_limits<double>::infinity(), 4.0);
    CHECK(std::isinf(b.gate_pose()) && b.gate_lm() == 4.0);
}

static void check_records()
{
    PfScoreBook b;
    b.set_truth_count(7);
    b.reset(1, 2, 0.0, 0.0);
    CHECK(b.truth_count() == 7); // a reset keeps the truth
    const long long want_next[5] = {0, 1, -1, -1, -1};
    const int       want_rec[5]  = {0, 1, 2, 2, 2};
    for (int i = 0; i < 5; i++)
    {
        CHECK(b.calls() == i && b.next_record() == want_next[i] && b.records() == want_rec[i]);
        b.called();
    }
    CHECK(b.calls() == 5 && b.records() == 2);
    CHECK(b.records_to_copy(0) == 0 && b.records_to_copy(1) == 1 && b.records_to_copy(2) == 2 && b.records_to_copy(9) == 2);
    CHECK(b.records_to_copy(-3) == 0);
    b.reset(0, 0, 0.0, 0.0);
    CHECK(b.calls() == 0 && b.records() == 0 && b.next_record() == -1 && b.records_to_copy(4) == 0);
    for (int i = 0; i < 3; i++)
    {
        b.called(); // totals only: the calls still count
    }
    CHECK(b.calls() == 3 && b.records() == 0 && b.next_record() == -1);
    // a capacity beyond any call count, and a call count beyond an int
    b.reset(0, std::numeric_limits<int>::max(), 0.0, 0.0);
    CHECK(b.next_record() == 0 && b.records() == 0);
}

static void check_scored_and_blocks()
{
    PfScoreBook b;
    CHECK(b.scored(5, 1) == 0); // no truth yet
    b.set_truth_count(200);
    CHECK(b.scored(257, 1) == 200 && b.scored(100, 1) == 100 && b.scored(0, 1) == 0 && b.scored(257, 0) == 0);
    b.set_truth_count(0);
    CHECK(b.scored(257, 1) == 0);
    CHECK(PfScoreBook::blocks(0) == 0 && PfScoreBook::blocks(1) == 1 && PfScoreBook::blocks(256) == 1 &&
          PfScoreBook::blocks(257) == 2 && PfScoreBook::blocks(512) == 2 && PfScoreBook::blocks(513) == 3);
    // every feature has a lane, and no workgroup is empty
    for (int c = 1; c < 1100; c++)
    {
        const int g = PfScoreBook::blocks(c);
        CHECK(g * PfScoreBook::kLanes >= c && (g - 1) * PfScoreBook::kLanes < c);
    }
}

static void check_series_fits()
{
    CHECK(PfScoreBook::series_fits(0, 0));   // totals only: nothing to allocate
    CHECK(!PfScoreBook::series_fits(0, 1));
    CHECK(PfScoreBook::series_fits(8, 8) && PfScoreBook::series_fits(8, 3) && !PfScoreBook::series_fits(8, 9));
}

int main()
{
    check_arguments();
    check_defaults_and_gates();
    check_records();
    check_scored_and_blocks();
    check_series_fits();
    std::printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
