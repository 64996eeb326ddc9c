// pf_fs1_check.cpp -- host-only check of the refusal rules of the FastSLAM-1 step in
// conan_slam_amd/csrc/pf_host_parts.hpp: pf_fs1_control_check (cslam_pf_control_run_sampled and the run in front of
// cslam_pf_fs1_cycle_drawn), pf_fs1_draws_check (cslam_pf_get_control_draws), pf_fs1_scan_check (cslam_pf_likelihood_update
// and the scan of the cycle) and pf_fs1_chunk_step.  Built and run by tests/test_pf_fs1_cpu.py, plain and under the address
// and undefined-behaviour sanitizers.  No HIP.
#include <climits>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "pf_host_parts.hpp"

using namespace cslam;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                       \
    do                                                                    \
    {                                                                     \
        g_checks++;                                                       \
        if (!(cond))                                                      \
        {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                   \
        }                                                                 \
    } while (0)

int main()
{
    using R = PfFs1Refusal;
    const double good[2] = {0.09, 3e-3}, zero[2] = {0.0, 0.0}, neg0[2] = {-1e-30, 1.0}, neg1[2] = {1.0, -2.0};
    const double nan0[2] = {std::numeric_limits<double>::quiet_NaN(), 1.0}, mzero[2] = {-0.0, -0.0};

    // the control rule in front: every combination of (k, v, swa, Q, phi, heading) refuses what pf_control_check refuses
    for (int k : {-5, -1, 0, 1, 16, 33})
    {
        for (int bits = 0; bits < 32; bits++)
        {
            const bool v = bits & 1, swa = bits & 2, Q = bits & 4, phi = bits & 8, use = bits & 16;
            R          expect = R::none;
            switch (pf_control_check(k, v, swa, Q, phi, use))
            {
            case PfControlRefusal::none:
                break;
            case PfControlRefusal::bad_k:
                expect = R::bad_k;
                break;
            case PfControlRefusal::null_control:
                expect = R::null_control;
                break;
            case PfControlRefusal::null_phi:
                expect = R::null_phi;
                break;
            }
            CHECK(pf_fs1_control_check(k, v, swa, Q ? good : nullptr, phi, use, 0) == expect);
            CHECK(pf_fs1_control_check(k, v, swa, Q ? good : nullptr, phi, use, LLONG_MAX) == expect);
            // a negative control step is refused wherever the arrays pass
            CHECK(pf_fs1_control_check(k, v, swa, Q ? good : nullptr, phi, use, -1) == (expect == R::none ? R::bad_step : expect));
        }
    }
    // the diagonal of Q: zero (and minus zero) is the noise-free run, a negative value or a NaN has no standard deviation
    CHECK(pf_fs1_control_check(3, true, true, zero, true, true, 5) == R::none);
    CHECK(pf_fs1_control_check(3, true, true, mzero, true, true, 5) == R::none);
    CHECK(pf_fs1_control_check(3, true, true, neg0, true, true, 5) == R::bad_q);
    CHECK(pf_fs1_control_check(3, true, true, neg1, true, true, 5) == R::bad_q);
    CHECK(pf_fs1_control_check(3, true, true, nan0, true, true, 5) == R::bad_q);
    // nothing is read at k = 0 -- not even Q -- but k and ctl_step are still looked at
    CHECK(pf_fs1_control_check(0, false, false, nullptr, false, true, 0) == R::none);
    CHECK(pf_fs1_control_check(0, false, false, neg0, false, true, 0) == R::none);
    CHECK(pf_fs1_control_check(0, false, false, nullptr, false, true, -1) == R::bad_step);
    CHECK(pf_fs1_control_check(0, false, false, nullptr, false, true, LLONG_MIN) == R::bad_step);
    // the order: k, the arrays, the step, Q
    CHECK(pf_fs1_control_check(-1, true, true, neg0, true, true, -1) == R::bad_k);
    CHECK(pf_fs1_control_check(3, true, true, neg0, false, true, -1) == R::null_phi);
    CHECK(pf_fs1_control_check(3, true, true, neg0, true, true, -1) == R::bad_step);

    // the draws read
    CHECK(pf_fs1_draws_check(0, 0, false) == R::none);
    CHECK(pf_fs1_draws_check(3, 0, true) == R::none);
    CHECK(pf_fs1_draws_check(3, (1LL << 31) + 5, true) == R::none);
    CHECK(pf_fs1_draws_check(3, 0, false) == R::null_control);
    CHECK(pf_fs1_draws_check(-1, 0, true) == R::bad_k);
    CHECK(pf_fs1_draws_check(3, -1, true) == R::bad_step);

    // the scan
    const int idf[4] = {3, 1, 8, 2}, low[3] = {3, 0, 9}, high[3] = {3, 9, 0}, twice[3] = {2, 5, 2};
    int       index  = 7;
    CHECK(pf_fs1_scan_check(0, false, nullptr, 0, false, false, 8, 9, &index) == R::none && index == -1);
    CHECK(pf_fs1_scan_check(4, true, idf, 0, false, true, 8, 8, &index) == R::none && index == -1);
    CHECK(pf_fs1_scan_check(4, true, idf, 1, true, true, 8, 9, &index) == R::none);
    CHECK(pf_fs1_scan_check(3, true, twice, 0, false, true, 8, 8, &index) == R::none); // (a feature named twice is no refusal)
    CHECK(pf_fs1_scan_check(0, false, nullptr, 2, true, true, 0, 2, &index) == R::none); // (from an empty map)
    CHECK(pf_fs1_scan_check(-1, true, idf, 0, false, true, 8, 9, &index) == R::bad_scan);
    CHECK(pf_fs1_scan_check(4, true, idf, -1, true, true, 8, 9, &index) == R::bad_scan);
    CHECK(pf_fs1_scan_check(4, false, idf, 0, false, true, 8, 9, &index) == R::bad_scan);
    CHECK(pf_fs1_scan_check(4, true, nullptr, 0, false, true, 8, 9, &index) == R::bad_scan);
    CHECK(pf_fs1_scan_check(4, true, idf, 0, false, false, 8, 9, &index) == R::bad_scan);
    CHECK(pf_fs1_scan_check(0, false, nullptr, 1, false, true, 8, 9, &index) == R::bad_scan);
    CHECK(pf_fs1_scan_check(0, false, nullptr, 1, true, false, 8, 9, &index) == R::bad_scan);
    CHECK(pf_fs1_scan_check(3, true, low, 0, false, true, 8, 9, &index) == R::bad_idf && index == 1);
    CHECK(pf_fs1_scan_check(3, true, high, 0, false, true, 8, 9, &index) == R::bad_idf && index == 1);
    CHECK(pf_fs1_scan_check(4, true, idf, 0, false, true, 7, 9, &index) == R::bad_idf && index == 2); // (8 on a map of 7)
    CHECK(pf_fs1_scan_check(4, true, idf, 0, false, true, 0, 9, &index) == R::bad_idf && index == 0); // (an empty map)
    CHECK(pf_fs1_scan_check(4, true, idf, 2, true, true, 8, 9, &index) == R::capacity && index == -1);
    CHECK(pf_fs1_scan_check(0, false, nullptr, 1, true, true, 9, 9, &index) == R::capacity);
    CHECK(pf_fs1_scan_check(0, false, nullptr, INT_MAX, true, true, 9, 9, &index) == R::capacity); // (no overflow)
    // a bad idf before the capacity, a null array before either
    CHECK(pf_fs1_scan_check(3, true, low, 5, true, true, 8, 9, &index) == R::bad_idf);
    CHECK(pf_fs1_scan_check(3, true, low, 5, false, true, 8, 9, &index) == R::bad_scan);
    // a long list is walked to its end and no further
    std::vector<int> big(1000);
    for (int i = 0; i < 1000; i++)
    {
        big[(size_t)i] = i % 40 + 1;
    }
    CHECK(pf_fs1_scan_check(1000, true, big.data(), 0, false, true, 40, 40, &index) == R::none);
    big[999] = 41;
    CHECK(pf_fs1_scan_check(1000, true, big.data(), 0, false, true, 40, 40, &index) == R::bad_idf && index == 999);
    CHECK(pf_fs1_scan_check(999, true, big.data(), 0, false, true, 40, 40, &index) == R::none);

    // chunk c of a sampled run starts 16 c control steps on
    CHECK(pf_fs1_chunk_step(0, 0) == 0 && pf_fs1_chunk_step(5, 1) == 21 && pf_fs1_chunk_step(5, 2) == 37);
    CHECK(pf_fs1_chunk_step((1LL << 31) + 5, 2) == (1LL << 31) + 37);
    int first = 0, count = 0;
    for (int c = 0; pf_control_chunk(33, c, &first, &count); c++)
    {
        CHECK(pf_fs1_chunk_step(100, c) == 100 + first);
    }
    std::printf("pf_fs1_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
