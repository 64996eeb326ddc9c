// pf_control_check.cpp -- host-only check of the control run's host parts in conan_slam_amd/csrc/pf_host_parts.hpp: the
// split of k control steps into launches of kPfControlChunk (pf_control_chunks / pf_control_chunk) and the argument rule
// of cslam_pf_control_run and of the run in front of the cycle calls (pf_control_check).  Built and run by
// tests/test_pf_cycle_cpu.py, plain and under the address and undefined-behaviour sanitizers.  No HIP.
#include <climits>
#include <cstdio>
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

// the chunks of a run of k steps cover 0 .. k-1 once each, in order, none longer than a launch holds, none empty
static void check_split(int k, int expect_chunks, int expect_last)
{
    CHECK(pf_control_chunks(k) == expect_chunks);
    std::vector<int> seen((size_t)(k > 0 ? k : 0), 0);
    int              first = -1, count = -1, next = 0, c = 0, last = 0;
    for (; pf_control_chunk(k, c, &first, &count); c++)
    {
        CHECK(first == next);
        CHECK(count >= 1 && count <= kPfControlChunk);
        CHECK(first + count <= k);
        for (int j = first; j < first + count && j < k; j++)
        {
            seen[(size_t)j]++;
        }
        next = first + count;
        last = count;
    }
    CHECK(c == expect_chunks);
    CHECK(next == (k > 0 ? k : 0));
    CHECK(last == expect_last);
    CHECK(first == 0 && count == 0); // (what the refusing call leaves behind)
    for (int s : seen)
    {
        CHECK(s == 1);
    }
    int f = 7, n = 7;
    CHECK(!pf_control_chunk(k, -1, &f, &n) && f == 0 && n == 0);
    CHECK(!pf_control_chunk(k, expect_chunks, &f, &n));
}

int main()
{
    CHECK(kPfControlChunk == 16);
    check_split(0, 0, 0);
    check_split(1, 1, 1);
    check_split(15, 1, 15);
    check_split(16, 1, 16);
    check_split(17, 2, 1);
    check_split(32, 2, 16);
    check_split(33, 3, 1);
    check_split(-1, 0, 0);
    check_split(INT_MIN, 0, 0);
    CHECK(pf_control_chunks(INT_MAX) == INT_MAX / 16 + 1); // (no overflow in the rounding up)
    int f = 0, n = 0;
    CHECK(pf_control_chunk(INT_MAX, INT_MAX / 16, &f, &n) && f == INT_MAX - 15 && n == 15);

    // every combination of (k, v, swa, Q, phi, heading)
    using R = PfControlRefusal;
    for (int k : {-5, -1, 0, 1, 16, 33})
    {
        for (int bits = 0; bits < 32; bits++)
        {
            const bool v = bits & 1, swa = bits & 2, Q = bits & 4, phi = bits & 8, use = bits & 16;
            R          expect = R::none;
            if (k < 0)
            {
                expect = R::bad_k;
            }
            else if (k > 0 && !(v && swa && Q))
            {
                expect = R::null_control;
            }
            else if (k > 0 && use && !phi)
            {
                expect = R::null_phi;
            }
            CHECK(pf_control_check(k, v, swa, Q, phi, use) == expect);
        }
    }
    // spelled out: nothing is read at k = 0; phi only with the heading; a bad k before a null array
    CHECK(pf_control_check(0, false, false, false, false, true) == R::none);
    CHECK(pf_control_check(3, true, true, true, false, false) == R::none);
    CHECK(pf_control_check(3, true, true, true, false, true) == R::null_phi);
    CHECK(pf_control_check(3, false, true, true, true, true) == R::null_control);
    CHECK(pf_control_check(3, true, false, true, true, true) == R::null_control);
    CHECK(pf_control_check(3, true, true, false, true, true) == R::null_control);
    CHECK(pf_control_check(-1, false, false, false, false, false) == R::bad_k);
    std::printf("pf_control_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
