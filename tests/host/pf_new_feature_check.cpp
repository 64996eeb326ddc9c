// pf_new_feature_check.cpp -- host-only check of pf_new_feature_check in conan_slam_amd/csrc/pf_host_parts.hpp, the
// argument rule of cslam_pf_sample_pose / cslam_pf_new_feature_step and their _drawn forms (built and run by
// tests/test_pf_new_feature_cpu.py under the address and undefined-behaviour sanitizers).  No HIP.
#include <climits>
#include <cstdio>

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

int main()
{
    using R = PfNewFeatureRefusal;
    // q = 0: neither Z nor R is needed, the normals are
    CHECK(pf_new_feature_check(0, false, false, true, 0, 0) == R::none);
    CHECK(pf_new_feature_check(0, false, false, false, 0, 8) == R::bad_arg);
    CHECK(pf_new_feature_check(-1, true, true, true, 0, 8) == R::bad_arg);
    // q > 0: Z and R
    CHECK(pf_new_feature_check(2, true, true, true, 0, 8) == R::none);
    CHECK(pf_new_feature_check(2, false, true, true, 0, 8) == R::bad_arg);
    CHECK(pf_new_feature_check(2, true, false, true, 0, 8) == R::bad_arg);
    CHECK(pf_new_feature_check(2, true, true, false, 0, 8) == R::bad_arg);
    // the last slot of the store may be written, the one behind it not
    CHECK(pf_new_feature_check(2, true, true, true, 6, 8) == R::none);
    CHECK(pf_new_feature_check(3, true, true, true, 6, 8) == R::capacity);
    CHECK(pf_new_feature_check(1, true, true, true, 8, 8) == R::capacity);
    CHECK(pf_new_feature_check(1, true, true, true, 0, 0) == R::capacity);
    // a bad argument is reported before the capacity, and a huge q does not overflow nf + q
    CHECK(pf_new_feature_check(9, false, true, true, 6, 8) == R::bad_arg);
    CHECK(pf_new_feature_check(INT_MAX, true, true, true, 6, 8) == R::capacity);
    if (g_failed)
    {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("pf_new_feature_check: ok\n");
    return 0;
}
