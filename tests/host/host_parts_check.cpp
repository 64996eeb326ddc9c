// host_parts_check.cpp -- host-only check of conan_slam_amd/csrc/ekf_options.hpp and ekf_pending_store.hpp (built and run
// by tests/test_host_parts_cpu.py, with plain g++ and once more under the address and undefined-behaviour sanitizers).
// Options: the defaults DESIGN.md lists, then every variable parsed by from_env(), with each clamp.  Pending store: its
// invariants as event sequences.  No HIP.
#include <cstdio>
#include <cstdlib>

#include "ekf_options.hpp"
#include "ekf_pending_store.hpp"

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

static const char* const kVars[] = {
    "CSLAM_FUSE_PREDICT", "CSLAM_FUSE_F64",     "CSLAM_SEQ_DEFER",   "CSLAM_STORAGE",      "CSLAM_PIPELINE",
    "CSLAM_PGEMM_SPARE",  "CSLAM_GATHER_WIDE",  "CSLAM_LOOKAHEAD",   "CSLAM_LA_HOLD_WIDE", "CSLAM_LA_K64",
    "CSLAM_LA_WG_SIGNAL", "CSLAM_LA_MIRROR",    "CSLAM_LA_FUSED",    "CSLAM_LA_STAMPS",    "CSLAM_PGEMM_LIMBS",
    "CSLAM_LIMBS_KMIN",   "CSLAM_XCD_QUEUES",   "CSLAM_PSYM_NT",     "CSLAM_F64_KCM",      "CSLAM_F64_CB",
    "CSLAM_BATCH_WG_SIGNAL", "CSLAM_BATCH_WIDE_PAIRS", "CSLAM_BATCH_STAMPS"};

static void clear_env()
{
    for (const char* v : kVars)
    {
        unsetenv(v);
    }
}

// the single-filter options with ONE variable set
static EkfOptions with(const char* name, const char* value)
{
    clear_env();
    setenv(name, value, 1);
    const EkfOptions o = EkfOptions::from_env();
    unsetenv(name);
    return o;
}
static EkfBatchOptions bwith(const char* name, const char* value)
{
    clear_env();
    setenv(name, value, 1);
    const EkfBatchOptions o = EkfBatchOptions::from_env();
    unsetenv(name);
    return o;
}

static void check_defaults()
{
    clear_env();
    const EkfOptions o = EkfOptions::from_env();
    CHECK(o.fuse_predict == 1 && o.fuse_f64 == 1 && o.seq_defer == 1);
    CHECK(o.lower == 1 && o.pipeline == 0 && o.pgemm_spare == 16 && o.gather_corr_wide == 1);
    CHECK(o.lookahead == -1 && o.la_hold_wide == 1 && o.la_k64 == 1 && o.la_wg_signal == 0 && o.la_mirror == 1);
    CHECK(o.la_fused == 1 && o.la_stamps == 0);
    CHECK(o.pgemm_limbs == 0 && o.limbs_kmin == 65 && o.xcd_queues == 0 && o.psym_nt == -1);
    CHECK(o.f64_kcm == 16 && o.f64_cb == 0);
    const EkfBatchOptions b = EkfBatchOptions::from_env();
    CHECK(b.wg_signal == 0 && b.wide_pairs == 2 && b.la_k64 == 1 && b.stamps == 0);
}

static void check_values_and_clamps()
{
    // one in-range value per variable
    CHECK(with("CSLAM_FUSE_PREDICT", "0").fuse_predict == 0);
    CHECK(with("CSLAM_FUSE_F64", "0").fuse_f64 == 0);
    CHECK(with("CSLAM_SEQ_DEFER", "0").seq_defer == 0);
    CHECK(with("CSLAM_PIPELINE", "1").pipeline == 1);
    CHECK(with("CSLAM_PGEMM_SPARE", "64").pgemm_spare == 64);
    CHECK(with("CSLAM_GATHER_WIDE", "0").gather_corr_wide == 0);
    CHECK(with("CSLAM_LOOKAHEAD", "1").lookahead == 1);
    CHECK(with("CSLAM_LOOKAHEAD", "0").lookahead == 0);
    CHECK(with("CSLAM_LA_HOLD_WIDE", "0").la_hold_wide == 0);
    CHECK(with("CSLAM_LA_K64", "0").la_k64 == 0);
    CHECK(with("CSLAM_LA_WG_SIGNAL", "1").la_wg_signal == 1);
    CHECK(with("CSLAM_LA_MIRROR", "0").la_mirror == 0);
    CHECK(with("CSLAM_LA_FUSED", "0").la_fused == 0);
    CHECK(with("CSLAM_LA_STAMPS", "1").la_stamps == 1);
    CHECK(with("CSLAM_PGEMM_LIMBS", "9").pgemm_limbs == 9);
    CHECK(with("CSLAM_PGEMM_LIMBS", "6").pgemm_limbs == 6);
    CHECK(with("CSLAM_LIMBS_KMIN", "96").limbs_kmin == 96);
    CHECK(with("CSLAM_XCD_QUEUES", "1").xcd_queues == 1);
    CHECK(with("CSLAM_PSYM_NT", "1").psym_nt == 1);
    CHECK(with("CSLAM_PSYM_NT", "0").psym_nt == 0);
    CHECK(with("CSLAM_F64_KCM", "32").f64_kcm == 32);
    CHECK(with("CSLAM_F64_CB", "2").f64_cb == 2);
    CHECK(with("CSLAM_F64_CB", "4").f64_cb == 4);
    // a variable changes its own field only
    CHECK(with("CSLAM_PIPELINE", "1").lower == 1 && with("CSLAM_LA_FUSED", "0").lookahead == -1);
    // the clamps
    CHECK(with("CSLAM_PGEMM_LIMBS", "7").pgemm_limbs == 0);
    CHECK(with("CSLAM_LIMBS_KMIN", "10").limbs_kmin == 57 && with("CSLAM_LIMBS_KMIN", "-1").limbs_kmin == 65);
    CHECK(with("CSLAM_LOOKAHEAD", "-3").lookahead == -1);
    CHECK(with("CSLAM_LOOKAHEAD", "5").lookahead == 1);
    CHECK(with("CSLAM_F64_KCM", "70").f64_kcm == 64);
    CHECK(with("CSLAM_F64_KCM", "1").f64_kcm == 4);
    CHECK(with("CSLAM_F64_KCM", "18").f64_kcm == 20); // (rounded up to a multiple of 4)
    CHECK(with("CSLAM_F64_CB", "3").f64_cb == 4);
    CHECK(with("CSLAM_STORAGE", "lower").lower == 1);
    CHECK(with("CSLAM_STORAGE", "full").lower == 0);
    CHECK(with("CSLAM_PGEMM_SPARE", "-4").pgemm_spare == 0);
    // the batched engine
    CHECK(bwith("CSLAM_BATCH_WG_SIGNAL", "1").wg_signal == 1);
    CHECK(bwith("CSLAM_BATCH_WIDE_PAIRS", "1").wide_pairs == 1);
    CHECK(bwith("CSLAM_BATCH_WIDE_PAIRS", "3").wide_pairs == 2);
    CHECK(bwith("CSLAM_LA_K64", "0").la_k64 == 0);
    CHECK(bwith("CSLAM_BATCH_STAMPS", "1").stamps == 1);
    // the result is a value: the environment afterwards does not reach it
    clear_env();
    setenv("CSLAM_LOOKAHEAD", "1", 1);
    const EkfOptions kept = EkfOptions::from_env();
    unsetenv("CSLAM_LOOKAHEAD");
    CHECK(kept.lookahead == 1 && EkfOptions::from_env().lookahead == -1);
}

static void check_mirror()
{
    const int   n = 1203;
    PendingCols p;
    p.regrown(256);
    p.appended(64);
    p.appended(64);
    p.mirror_written(128, n);
    CHECK(p.kp == 128 && p.mirror_covers(p.kp, n));
    CHECK(!p.mirror_covers(p.kp, n + 2)); // (the map has grown since)
    p.appended(1, true);                  // a heading column the mirror does not hold
    CHECK(p.kp == 129 && !p.mirror_covers(p.kp, n));
    // applied: nothing pending, the other region, mirror void
    PendingCols q;
    q.regrown(256);
    q.appended(128);
    q.mirror_written(128, n);
    CHECK(!q.applied());
    CHECK(q.kp == 0 && q.wcur == 1 && !q.mirror_covers(128, n) && !q.mirror_covers(0, n));
    q.mirror_written(64, n);
    q.mirror_void();
    CHECK(!q.mirror_covers(64, n));
}

static void check_in_flight()
{
    PendingCols p;
    p.regrown(128);
    CHECK(!p.in_flight() && !p.in_flight(0) && !p.in_flight(1));
    p.appended(64);
    p.pgemm_on_second_stream(); // region 0 is read by a P-GEMM on stream B
    p.applied();
    CHECK(p.wcur == 1 && p.inflight_mask == 1u);
    CHECK(p.in_flight() && p.in_flight(0) && !p.in_flight(1)); // own_region(1) needs no wait, own_region(0) does
    p.waited();
    CHECK(!p.in_flight() && !p.in_flight(0));
    // both regions in flight, one wait for both
    p.appended(8);
    p.pgemm_on_second_stream();
    p.applied();
    p.appended(8);
    p.pgemm_on_second_stream();
    p.applied();
    CHECK(p.inflight_mask == 3u && p.in_flight(0) && p.in_flight(1));
    p.waited();
    CHECK(p.inflight_mask == 0u);
    // a single-stream flush marks nothing
    p.appended(8);
    p.applied();
    CHECK(!p.in_flight());
}

static void check_heading_counts()
{
    PendingCols p;
    p.regrown(128);
    p.appended(1, true);
    p.appended(64);
    p.appended(2, true);
    CHECK(p.kp == 67 && p.hd_cols[0] == 3 && p.hd_cols[1] == 0);
    // region 0 applied: region 1 was never used, nothing to clear; region 0 keeps its count (its signs are still set)
    CHECK(!p.applied());
    CHECK(p.wcur == 1 && p.hd_cols[0] == 3 && p.hd_cols[1] == 0);
    p.appended(1, true);
    CHECK(p.hd_cols[0] == 3 && p.hd_cols[1] == 1);
    // region 1 applied: region 0 becomes current again after having been applied -> its signs are cleared, its count reset
    CHECK(p.applied());
    CHECK(p.wcur == 0 && p.hd_cols[0] == 0 && p.hd_cols[1] == 1);
    p.appended(64); // no heading column this time
    CHECK(p.applied());
    CHECK(p.wcur == 1 && p.hd_cols[0] == 0 && p.hd_cols[1] == 0);
    CHECK(!p.applied());
}

static void check_discard_and_regrow()
{
    PendingCols p;
    p.regrown(128);
    p.appended(64);
    p.pgemm_on_second_stream();
    p.applied();
    p.appended(3, true);
    p.mirror_written(3, 77);
    p.discarded();
    CHECK(p.wcap == 128 && p.wcur == 0 && p.kp == 0 && p.hd_cols[0] == 0 && p.hd_cols[1] == 0);
    CHECK(!p.in_flight() && !p.mirror_covers(3, 77));
    p.appended(8);
    p.applied();
    p.appended(5, true);
    p.mirror_written(5, 77);
    p.regrown(256);
    CHECK(p.wcap == 256 && p.wcur == 0 && p.kp == 0 && p.hd_cols[0] == 0 && p.hd_cols[1] == 0);
    CHECK(!p.in_flight() && !p.mirror_covers(5, 77));
}

int main()
{
    check_defaults();
    check_values_and_clamps();
    check_mirror();
    check_in_flight();
    check_heading_counts();
    check_discard_and_regrow();
    std::printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
