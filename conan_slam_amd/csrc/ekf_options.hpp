// ekf_options.hpp -- the engine switches of the EKF handles (DESIGN.md 6 "Engine switches").  Host only, no HIP.
// from_env() is the ONE place that reads the environment: cslam_ekf_create and cslam_ekf_batch_create* call it once and
// the handle keeps the result, so a variable set or cleared after create changes nothing and no launch path parses a string.
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace cslam
{
inline int env_int(const char* name, int dflt) { const char* s = getenv(name); return s ? atoi(s) : dflt; }
inline int env_flag(const char* name, int dflt) { const char* s = getenv(name); return s ? (atoi(s) ? 1 : 0) : dflt; }
// CSLAM_PGEMM_TAIL, the tail phase of the f32 P-GEMM (ekf_pgemm_tiles.hpp): tiles handed out as 32-row strips.  -1: the
// value's own meaning is "by the rule" (a negative value reads as that), 0: no strips, N > 0: exactly min(N, tiles) tiles
constexpr int kPgemmTailMax = 1 << 20;
inline int env_pgemm_tail(int dflt) { return std::max(-1, std::min(kPgemmTailMax, env_int("CSLAM_PGEMM_TAIL", dflt))); }

struct EkfOptions
{
    int fuse_predict = 1; // predicts / headings are held and fused (CSLAM_FUSE_PREDICT=0 launches every one at once)
    int fuse_f64     = 1; // the f64 MFMA kernels take a held predict too (CSLAM_FUSE_F64=0: its own launch)
    int seq_defer    = 1; // sequential update(): one P-GEMM per call (CSLAM_SEQ_DEFER=0 restores m passes)
    // Block-lower storage (default): only the 128x128 tiles on / below the tile diagonal of the symmetric P are maintained
    // (the P-GEMM writes each tile once).  CSLAM_STORAGE=full keeps both triangles (mirror stores in the P-GEMM).
    int lower = 1;
    // P-GEMM of update t on stream B under the chain of update t+1 (CSLAM_PIPELINE=1).  An option, not the default:
    // measured at N = 5000, k = 64 (profiles/r02_*): the kernels of update t+1 that touch memory crawl underneath the
    // persistent P-GEMM (its waves are older and keep ~24 KB of requests in flight each: the pending-panel correction
    // takes 65 us instead of 5.5) and every cross-stream hand-over costs ~6 us, so the period is 138 us against 112 us
    // on one stream.
    int pipeline    = 0;
    int pgemm_spare = 16; // pipelined: workgroups the persistent P-GEMM grid leaves out (CSLAM_PGEMM_SPARE >= 0)
    int gather_corr_wide = 1; // a pending batch panel (<= 64 columns) corrected for inside the gather kernel (CSLAM_GATHER_WIDE)
    int lookahead    = -1; // look-ahead windows (ekf_lookahead.hpp): -1 where they pay, CSLAM_LOOKAHEAD=1 / 0 forces
    int la_hold_wide = 1;  // CSLAM_LA_HOLD_WIDE=0: every window launches its own wide kernel at once (A/B)
    int la_k64       = 1;  // CSLAM_LA_K64=0: the general wide kernel for m = 32 too (A/B)
    int la_wg_signal = 0;  // CSLAM_LA_WG_SIGNAL=1: always the blocks kernel's own release (A/B: the first form)
    int la_mirror    = 1;  // CSLAM_LA_MIRROR=0: rows + blocks kernels for every window, no mirror stores (A/B)
    int la_fused     = 1;  // CSLAM_LA_FUSED=0: gather + gain per update instead of the one wide launch (A/B)
    int la_stamps    = 0;  // CSLAM_LA_STAMPS set: phase stamps of factor(a) underneath the P-GEMM and of the wide kernel
    // f32 P-GEMM on the bf16 matrix cores (ekf_pgemm_limbs.hpp): limb pairs per product (9 exact, 6, 0 = the f32 MFMA
    // kernel; CSLAM_PGEMM_LIMBS) and from how many columns on (CSLAM_LIMBS_KMIN; at least four chunks of 16: k8 >= 57
    // rounds to 64).  Off by default: correct and as accurate as the f32 MFMA kernel (tests), but measured no faster --
    // 120 - 132 us against 115 at k = 128, N = 5000 -- see DESIGN.md 8.
    int pgemm_limbs = 0;
    int limbs_kmin  = 65;
    // the f32 P-GEMM draws its tiles from one queue per XCD over a Morton-ordered list (CSLAM_XCD_QUEUES=1).  Off by
    // default: it cuts the HBM fetch traffic of a launch by a sixth (k = 64: 487 -> 435 MB, 1.04x the algorithmic bytes;
    // k = 128: 584 -> 483 MB) but not its time (81.7 vs 80.9 us, 115.3 vs 114.6 us), and the loops built on it came out
    // 0 - 4 % slower (profiles/r02_pmc_xcd_queues.txt)
    int xcd_queues = 0;
    int psym_nt    = -1; // CSLAM_PSYM_NT=0|1: non-temporal P accesses in the P-GEMM (-1: by footprint)
    int pgemm_tail = -1; // CSLAM_PGEMM_TAIL: tiles the P-GEMM hands out as strips (-1: by the rule, 0: none, N: exactly N)
    // f64 P-GEMM: columns of W1 staged per pass: 16, register-staged and double-buffered (see the kernel).  The
    // synchronous staging loop (other values of CSLAM_F64_KCM, a multiple of 4 in 4..64) measured at N = 1000, k = 64:
    // 8 / 16 / 32 -> 22.8 / 21.9 / 22.9 us, 64 (the whole panel at once, 96 KB of LDS, one workgroup per CU) -> 30.5 us.
    int f64_kcm = 16;
    int f64_cb  = 0; // f64 P-GEMM tile width in 16 columns: CSLAM_F64_CB = 2 or 4 (0: by the size of the state)

    static EkfOptions from_env()
    {
        EkfOptions o;
        o.fuse_predict     = env_int("CSLAM_FUSE_PREDICT", o.fuse_predict);
        o.fuse_f64         = env_flag("CSLAM_FUSE_F64", o.fuse_f64);
        o.seq_defer        = env_int("CSLAM_SEQ_DEFER", o.seq_defer);
        const char* sv     = getenv("CSLAM_STORAGE");
        o.lower            = (sv && !strcmp(sv, "full")) ? 0 : 1;
        o.pipeline         = env_flag("CSLAM_PIPELINE", o.pipeline);
        o.pgemm_spare      = std::max(0, env_int("CSLAM_PGEMM_SPARE", o.pgemm_spare));
        o.gather_corr_wide = env_flag("CSLAM_GATHER_WIDE", o.gather_corr_wide);
        const int la       = env_int("CSLAM_LOOKAHEAD", o.lookahead);
        o.lookahead        = la > 0 ? 1 : (la < 0 ? -1 : 0);
        o.la_hold_wide     = env_flag("CSLAM_LA_HOLD_WIDE", o.la_hold_wide);
        o.la_k64           = env_flag("CSLAM_LA_K64", o.la_k64);
        o.la_wg_signal     = env_flag("CSLAM_LA_WG_SIGNAL", o.la_wg_signal);
        o.la_mirror        = env_flag("CSLAM_LA_MIRROR", o.la_mirror);
        o.la_fused         = env_flag("CSLAM_LA_FUSED", o.la_fused);
        o.la_stamps        = getenv("CSLAM_LA_STAMPS") ? 1 : 0;
        const int limbs    = env_int("CSLAM_PGEMM_LIMBS", o.pgemm_limbs);
        o.pgemm_limbs      = (limbs == 6 || limbs == 9) ? limbs : 0;
        const int kmin     = env_int("CSLAM_LIMBS_KMIN", o.limbs_kmin);
        o.limbs_kmin       = kmin < 0 ? o.limbs_kmin : std::max(57, kmin); // (a negative value keeps the default)
        o.xcd_queues       = env_flag("CSLAM_XCD_QUEUES", o.xcd_queues);
        o.psym_nt          = env_flag("CSLAM_PSYM_NT", o.psym_nt);
        o.pgemm_tail       = env_pgemm_tail(o.pgemm_tail);
        o.f64_kcm          = std::max(4, std::min(64, (env_int("CSLAM_F64_KCM", o.f64_kcm) + 3) / 4 * 4));
        if (getenv("CSLAM_F64_CB"))
        {
            o.f64_cb = env_int("CSLAM_F64_CB", 0) == 2 ? 2 : 4;
        }
        return o;
    }
};

struct EkfBatchOptions
{
    // A/B switches: the first forms of two stages, kept measurable
    int wg_signal  = 0; // CSLAM_BATCH_WG_SIGNAL=1: the blocks kernel's workgroups release the chains themselves
    int wide_pairs = 2; // 32-row blocks per wide workgroup (CSLAM_BATCH_WIDE_PAIRS=1: one, the first form)
    int la_k64     = 1; // CSLAM_LA_K64=0: the general wide kernel for m = 32 too (A/B)
    int stamps     = 0; // CSLAM_BATCH_STAMPS set: see LaBatchWin::stamps (printed after 300 windows)
    int pgemm_tail = -1; // CSLAM_PGEMM_TAIL as above (by the rule: measured to pay at 8 x N = 2000)

    static EkfBatchOptions from_env()
    {
        EkfBatchOptions o;
        o.wg_signal  = env_flag("CSLAM_BATCH_WG_SIGNAL", o.wg_signal);
        o.wide_pairs = env_int("CSLAM_BATCH_WIDE_PAIRS", o.wide_pairs) == 1 ? 1 : 2;
        o.la_k64     = env_flag("CSLAM_LA_K64", o.la_k64);
        o.stamps     = getenv("CSLAM_BATCH_STAMPS") ? 1 : 0;
        o.pgemm_tail = env_pgemm_tail(o.pgemm_tail);
        return o;
    }
};

} // namespace cslam
