// cslam_ekf.hip -- host side of the EKF-SLAM engine behind the C ABI of include/cslam.h.
//
// One handle = one filter instance bound to one device; X and P live in HBM for the lifetime of the handle.
// update() is a chain of launches on the handle's stream: gather (+ the correction for pending panels), factor, gain
// (which also takes the pose stripe's share of the downdate), and the covariance downdate P -= W1 W1^T (the P-GEMM).
//
//   immediate mode (default): every update launches its own P-GEMM behind its gain kernel.
//   deferred mode (cslam_ekf_set_deferred, and always inside a sequential update): the covariance is held as
//     P = Ps - Wp Wp^T with up to kmax columns of W1 panels (and the rank-1 columns of heading observations) pending;
//     readers of P correct for them, ONE P-GEMM applies them all.
//   two-stream mode (CSLAM_PIPELINE=1, an experiment that is NOT the default: measured slower): the
//     pending columns' P-GEMM runs on a second stream underneath the next update's factor / gain chain.  What makes it
//     legal is the pose stripe Pv (ekf_kernels.hpp p_get): predicts and heading observations never touch Ps.
// Nothing returns to the host unless the caller asks (get_x / get_state / sync mode).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "cslam_common.hpp"
#include "device_owners.hpp"
#include "ekf_kernels.hpp"
#include "ekf_kernels_fast.hpp"
#include "ekf_assoc_deferred_kernels.hpp"
#include "ekf_augment_kernels.hpp"
#include "ekf_counted_kernels.hpp"
#include "ekf_landmark_kernels.hpp"
#include "ekf_lookahead.hpp"
#include "ekf_options.hpp"
#include "ekf_pending_store.hpp"
#include "ekf_pgemm_limbs.hpp"
#include "ekf_pgemm_tiles.hpp"
#include "ekf_pose_kernels.hpp"
#define CSLAM_SCORE_SINGLE_ONLY // (the batch score kernels belong to cslam_ekf_batch.hip)
#include "ekf_score_kernels.hpp"
#include "ekf_staging.hpp"
#include "host_linalg.hpp"
#include "pf_host_parts.hpp"

namespace cslam
{
// the chain's go-ahead as a kernel of its own (only when the P-GEMM launch that should carry it did not happen)
__global__ void ekf_la_signal_kernel(unsigned* signal, unsigned add)
{
    if (threadIdx.x == 0)
    {
        atomicAdd(signal, add);
    }
}
// the snapshot job a wide launch may carry (LaSnapJob): the host adds ONE workgroup to the grid for it, the last one.  It
// copies 3 m words with plain vector loads and stores and leaves; no other workgroup looks at the job, and this one neither
// polls for the chain nor touches a row, so the wide kernel's own critical path is what it was.
__device__ __forceinline__ bool la_wide_snapshot(const LaSnapJob& j)
{
    if (j.Z == nullptr || blockIdx.x + 1 != gridDim.x)
    {
        return false;
    }
    for (int i = threadIdx.x; i < 3 * j.m; i += 128)
    {
        if (i < 2 * j.m)
        {
            j.Z_out[i] = j.Z[i];
        }
        else
        {
            j.idf_out[i - 2 * j.m] = j.idf[i - 2 * j.m];
        }
    }
    return true;
}
// the wide half of a look-ahead window (ekf_lookahead.hpp: ekf_la_wide_body), one filter
__global__ void __launch_bounds__(128) ekf_la_wide_f32(LaWideArgs a)
{
    if (la_wide_snapshot(a.snap))
    {
        return;
    }
    ekf_la_wide_body<1, 0>(a);
}
// ... with both updates of m = 32 observations (k = 64 known at compile time)
__global__ void __launch_bounds__(128) ekf_la_wide_f32_k64(LaWideArgs a)
{
    if (la_wide_snapshot(a.snap))
    {
        return;
    }
    ekf_la_wide_body<1, 64>(a);
}

// ... and the same kernel leaving the row-major mirror WT of both panels behind (ekf_la_wide_body: MIRROR)
__global__ void __launch_bounds__(128) ekf_la_wide_f32_k64m(LaWideArgs a, float* WT)
{
    if (la_wide_snapshot(a.snap))
    {
        return;
    }
    ekf_la_wide_body<1, 64, 1>(a, WT);
}

// the blocks kernel that reads the panel rows from that mirror and needs no rows kernel (ekf_la_blocks_mirror_body);
// the grid of ekf_la_blocks_kernel, 256 threads
__global__ void __launch_bounds__(256) ekf_la_blocks_mirror_kernel(LaPrepArgs<float> a, LaMirrorArgs mi)
{
    ekf_la_blocks_mirror_body(a, mi);
}
} // namespace cslam

using namespace cslam;

namespace
{

// Live engines of this process.  The look-ahead windows' fast hand-overs are waits INSIDE kernels (the chain kernel is
// launched early and waits for the blocks kernel; the wide kernel polls the chain's completion word).  They are only safe
// while the two streams of ONE engine have the device to themselves: with several engines, streams share the few hardware
// queues (a chain kernel spinning at the head of a queue blocks the kernel it waits for when that one sits behind another
// engine's waiting kernel in a second queue) and spinning wide kernels can hold every compute unit -- measured as 0.2 s
// time-outs with 8 co-running instances.  So with more than one engine alive: windows only if forced
// (CSLAM_LOOKAHEAD=1), and then with stream events only (ev_raw / ev_fb): a plain dependency graph, no waiting kernels.
std::atomic<int>& g_engines = ::cslam::live_engines();

constexpr size_t kLdsBudget    = 150 * 1024; // of the 160 KiB per CU, leave room for the small arrays

struct EkfBase
{
    explicit EkfBase(const EkfOptions& o) : opt(o) {}
    virtual ~EkfBase() {}
    const EkfOptions opt; // the engine switches, as the environment had them at cslam_ekf_create (ekf_options.hpp)
    int         dtype    = CSLAM_F32;
    int         device   = 0;
    int         quirks   = CSLAM_Q_REF_EXACT;
    int         nmax     = 0; // max landmarks
    int         ncap     = 0; // 3 + 2*nmax
    int         ldp      = 0; // padded leading dimension / column count
    int         n        = 3;
    int         sync_mode = 1;
    int         pgemm_wgs     = 0;  // > 0: cap on the persistent P-GEMM grid (cslam_ekf_set_pgemm_workgroups: co-running instances)
    int         split_whole = 0, split_strips = 0; // whole tiles and strips of the last psym4 launch (cslam_ekf_pgemm_split)
    // (the owners live in the base, so they are destroyed after every buffer and event of Ekf<T>)
    Stream      stream_own, stream_b_own, stream_f_own;
    hipStream_t stream   = nullptr; // A: everything except the P-GEMM (= stream_own.get())
    hipStream_t stream_b = nullptr; // B: the P-GEMM (== stream when not pipelined, else stream_b_own.get())
    long long   la_windows = 0;     // look-ahead windows launched (cslam_ekf_lookahead_windows)
    long long   stage_launches = 0; // ekf_stage_obs_kernel launches (cslam_ekf_stage_launches)
    long long   rows_launches = 0;  // ekf_la_rows_kernel launches (cslam_ekf_rows_launches)
    long long   augment_launches = 0; // ekf_augment_kernel + ekf_augment_many_kernel launches (cslam_ekf_augment_launches)

    virtual int init()                                                                        = 0;
    virtual int set_state(const void* X, int n, const void* P, int ldp)                        = 0;
    virtual int get_state(void* X, void* P, int ldp)                                           = 0;
    virtual int get_x(void* X, int cap)                                                        = 0;
    virtual int get_landmarks(int first, int count, void* x, void* pll, void* pvl)             = 0;
    virtual int trace(double* tr)                                                              = 0;
    virtual int get_pose(void* x, void* pvv)                                                   = 0;
    // the score kept on the device (ekf_score_kernels.hpp)
    virtual int score_reset(int series_capacity, double gate_pose, double gate_lm)             = 0;
    virtual int score_set_truth(const double* lm_true, int count)                              = 0;
    virtual int score(const double* xv_true, int with_map)                                     = 0;
    virtual int get_scores(double* totals, float* series, double* track, int capacity_records, int* records,
                           long long* calls)                                                   = 0;
    virtual int predict(double v, double swa, const void* Q, double wb, double dt)             = 0;
    virtual int update(const void* Z, int m, const void* R, const int* idf, int batch, bool on_device) = 0;
    virtual int augment(const void* Z, int q, const void* R)                                   = 0;
    virtual int augment_device(const void* dZ, int q, const void* R)                           = 0;
    virtual int observe_heading(double phi, int use)                                           = 0;
    virtual int associate(const void* Z, int m, const void* R, double g1, double g2, int* idf_out, int* kind) = 0;
    virtual int update_counted(const void* dZ, int m_cap, const void* R, const int* d_idf, const int* d_count,
                               int batch)                                                      = 0;
    virtual int associate_deferred(const void* Z, int m, const void* R, double g1, double g2, int* idf_out, int* kind,
                                   int* counts)                                                = 0;
    virtual int associate_deferred_async(const void* Z, int m, const void* R, double g1, double g2) = 0;
    virtual int association_wait(int* idf_out, int* kind, int* counts)                         = 0;
    virtual int association_device_ptrs(const void** dZF, const int** d_idf, const void** dZN,
                                        const int** d_counts)                                  = 0;
    virtual int factor_status(int* flags, int clear)                                           = 0;
    virtual int set_profiling(int on)                                                          = 0;
    virtual int get_stage_times(double* ms, int* launches)                                     = 0;
    virtual int debug_last_update(void* PHT, void* S, void* G, void* W1, void* V, int* k)      = 0;
    virtual int set_deferred(int max_cols)                                                     = 0;
    virtual int do_flush()                                                                     = 0;
    virtual int resolve_predict()                                                              = 0;
    virtual int sync_all()                                                                     = 0;
    virtual int la_drain()                                                                     = 0;
};

template <typename T>
struct Ekf : EkfBase
{
    using EkfBase::EkfBase;
    DevBuf<T>   dX, dP;
    DevBuf<T>   dPv;       // pose stripe: columns 0..2 of P (always current; see p_get in ekf_kernels.hpp)
    DevBuf<int> dPoseDone; // ticket counters: [0] ekf_pose_step_kernel, [1] ekf_pose_downdate_kernel
    DevBuf<int> dSign;     // per region: wcap column signs (heading columns with S < 0), then [2*wcap + r] their count
    DevBuf<T>   dLm;       // landmark read outputs: 12 scalars per landmark of capacity (allocated by the first read)
    PendingCols pend;    // the pending W1 store's bookkeeping (ekf_pending_store.hpp); its buffers are dW1 and dSign
    Event      ev_a2b, ev_pgemm;
    T*         last_slot = nullptr; // W1 of the last update
    // update workspace for batches of up to kcap rows of H: one set, replaced as a whole by ensure_k
    struct Workspace
    {
        DevBuf<T> dPHT, dS, dG, dGt, dV, dt_, dScrS, dScrG;
        DevBuf<T> dSub; // (3 + 64) x 64 compact block of PHT (see ekf_gather_kernel)
        DevBuf<T> dM;   // 3 x 64: M = G G^T PHT[0:3,:]^T from ekf_factor_mfma_f32 (pose-stripe downdate in the gain kernel)
        DevBuf<T> dU;   // u = G*(G^T V), the gain kernel's X update vector
        DevBuf<T> dWv;  // pose rows of the last update's W1 (3 x kcap), saved by the pose downdate before it zeroes them
        DevBuf<T> dY;   // Y = H*Wp (kcap x wcap), correction of PHT under pending panels (ensure_w replaces it alone)

        int alloc(int ldp, int newk, int wcap, hipStream_t st)
        {
            const size_t kk = (size_t)newk * (newk + 1);
            int          rc = dPHT.alloc_zeroed((size_t)ldp * newk, st);
            if (rc || (rc = dS.alloc(kk)) || (rc = dG.alloc(kk)) || (rc = dSub.alloc((size_t)(3 + 64) * 64)) ||
                (rc = dM.alloc((size_t)3 * 128)) || (rc = dGt.alloc(kk)) || (rc = dScrS.alloc(kk)) ||
                (rc = dScrG.alloc(kk)) || (rc = dV.alloc((size_t)newk)) || (rc = dt_.alloc((size_t)newk)) ||
                (rc = dU.alloc((size_t)newk)) || (rc = dWv.alloc_zeroed((size_t)3 * newk, st)) || (wcap > 0 &&
                (rc = dY.alloc((size_t)newk * wcap))))
            {
                return rc;
            }
            return CSLAM_OK;
        }
    };
    Workspace ws;
    int       kcap = 0;
    DevBuf<T> dW1;      // pending W1 panels, two regions of ldp x pend.wcap
    int       defer_max = 0; // > 0: keep up to this many pending columns across calls (cslam_ekf_set_deferred)
    bool m_valid = false; // the last factor launch produced dM
    bool g_from_gt  = false; // the last factor launch wrote only G^T (ekf_factor_mfma_f32): debug transposes it
    bool sub_valid = false;
    DevBuf<int>    dFlags; // [0] sticky, [1] last
    PinnedBuf<int> hFlags; // pinned mirror
    // heading scratch: w, cp2, rrow (ldp each) + 2 scalars
    DevBuf<T> dHead;
    StageRing<T> ring; // observation staging (ekf_staging.hpp)
    // tile list of the persistent symmetric downdate
    DevBuf<int> dTicket; // two tile-ticket counters used alternately by successive P-GEMM launches
    // the limb store of the bf16-limb P-GEMM (opt.pgemm_limbs) and its size
    DevBuf<uint4> dWb;
    size_t        wb_bytes = 0;
    DevBuf<int2>  dTilesM;  // the tile list in Morton order, cut into eight segments (one per XCD) ...
    DevBuf<int>   dSegOff;  // ... at these offsets (9), and two sets of eight ticket counters
    DevBuf<int>   dTicketX;
    int        tilesM_built = 0;
    int        limb_parity = 0;
    unsigned   launch_parity = 0;
    DevBuf<int2> dTiles;
    int   tiles_built = 0;
    int   n_sym_tiles = 0;
    // the work lists of ekf_downdate_psym4_f32 with its tail phase (ekf_pgemm_tiles.hpp), one per chunk class: whole
    // tiles, then strips.  Built by ensure_tile_list for (tile rows, valid strips of the last tile row, grid); a class
    // without strips uses dTiles.
    DevBuf<int2> dWork[3];
    int   work_whole[3] = {0, 0, 0}, work_strips[3] = {0, 0, 0};
    int   work_tiles = 0, work_valid = 0, work_grid = 0;
    int   num_cus     = 256;
    // status
    int sticky_host = 0; // flags raised by host-side decisions (FALLBACK/SKIPPED)
    int last_k      = 0;
    int kp_call_limit = 0; // pending columns a sequential update() may accumulate within the call
    StageProfiler prof; // ekf_staging.hpp

    ~Ekf() override
    {
        (void)hipSetDevice(device);
        (void)la_launch_held_wide(nullptr); // (its chain kernel has run: the window ends as every other one does)
        if (stream)
        {
            (void)hipStreamSynchronize(stream);
        }
        if (stream_b && stream_b != stream)
        {
            (void)hipStreamSynchronize(stream_b);
        }
        if (stream_f)
        {
            (void)hipStreamSynchronize(stream_f);
        }
    }

    T* wbase(int region) const { return dW1.get() + (size_t)region * pend.wcap * ldp; }
    int* signs(int region) const { return dSign.get() + (size_t)region * pend.wcap; }
    int* sign_count(int region) const { return dSign.get() + (size_t)2 * pend.wcap + region; }

    int use_device() { CSLAM_HIP_TRY(hipSetDevice(device)); return CSLAM_OK; }

    int init() override
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if (opt.pipeline)
        {
            // the chain (A) outranks the P-GEMM (B): its small kernels must get in while the P-GEMM fills the chip
            int lo = 0, hi = 0;
            CSLAM_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
            if ((rc = stream_own.create_with_priority(hipStreamNonBlocking, hi)) ||
                (rc = stream_b_own.create_with_priority(hipStreamNonBlocking, lo)))
            {
                return rc;
            }
            stream   = stream_own.get();
            stream_b = stream_b_own.get();
        }
        else
        {
            CSLAM_TRY(stream_own.create(hipStreamNonBlocking));
            stream = stream_b = stream_own.get();
        }
        if ((rc = ev_a2b.create(hipEventDisableTiming)) || (rc = ev_pgemm.create(hipEventDisableTiming)))
        {
            return rc;
        }
        {
            hipDeviceProp_t prop;
            CSLAM_HIP_TRY(hipGetDeviceProperties(&prop, device));
            num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        }
        if ((rc = dX.alloc_zeroed((size_t)ldp, stream)) || (rc = dP.alloc_zeroed((size_t)ldp * ldp, stream)) ||
            (rc = dPv.alloc_zeroed((size_t)3 * ldp, stream)) || (rc = dPoseDone.alloc_zeroed(4, stream)) ||
            (rc = dFlags.alloc_zeroed(2, stream)) || (rc = hFlags.alloc(2)) ||
            (rc = dHead.alloc_zeroed((size_t)3 * ldp + 2, stream)))
        {
            return rc;
        }
        // allow the factor kernel its large dynamic LDS
        CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_factor_kernel<T>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (sizeof(T) == 4)
        {
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_factor_mfma_big_f32<128>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_factor_mfma_big_f32_counted<128>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        }
        else
        {
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_factor_mfma_f64_counted<64>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_factor_mfma_f64_counted<32>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_factor_mfma_f64<64>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_factor_mfma_f64<32>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_downdate_f64<4>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_downdate_f64<2>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        }
        CSLAM_TRY(dTicket.alloc_zeroed(2, stream));
        rc = ensure_k(64);
        if (rc)
        {
            return rc;
        }
        rc = ensure_w(128);
        if (rc)
        {
            return rc;
        }
        rc = ensure_m(64);
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // workspace for batches of up to k rows of H
    int ensure_k(int k)
    {
        if (k <= kcap)
        {
            return CSLAM_OK;
        }
        int newk = round_up(std::max(k, 2 * kcap), 8);
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        Workspace nw;
        CSLAM_TRY(nw.alloc(ldp, newk, pend.wcap, stream));
        ws   = std::move(nw);
        kcap = newk;
        return CSLAM_OK;
    }

    // room for `cols` pending columns per region; applies what is pending first when the buffer has to move
    int ensure_w(int cols)
    {
        cols = round_up(cols, 8);
        if (cols <= pend.wcap)
        {
            return CSLAM_OK;
        }
        int rc = flush();
        if (rc || (rc = sync_all()))
        {
            return rc;
        }
        int neww = round_up(std::max(cols, 2 * pend.wcap), 8);
        DevBuf<T>   w1, y;
        DevBuf<int> sign;
        if ((rc = w1.alloc_zeroed((size_t)2 * ldp * neww, stream)) || (rc = y.alloc((size_t)std::max(kcap, 8) * neww)) ||
            (rc = sign.alloc_zeroed((size_t)2 * neww + 2, stream)))
        {
            return rc;
        }
        dW1   = std::move(w1);
        ws.dY = std::move(y);
        dSign = std::move(sign);
        pend.regrown(neww);
        last_slot = nullptr;
        return CSLAM_OK;
    }

    int sync_all() override
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        if (stream_b != stream)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream_b));
        }
        if (stream_f)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream_f));
        }
        pend.waited();
        return CSLAM_OK;
    }

    // stream A waits until every P-GEMM launched so far (stream B) has completed: needed before anything reads or
    // writes Ps, or writes a W1 region such a P-GEMM reads
    int wait_pgemm()
    {
        if (pend.in_flight() && stream_b != stream)
        {
            CSLAM_HIP_TRY(hipStreamWaitEvent(stream, ev_pgemm.get(), 0));
        }
        pend.waited();
        return CSLAM_OK;
    }

    // before stream A writes into W1 region r
    int own_region(int r)
    {
        return pend.in_flight(r) ? wait_pgemm() : CSLAM_OK;
    }

    // launch the P-GEMM of every pending column (slam.h:260 is linear in the panels: ONE pass with k = kp) on stream B,
    // ordered behind everything enqueued on stream A so far; the pending store moves on to the other region
    int flush()
    {
        int rc = launch_pose_queue(); // queued heading steps write pending columns of this region
        if (rc)
        {
            return rc;
        }
        if (pend.kp == 0)
        {
            return CSLAM_OK;
        }
        if ((rc = use_device()))
        {
            return rc;
        }
        T*        W   = wbase(pend.wcur);
        const int kp8 = round_up(pend.kp, 8);
        // (the shipped f32 P-GEMM bounds its W1 buffer resource at kp columns: the hardware returns zeros beyond, no
        // padding needed; the other kernels read whole blocks of 8 columns)
        if (kp8 > pend.kp && !psym4_takes(kp8))
        {
            CSLAM_HIP_TRY(hipMemset2DAsync(W + (size_t)pend.kp * ldp, (size_t)ldp * sizeof(T), 0,
                                           (size_t)round_up(n, kTile) * sizeof(T), (size_t)(kp8 - pend.kp), stream));
        }
        if (stream_b != stream)
        {
            CSLAM_HIP_TRY(hipEventRecord(ev_a2b.get(), stream));
            CSLAM_HIP_TRY(hipStreamWaitEvent(stream_b, ev_a2b.get(), 0));
        }
        if (pend.hd_cols[pend.wcur] > 0) // exceptional heading columns (S < 0) enter with the opposite sign: exits at once otherwise
        {
            if ((rc = launch_negcol_fix(W, pend.kp, stream_b)))
            {
                return rc;
            }
        }
        if ((rc = prof.begin(CSLAM_STAGE_DOWNDATE, stream_b)) || (rc = launch_downdate(W, pend.kp, stream_b)) ||
            (rc = prof.end(CSLAM_STAGE_DOWNDATE, stream_b)))
        {
            return rc;
        }
        if (stream_b != stream)
        {
            CSLAM_HIP_TRY(hipEventRecord(ev_pgemm.get(), stream_b));
            pend.pgemm_on_second_stream();
        }
        const bool clear_signs = pend.applied(); // its column signs belong to columns that have been applied
        // the other region becomes the pending store: a still older P-GEMM may be reading it
        if ((rc = own_region(pend.wcur)))
        {
            return rc;
        }
        if (clear_signs && stream_b != stream) // (single stream: ekf_negcol_fix_kernel clears them itself when it had work)
        {
            CSLAM_HIP_TRY(hipMemsetAsync(signs(pend.wcur), 0, (size_t)pend.wcap * sizeof(int), stream));
            CSLAM_HIP_TRY(hipMemsetAsync(sign_count(pend.wcur), 0, sizeof(int), stream));
        }
        return CSLAM_OK;
    }

    // the tile list in Morton order, cut into eight equal segments (one per XCD), and the 2 x 8 ticket counters
    int ensure_tiles_morton(int tiles, hipStream_t stream)
    {
        if (tilesM_built == tiles)
        {
            return CSLAM_OK;
        }

        // Morton order over the lower triangle, eight equal segments
        auto spread = [](unsigned v) {
            v &= 0xFFFF;
            v = (v | (v << 8)) & 0x00FF00FF;
            v = (v | (v << 4)) & 0x0F0F0F0F;
            v = (v | (v << 2)) & 0x33333333;
            v = (v | (v << 1)) & 0x55555555;
            return v;
        };
        std::vector<std::pair<unsigned, int2>> keyed;
        keyed.reserve((size_t)tiles * (tiles + 1) / 2);
        for (int tj = 0; tj < tiles; tj++)
        {
            for (int ti = tj; ti < tiles; ti++)
            {
                keyed.push_back({spread((unsigned)ti) | (spread((unsigned)tj) << 1), make_int2(ti, tj)});
            }
        }
        std::sort(keyed.begin(), keyed.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        std::vector<int2> hl(keyed.size());
        for (size_t i = 0; i < keyed.size(); i++)
        {
            hl[i] = keyed[i].second;
        }
        int off[9];
        for (int sgi = 0; sgi <= 8; sgi++)
        {
            off[sgi] = (int)((size_t)hl.size() * sgi / 8);
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        DevBuf<int2> list;
        DevBuf<int>  seg, ticket;
        int          rc = list.alloc(hl.size());
        if (rc || (!dSegOff.get() && ((rc = seg.alloc(9)) || (rc = ticket.alloc_zeroed_blocking(16)))))
        {
            return rc;
        }
        dTilesM = std::move(list);
        if (!dSegOff.get())
        {
            dSegOff  = std::move(seg);
            dTicketX = std::move(ticket);
        }
        CSLAM_HIP_TRY(hipMemcpy(dTilesM.get(), hl.data(), hl.size() * sizeof(int2), hipMemcpyHostToDevice));
        CSLAM_HIP_TRY(hipMemcpy(dSegOff.get(), off, sizeof(off), hipMemcpyHostToDevice));
        tilesM_built = tiles;
        return CSLAM_OK;
    }

    // k8 columns go through ekf_downdate_psym4_f32 (see launch_downdate)
    bool psym4_takes(int k8) const
    {
        return sizeof(T) == 4 && (k8 <= 128 || limbs_take(k8)) && opt.lower && ldp < 32768;
    }
    // ... or through ekf_downdate_psym5_bf16 (which pads its own limb store)
    bool limbs_take(int k8) const
    {
        return sizeof(T) == 4 && opt.pgemm_limbs > 0 && k8 >= opt.limbs_kmin && k8 <= 256 && opt.lower && ldp < 32768;
    }

    int launch_negcol_fix(T* W, int kcols, hipStream_t st)
    {
        const int tiles = round_up(n, kTile) / kTile;
        int       rc    = CSLAM_OK;
        if (opt.lower && (rc = ensure_tile_list(tiles)))
        {
            return rc;
        }
        const int nt = opt.lower ? n_sym_tiles : tiles * tiles;
        hipLaunchKernelGGL(ekf_negcol_fix_kernel<T>, dim3(std::min(nt, 2 * num_cus)), dim3(256), 0, st, dP.get(), ldp,
                           n, W, ldp, kcols, signs(pend.wcur), sign_count(pend.wcur),
                           opt.lower ? dTiles.get() : (const int2*)nullptr, nt, tiles, dPoseDone.get() + 2,
                           (stream_b == stream) ? 1 : 0);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    // everything applied and Ps quiescent as far as stream A is concerned
    int flush_wait()
    {
        int rc = flush();
        return rc ? rc : wait_pgemm();
    }

    // room in the staging ring for m observations per slot
    int ensure_m(int m)
    {
        if (m <= ring.mcap)
        {
            return CSLAM_OK;
        }
        if (int rc = la_drain()) // (queued updates read the ring that is about to move)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        if (stream_f)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream_f));
        }
        return ring.grow(m);
    }

    // copies (Z, idf) of one call into the next slot of the ring on the main stream; returns device pointers
    int stage_obs(const void* Z, const int* idf, int m, bool on_device, const T** dZ, const int** dIdf)
    {
        int rc = ensure_m(m);
        return rc ? rc : ring.stage(Z, idf, m, on_device, stream, stage_launches, dZ, dIdf);
    }

    // ---------------------------------------------------------------- state transfer
    int set_state(const void* X, int nn, const void* P, int ldph) override
    {
        if (!X || !P || nn < 3 || nn > ncap || ((nn - 3) & 1) || ldph < nn)
        {
            return fail(CSLAM_ERR_BAD_ARG, "set_state: bad n=%d (cap %d) or ldp=%d", nn, ncap, ldph);
        }
        int rc = sync_all();
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(dX.get(), X, (size_t)nn * sizeof(T), hipMemcpyHostToDevice, stream));
        CSLAM_HIP_TRY(hipMemcpy2DAsync(dP.get(), (size_t)ldp * sizeof(T), P, (size_t)ldph * sizeof(T),
                                       (size_t)nn * sizeof(T), (size_t)nn, hipMemcpyHostToDevice, stream));
        // the pose stripe = columns 0..2 of P (contiguous in the column-major buffer)
        CSLAM_HIP_TRY(hipMemcpyAsync(dPv.get(), dP.get(), (size_t)3 * ldp * sizeof(T), hipMemcpyDeviceToDevice,
                                     stream));
        // panels: rows beyond the new n must read as zero (the tuned gain kernel relies on it)
        pend.discarded(); // a new state discards updates that were never applied
        last_slot = nullptr;
        CSLAM_HIP_TRY(hipMemsetAsync(dSign.get(), 0, ((size_t)2 * pend.wcap + 2) * sizeof(int), stream));
        CSLAM_HIP_TRY(hipMemsetAsync(ws.dPHT.get(), 0, (size_t)ldp * kcap * sizeof(T), stream));
        CSLAM_HIP_TRY(hipMemsetAsync(dW1.get(), 0, (size_t)2 * ldp * pend.wcap * sizeof(T), stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        n = nn;
        return CSLAM_OK;
    }

    int get_state(void* X, void* P, int ldph) override
    {
        if (ldph < n && P)
        {
            return fail(CSLAM_ERR_BAD_ARG, "get_state: ldp=%d < n=%d", ldph, n);
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if (P && (rc = flush_wait()))
        {
            return rc;
        }
        if (X)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(X, dX.get(), (size_t)n * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        if (P)
        {
            if (opt.lower)
            {
                const int g = (n + 31) / 32;
                hipLaunchKernelGGL(ekf_mirror_upper_kernel<T>, dim3(g, g), dim3(256), 0, stream, dP.get(), ldp, n);
                CSLAM_HIP_TRY(hipGetLastError());
            }
            // rows / columns 0..2 of the buffer come from the pose stripe
            hipLaunchKernelGGL(ekf_patch_pose_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, stream, dP.get(),
                               dPv.get(), ldp, n);
            CSLAM_HIP_TRY(hipGetLastError());
            CSLAM_HIP_TRY(hipMemcpy2DAsync(P, (size_t)ldph * sizeof(T), dP.get(), (size_t)ldp * sizeof(T),
                                           (size_t)n * sizeof(T), (size_t)n, hipMemcpyDeviceToHost, stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int get_x(void* X, int cap) override
    {
        if (!X || cap < n)
        {
            return fail(CSLAM_ERR_BAD_ARG, "get_x: capacity %d < n=%d", cap, n);
        }
        return get_state(X, nullptr, 0);
    }

    // Landmarks first .. first + count - 1 (arguments checked by cslam_ekf_get_landmarks, queued work launched by
    // resolve_predict): P = Ps - Wp diag(s) Wp^T is read as it stands (ekf_landmark_kernels.hpp), so the pending columns
    // stay pending and every later result is the one the run would give without this read.  Two-stream mode: the read
    // is ORDERED behind the P-GEMMs in flight on stream B (they write Ps), as get_state is; it does not correct for them.
    int get_landmarks(int first, int count, void* x, void* pll, void* pvl) override
    {
        int rc = use_device();
        if (rc || (rc = wait_pgemm()))
        {
            return rc;
        }
        if (!dLm.get() && (rc = dLm.alloc((size_t)std::max(nmax, 1) * 12)))
        {
            return rc;
        }
        const size_t c  = (size_t)count;
        T*           ox = dLm.get(), *opll = dLm.get() + 2 * c, *opvl = dLm.get() + 6 * c;
        const int*   sg = (pend.kp > 0 && pend.hd_cols[pend.wcur] > 0) ? signs(pend.wcur) : (const int*)nullptr;
        hipLaunchKernelGGL(ekf_landmark_read_kernel<T>, dim3((count + 255) / 256), dim3(256), 0, stream, dX.get(),
                           dPv.get(), dP.get(), ldp, opt.lower, (const T*)wbase(pend.wcur), ldp, pend.kp, sg, first, count,
                           x ? ox : (T*)nullptr, pll ? opll : (T*)nullptr, pvl ? opvl : (T*)nullptr);
        CSLAM_HIP_TRY(hipGetLastError());
        if (x)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(x, ox, 2 * c * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        if (pll)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(pll, opll, 4 * c * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        if (pvl)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(pvl, opvl, 6 * c * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int trace(double* tr) override
    {
        if (!tr)
        {
            return fail(CSLAM_ERR_BAD_ARG, "trace: null");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if ((rc = flush_wait()))
        {
            return rc;
        }
        std::vector<T> diag((size_t)n);
        CSLAM_HIP_TRY(hipMemcpy2DAsync(diag.data(), sizeof(T), dP.get(), ((size_t)ldp + 1) * sizeof(T), sizeof(T),
                                       (size_t)n, hipMemcpyDeviceToHost, stream));
        // the pose block lives in the stripe
        CSLAM_HIP_TRY(hipMemcpy2DAsync(diag.data(), sizeof(T), dPv.get(), ((size_t)ldp + 1) * sizeof(T), sizeof(T),
                                       (size_t)3, hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        double s = 0.0;
        for (T d : diag)
        {
            s += (double)d;
        }
        *tr = s;
        return CSLAM_OK;
    }

    // The pose X[0:3] and the 3 x 3 pose block (arguments checked by cslam_ekf_get_pose, queued work launched by
    // resolve_predict).  Both are exact as they stand: the pending panels hold zeros in rows 0..2 and the block lives in
    // the stripe, P[r, c] = Pv[c ldp + r].  No flush, no P-GEMM, no copy of P: 12 scalars.
    int get_pose(void* x, void* pvv) override
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(x, dX.get(), 3 * sizeof(T), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipMemcpy2DAsync(pvv, 3 * sizeof(T), dPv.get(), (size_t)ldp * sizeof(T), 3 * sizeof(T), (size_t)3,
                                       hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // ---------------------------------------------------------------- the score, kept on the device
    // (ekf_score_kernels.hpp: ekf_score_landmarks / ekf_score_finish).  Two levels, each all-or-nothing, as the particle
    // handle's: the base (totals, the landmark kernel's slots and the truth rows, sized for max_landmarks once, by the
    // first score call or score_reset) and the log (series and track, sized by the largest series_capacity a reset has
    // asked for).  A handle that never scores allocates neither; set_state leaves both alone.  The book is the particle
    // handle's (pf_host_parts.hpp) with the estimator left at 0: the same argument rules, gate defaults and record count.
    struct ScoreBufs
    {
        struct Base
        {
            DevBuf<double> totals; // [CSLAM_SCORE_FIELDS]
            DevBuf<double> parts;  // [blocks(max_landmarks)][kScorePartsSingle]
            DevBuf<double> truth;  // [max_landmarks][2]
        };
        struct Log
        {
            DevBuf<float>  series; // [capacity][4]
            DevBuf<double> track;  // [capacity][kScoreTrack]
        };
        Base        base;
        Log         log;
        PfScoreBook book;
        bool        allocated() const { return (bool)base.totals; }
    };
    ScoreBufs sc;

    int ensure_score()
    {
        if (sc.allocated())
        {
            return CSLAM_OK;
        }
        const size_t             cf = (size_t)std::max(nmax, 1);
        typename ScoreBufs::Base b;
        CSLAM_TRY(b.totals.alloc_zeroed((size_t)CSLAM_SCORE_FIELDS, stream));
        CSLAM_TRY(b.parts.alloc((size_t)PfScoreBook::blocks((int)cf) * kScorePartsSingle));
        CSLAM_TRY(b.truth.alloc(2 * cf));
        sc.base = std::move(b);
        return CSLAM_OK;
    }

    int score_reset(int series_capacity, double gate_pose, double gate_lm) override
    {
        if (!PfScoreBook::reset_args_ok(0, series_capacity))
        {
            return fail(CSLAM_ERR_BAD_ARG, "ekf_score_reset: series_capacity %d (>= 0)", series_capacity);
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(ensure_score());
        if (!PfScoreBook::series_fits(sc.log.series.count() / 4, series_capacity))
        {
            typename ScoreBufs::Log l;
            CSLAM_TRY(l.series.alloc((size_t)series_capacity * 4));
            CSLAM_TRY(l.track.alloc((size_t)series_capacity * kScoreTrack));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still writes the old log
            sc.log = std::move(l);
        }
        CSLAM_HIP_TRY(hipMemsetAsync(sc.base.totals.get(), 0, CSLAM_SCORE_FIELDS * sizeof(double), stream));
        if (sc.log.series)
        {
            CSLAM_HIP_TRY(hipMemsetAsync(sc.log.series.get(), 0, sc.log.series.count() * sizeof(float), stream));
            CSLAM_HIP_TRY(hipMemsetAsync(sc.log.track.get(), 0, sc.log.track.count() * sizeof(double), stream));
        }
        sc.book.reset(0, series_capacity, gate_pose, gate_lm);
        return CSLAM_OK;
    }

    int score_set_truth(const double* lm_true, int count) override
    {
        if (!PfScoreBook::truth_args_ok(count, nmax) || (count > 0 && !lm_true))
        {
            return fail(CSLAM_ERR_BAD_ARG, "ekf_score_set_truth: count %d outside 0..max_landmarks=%d, or null rows", count, nmax);
        }
        CSLAM_TRY(use_device());
        CSLAM_TRY(ensure_score());
        if (count > 0)
        {
            // (behind whatever score call still reads the old rows; the host array is consumed before the return)
            CSLAM_HIP_TRY(hipMemcpyAsync(sc.base.truth.get(), lm_true, (size_t)2 * count * sizeof(double),
                                         hipMemcpyHostToDevice, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        }
        sc.book.set_truth_count(count);
        return CSLAM_OK;
    }

    // One score step (xv_true checked by cslam_ekf_score, queued work launched by resolve_predict).  What get_landmarks
    // does before its kernel, then the two kernels on the main stream: no flush, no synchronise, no copy, and after the
    // first call no allocation.  The pending columns stay pending, so the run continues bit for bit as without the call.
    int score(const double* xv_true, int with_map) override
    {
        int rc = use_device();
        if (rc || (rc = ensure_score()) || (rc = wait_pgemm()))
        {
            return rc;
        }
        const PfScoreBook& bk     = sc.book;
        const int          nl     = (n - 3) / 2;
        const int          blocks = with_map ? PfScoreBook::blocks(nl) : 0;
        if (blocks > 0)
        {
            const int* sg = (pend.kp > 0 && pend.hd_cols[pend.wcur] > 0) ? signs(pend.wcur) : (const int*)nullptr;
            hipLaunchKernelGGL(ekf_score_landmarks<T>, dim3(blocks), dim3(256), 0, stream, (const T*)dX.get(),
                               (const T*)dPv.get(), (const T*)dP.get(), ldp, opt.lower, (const T*)wbase(pend.wcur), pend.kp, sg,
                               nl, bk.scored(nl, 1), (const double*)sc.base.truth.get(), bk.gate_lm(), sc.base.parts.get());
            CSLAM_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(ekf_score_finish<T>, dim3(1), dim3(64), 0, stream, (const T*)dX.get(), (const T*)dPv.get(), ldp, n,
                           (const double*)sc.base.parts.get(), blocks, with_map ? 1 : 0, xv_true[0], xv_true[1], xv_true[2],
                           bk.gate_pose(), sc.base.totals.get(), sc.log.series.get(), sc.log.track.get(), bk.next_record());
        CSLAM_HIP_TRY(hipGetLastError());
        sc.book.called();
        return CSLAM_OK;
    }

    // The one synchronising call of the score: copies on the main stream and waits for it.  Nothing is flushed and
    // nothing queued is launched (a held predict, the pose queue and a queued look-ahead update stay as they are), so
    // the rest of the run does not depend on where the scores are read.
    int get_scores(double* totals, float* series, double* track, int capacity_records, int* records, long long* calls) override
    {
        if (capacity_records < 0)
        {
            return fail(CSLAM_ERR_BAD_ARG, "ekf_get_scores: capacity_records %d", capacity_records);
        }
        CSLAM_TRY(use_device());
        const PfScoreBook& bk = sc.book;
        const size_t       c  = (size_t)bk.records_to_copy(capacity_records);
        if (totals && !sc.allocated())
        {
            std::fill(totals, totals + CSLAM_SCORE_FIELDS, 0.0);
        }
        else if (totals)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(totals, sc.base.totals.get(), CSLAM_SCORE_FIELDS * sizeof(double),
                                         hipMemcpyDeviceToHost, stream));
        }
        if (series && c > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(series, sc.log.series.get(), c * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
        }
        if (track && c > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(track, sc.log.track.get(), c * kScoreTrack * sizeof(double), hipMemcpyDeviceToHost,
                                         stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        if (records)
        {
            *records = bk.records();
        }
        if (calls)
        {
            *calls = bk.calls();
        }
        return CSLAM_OK;
    }

    // ---------------------------------------------------------------- profiling (StageProfiler, ekf_staging.hpp)
    int set_profiling(int on) override
    {
        if (int rc = la_drain())
        {
            return rc;
        }
        if (int rc = sync_all())
        {
            return rc;
        }
        prof.set_mode(on);
        return CSLAM_OK;
    }
    int get_stage_times(double* ms, int* launches) override
    {
        if (!ms || !launches)
        {
            return fail(CSLAM_ERR_BAD_ARG, "get_stage_times: null");
        }
        if (int rc = la_drain())
        {
            return rc;
        }
        if (int rc = sync_all())
        {
            return rc;
        }
        return prof.times(ms, launches);
    }

    // ---------------------------------------------------------------- data association (EKF.cpp:131-144, 235-326)
    DevBuf<T>   dAssoc; // 8 scalars per feature
    int         assoc_cap = 0;
    DevBuf<int> dAssocOut; // idf[m], kind[m]
    int         assoc_mcap = 0;
    int associate(const void* Zv, int m, const void* Rv, double g1, double g2, int* idf_out, int* kind_out) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Zv || !idf_out || !kind_out)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "associate: bad arguments (m=%d)", m);
        }
        if (m == 0)
        {
            return CSLAM_OK;
        }
        int rc = use_device();
        if (rc || (rc = flush_wait()))
        {
            return rc;
        }
        const int nf = (n - 3) / 2;
        if (nf > assoc_cap)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            DevBuf<T> grown;
            CSLAM_TRY(grown.alloc((size_t)std::max(nf, 1) * 8));
            dAssoc    = std::move(grown);
            assoc_cap = nf;
        }
        if (m > assoc_mcap)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            DevBuf<int> grown;
            CSLAM_TRY(grown.alloc((size_t)2 * m));
            dAssocOut  = std::move(grown);
            assoc_mcap = m;
        }
        const T* R  = static_cast<const T*>(Rv);
        const T* dZ = nullptr;
        const int* dummy = nullptr;
        std::vector<int> zero_idf((size_t)m, 1);
        if ((rc = stage_obs(Zv, zero_idf.data(), m, false, &dZ, &dummy)))
        {
            return rc;
        }
        if (nf > 0)
        {
            hipLaunchKernelGGL(ekf_assoc_feature_kernel<T>, dim3((nf + 255) / 256), dim3(256), 0, stream, dX.get(),
                               dP.get(), dPv.get(), ldp, n, R[0], R[1], R[2], R[3], opt.lower, dAssoc.get());
            CSLAM_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(ekf_assoc_scan_kernel<T>, dim3(m), dim3(64), 0, stream, dAssoc.get(), nf, dZ, m, (T)g1,
                           (T)g2, dAssocOut.get(), dAssocOut.get() + m);
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipMemcpyAsync(idf_out, dAssocOut.get(), (size_t)m * sizeof(int), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipMemcpyAsync(kind_out, dAssocOut.get() + m, (size_t)m * sizeof(int), hipMemcpyDeviceToHost,
                                     stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // The same answer read from the deferred form P = Ps - Wp diag(s) Wp^T as it stands (ekf_assoc_deferred_kernels.hpp):
    // no flush, so pend.kp, the pending region, the sign words and P are what they were (arguments checked by
    // cslam_ekf_associate_deferred, queued work launched by resolve_predict).  Two-stream mode: ordered behind the P-GEMMs
    // in flight, as get_landmarks is.  One buffer set, replaced as a whole when m or the workgroup count outgrows it:
    //   dAdT  Z (2 M) | ZF (2 M) | ZN (2 M) | pnd (M G) | pnis (M G)
    //   dAdI  counts (4) | idf (M) | kind (M) | idf_f (M) | pj (M G)     -- of which counts | idf[m] | kind[m] are written
    //         contiguously for the m of the call, so that ONE copy into the pinned hAd brings the host results back
    DevBuf<T>      dAdT;
    DevBuf<int>    dAdI;
    PinnedBuf<int> hAd;  // counts (4) | idf (M) | kind (M)
    PinnedBuf<T>   hAdZ; // staging of Z (2 M)
    int            ad_mcap = 0, ad_gcap = 0;
    bool           ad_valid = false; // the device lists hold the split of a call
    // An asynchronous call leaves its results on their way into hAd behind ev_ad; association_wait hands them out.
    Event ev_ad;
    bool  ad_async = false; // an asynchronous call is outstanding ...
    int   ad_async_m = 0;   // ... for this many observations (0: nothing was enqueued)
    bool  ad_ev_pending = false; // ev_ad has been recorded and not waited for since
    int associate_deferred(const void* Zv, int m, const void* Rv, double g1, double g2, int* idf_out, int* kind_out,
                           int* counts_out) override
    {
        ad_async = false; // (a later associate call discards outstanding results)
        int rc   = associate_deferred_enqueue(Zv, m, Rv, g1, g2);
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        ad_results(m, idf_out, kind_out, counts_out);
        return CSLAM_OK;
    }

    int associate_deferred_async(const void* Zv, int m, const void* Rv, double g1, double g2) override
    {
        ad_async = false;
        int rc   = use_device();
        if (rc)
        {
            return rc;
        }
        if (m > 0)
        {
            if (!ev_ad && (rc = ev_ad.create(hipEventDisableTiming)))
            {
                return rc;
            }
            if ((rc = associate_deferred_enqueue(Zv, m, Rv, g1, g2)))
            {
                return rc;
            }
            CSLAM_HIP_TRY(hipEventRecord(ev_ad.get(), stream));
            ad_ev_pending = true;
        }
        ad_async   = true;
        ad_async_m = m;
        return CSLAM_OK;
    }

    int association_wait(int* idf_out, int* kind_out, int* counts_out) override
    {
        if (!ad_async)
        {
            return fail(CSLAM_ERR_BAD_ARG, "association_wait: no asynchronous association is outstanding on this handle");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        ad_async = false;
        if (ad_async_m == 0)
        {
            if (counts_out)
            {
                counts_out[0] = counts_out[1] = counts_out[2] = 0;
            }
            return CSLAM_OK;
        }
        CSLAM_HIP_TRY(hipEventSynchronize(ev_ad.get()));
        ad_ev_pending = false;
        ad_results(ad_async_m, idf_out, kind_out, counts_out);
        return CSLAM_OK;
    }

    // counts | idf[m] | kind[m] as the copy of the last call left them in hAd
    void ad_results(int m, int* idf_out, int* kind_out, int* counts_out) const
    {
        const int* h = hAd.get();
        if (counts_out)
        {
            std::copy(h, h + 3, counts_out);
        }
        if (idf_out)
        {
            std::copy(h + 4, h + 4 + m, idf_out);
        }
        if (kind_out)
        {
            std::copy(h + 4 + m, h + 4 + 2 * m, kind_out);
        }
    }

    // everything of an association up to and including the one copy into the pinned hAd, on the handle's stream
    int associate_deferred_enqueue(const void* Zv, int m, const void* Rv, double g1, double g2)
    {
        int rc = use_device();
        if (rc || (rc = wait_pgemm()))
        {
            return rc;
        }
        const int nf = (n - 3) / 2;
        const int G  = (nf + 255) / 256;
        if (m > ad_mcap || G > ad_gcap)
        {
            const int    M = std::max(m, ad_mcap), Gc = std::max(std::max(G, ad_gcap), 1);
            const size_t mg = (size_t)M * Gc;
            CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // (nothing reads the old lists any more)
            DevBuf<T>      t;
            DevBuf<int>    i;
            PinnedBuf<int> hi;
            PinnedBuf<T>   hz;
            CSLAM_TRY(t.alloc((size_t)6 * M + 2 * mg));
            CSLAM_TRY(i.alloc((size_t)4 + 3 * M + mg));
            CSLAM_TRY(hi.alloc((size_t)4 + 2 * M));
            CSLAM_TRY(hz.alloc((size_t)2 * M));
            dAdT     = std::move(t);
            dAdI     = std::move(i);
            hAd      = std::move(hi);
            hAdZ     = std::move(hz);
            ad_mcap  = M;
            ad_gcap  = Gc;
            ad_valid = false;
        }
        const size_t M = (size_t)ad_mcap, mg = M * ad_gcap;
        T *          dZ = dAdT.get(), *dZF = dZ + 2 * M, *dZN = dZ + 4 * M, *pnd = dZ + 6 * M, *pnis = pnd + mg;
        int *        d_counts = dAdI.get(), *d_idf = d_counts + 4, *d_kind = d_idf + m, *d_idf_f = d_counts + 4 + 2 * M,
            *pj = d_idf_f + M;
        const T* R = static_cast<const T*>(Rv);
        if (ad_ev_pending) // (an asynchronous call nobody waited for: its upload may still be reading hAdZ)
        {
            CSLAM_HIP_TRY(hipEventSynchronize(ev_ad.get()));
            ad_ev_pending = false;
        }
        memcpy(hAdZ.get(), Zv, (size_t)2 * m * sizeof(T));
        CSLAM_HIP_TRY(hipMemcpyAsync(dZ, hAdZ.get(), (size_t)2 * m * sizeof(T), hipMemcpyHostToDevice, stream));
        if (G > 0)
        {
            const int* sg = (pend.kp > 0 && pend.hd_cols[pend.wcur] > 0) ? signs(pend.wcur) : (const int*)nullptr;
            hipLaunchKernelGGL(ekf_assoc_pair_kernel<T>, dim3(G), dim3(256), 0, stream, (const T*)dX.get(), (const T*)dP.get(),
                               (const T*)dPv.get(), ldp, n, R[0], R[1], R[2], R[3], opt.lower, (const T*)wbase(pend.wcur), ldp,
                               pend.kp, sg, (const T*)dZ, m, (T)g1, pnd, pj, pnis);
            CSLAM_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(ekf_assoc_resolve_kernel<T>, dim3(1), dim3(kSimThreads), 0, stream, (const T*)pnd, (const int*)pj,
                           (const T*)pnis, G, (const T*)dZ, m, (T)g2, d_idf, d_kind, dZF, d_idf_f, dZN, d_counts);
        CSLAM_HIP_TRY(hipGetLastError());
        ad_valid = true;
        CSLAM_HIP_TRY(hipMemcpyAsync(hAd.get(), d_counts, ((size_t)4 + 2 * m) * sizeof(int), hipMemcpyDeviceToHost, stream));
        return CSLAM_OK;
    }

    int association_device_ptrs(const void** dZF, const int** d_idf, const void** dZN, const int** d_counts) override
    {
        if (!ad_valid)
        {
            return fail(CSLAM_ERR_BAD_ARG, "association_device_ptrs: no association has been made on this handle");
        }
        const size_t M = (size_t)ad_mcap;
        if (dZF)
        {
            *dZF = dAdT.get() + 2 * M;
        }
        if (dZN)
        {
            *dZN = dAdT.get() + 4 * M;
        }
        if (d_idf)
        {
            *d_idf = dAdI.get() + 4 + 2 * M;
        }
        if (d_counts)
        {
            *d_counts = dAdI.get();
        }
        return CSLAM_OK;
    }

    // ---------------------------------------------------------------- predict (EKF.cpp:406-455) / heading (EKF.cpp:328-352)
    // Control steps are accepted and held back until something needs their result:
    //   predict()          is held in `pp`;
    //   observe_heading()  joins the held predict into ONE step of the pose queue `seq` (the reference's driver calls
    //                      the two back to back on every control step, test/main.cpp:165-168); up to kPoseSeqMax steps
    //                      queue up and run in ONE ekf_pose_step_kernel launch (they only touch the pose stripe Pv, X and
    //                      the pending store: see ekf_pose_kernels.hpp);
    //   a batch update on the fast path (16 < k <= 64) applies a held predict on the fly in its gather / factor /
    //                      gain kernels and commits it (PredictArgs in ekf_kernels.hpp);
    //   anything else that reads X or P launches what is queued first (resolve_predict).
    // CSLAM_FUSE_PREDICT=0 launches every predict / heading at once.
    PredictArgs<T> pp{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, 0};
    PoseSeq<T>     seq{};
    DevBuf<T>      dPred; // 16 scalars: factor kernel -> gain kernel (see FactorArgs::pred_out)
    bool           fuse_now = false; // the batch in flight consumes pp

    int predict(double v, double swa, const void* Qv, double wb, double dt) override
    {
        if (!Qv)
        {
            return fail(CSLAM_ERR_BAD_ARG, "predict: Q is null");
        }
        int rc = CSLAM_OK;
        if (pp.valid && (rc = queue_step(pp, HeadingArgs<T>{0, (T)0, (T)0}))) // two predicts in a row
        {
            return rc;
        }
        const T* Q = static_cast<const T*>(Qv);
        int      w = 0;
        if (n > 3)
        {
            w = (quirks & CSLAM_Q_PREDICT_NM4) ? (n - 4) : (n - 3);
        }
        pp = PredictArgs<T>{1, (T)v, (T)swa, Q[0], Q[1], Q[2], Q[3], (T)wb, (T)dt, std::max(w, 0)};
        if (!opt.fuse_predict)
        {
            return resolve_predict();
        }
        return CSLAM_OK;
    }

    // append one control step (predict and / or heading) to the pose queue
    int queue_step(const PredictArgs<T>& p, const HeadingArgs<T>& hd)
    {
        int rc = la_drain(); // (queued look-ahead updates come before this control step)
        if (rc)
        {
            return rc;
        }
        if (seq.count == kPoseSeqMax && (rc = launch_pose_queue()))
        {
            return rc;
        }
        int col = -1;
        if (hd.valid && n > 3)
        {
            // the rank-1 downdate -p p^T / S of the map block is one more pending column
            if (pend.kp + 1 > pend.wcap)
            {
                if ((rc = launch_pose_queue()) || (rc = flush()))
                {
                    return rc;
                }
            }
            if ((rc = own_region(pend.wcur)))
            {
                return rc;
            }
            col = pend.kp;
            pend.appended(1, true);
        }
        const int s = seq.count++;
        seq.pp[s]   = p;
        seq.hd[s]   = hd;
        seq.col[s]  = col;
        if (&p == &pp)
        {
            pp.valid = 0;
        }
        return CSLAM_OK;
    }

    int launch_pose_queue()
    {
        if (seq.count == 0)
        {
            return CSLAM_OK;
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        const int n_pad = round_up(n, kTile);
        hipLaunchKernelGGL(ekf_pose_step_kernel<T>, dim3((n_pad + 255) / 256), dim3(256), 0, stream, dX.get(),
                           dPv.get(), ldp, n, n_pad, seq, wbase(pend.wcur), ldp, dHead.get(),
                           signs(pend.wcur), sign_count(pend.wcur), dPoseDone.get());
        CSLAM_HIP_TRY(hipGetLastError());
        seq.count = 0;
        return CSLAM_OK;
    }

    // everything queued (and the held predict) runs now
    int resolve_predict() override
    {
        int rc = la_drain();
        if (rc)
        {
            return rc;
        }
        if (pp.valid && (rc = queue_step(pp, HeadingArgs<T>{0, (T)0, (T)0})))
        {
            return rc;
        }
        return launch_pose_queue();
    }

    // ---------------------------------------------------------------- update
    int launch_factor(const T* dZ, const int* dIdf, int m, const T* R)
    {
        FactorArgs<T> a;
        a.X   = dX.get();
        a.n   = n;
        a.Z   = dZ;
        a.idf = dIdf;
        a.m   = m;
        for (int i = 0; i < 4; i++)
        {
            a.R[i] = R[i];
        }
        a.PHT      = ws.dPHT.get();
        a.ldw      = ldp;
        a.dS       = ws.dS.get();
        a.dG       = ws.dG.get();
        a.dGt      = ws.dGt.get();
        a.dV       = ws.dV.get();
        a.dt       = ws.dt_.get();
        a.flags    = dFlags.get();
        a.scratchS = ws.dScrS.get();
        a.scratchG = ws.dScrG.get();
        a.textbook = (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1;
        a.stamps   = nullptr;
        a.sub      = sub_valid ? ws.dSub.get() : nullptr;
        a.dM       = nullptr;
        m_valid    = false;
        g_from_gt  = false;
        a.pp       = fuse_now ? pp : PredictArgs<T>{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, 0};
        a.P3       = dPv.get(); // the pose block lives in the stripe
        a.ldp3     = ldp;
        a.pred_out = dPred.get();
        a.lds_S    = 1;
        a.lds_G    = 1;
        return launch_factor_args(a, ws.dU.get(), stream);
    }

    // dispatch on k (a.m); du: the X-update vector u = G (G^T V)
    int launch_factor_args(FactorArgs<T>& a, T* du, hipStream_t st)
    {
        const int k = 2 * a.m, m = a.m;
        const bool own = (a.dM == nullptr); // the handle's own workspace: record what the gain kernel will find
        // Which kernel factorises S (all of them produce G^T, t, u; the tuned ones also M for the gain kernel's
        // pose-stripe downdate):
        //   k <= 16            ekf_factor_small_kernel: one wave, a row per lane, v_readlane broadcasts
        //   16 < k <= 64       ekf_factor_mfma_f32 / _f64: rank-1 updates on the matrix cores
        //   64 < k <= 128 f32  ekf_factor_mfma_big_f32: four 32-wide blocks
        //   beyond             ekf_factor_kernel: the general LDS / global-scratch form
        if (k <= 4)
        {
            a.dM    = own ? ws.dM.get() : a.dM;
            m_valid = own ? true : m_valid;
            hipLaunchKernelGGL((ekf_factor_small_kernel<T, 4>), dim3(1), dim3(256), 0, st, a, du);
        }
        else if (k <= 16)
        {
            a.dM    = own ? ws.dM.get() : a.dM;
            m_valid = own ? true : m_valid;
            hipLaunchKernelGGL((ekf_factor_small_kernel<T, 16>), dim3(1), dim3(256), 0, st, a, du);
        }
        else if (k <= 64)
        {
            a.dM      = own ? ws.dM.get() : a.dM;
            m_valid   = own ? true : m_valid;
            g_from_gt = own ? true : g_from_gt;
            if constexpr (std::is_same<T, float>::value)
            {
                if (k <= 32)
                {
                    hipLaunchKernelGGL((ekf_factor_mfma_f32<32>), dim3(1), dim3(256), 0, st, a, du);
                }
                else
                {
                    hipLaunchKernelGGL((ekf_factor_mfma_f32<64>), dim3(1), dim3(256), 0, st, a, du);
                }
            }
            else
            {
                auto lds64 = [](int K) {
                    return (size_t)(K * (K + 1) + (3 + K) * (K + 1) + (K / 2) * 10 + 6 * K) * sizeof(double) +
                           (size_t)(K / 2 + 4) * sizeof(int) + 16;
                };
                if (k <= 32)
                {
                    hipLaunchKernelGGL((ekf_factor_mfma_f64<32>), dim3(1), dim3(256), lds64(32), st, a, du);
                }
                else
                {
                    hipLaunchKernelGGL((ekf_factor_mfma_f64<64>), dim3(1), dim3(256), lds64(64), st, a, du);
                }
            }
        }
        else if (std::is_same<T, float>::value && k <= 128)
        {
            if constexpr (std::is_same<T, float>::value)
            {
                constexpr int K   = 128;
                const size_t  lds = (size_t)(K * (K + 1) + (3 + K) * (K + 1) + (K / 2) * 10 + 6 * K) * sizeof(float) +
                                   (size_t)(K / 2 + 4) * sizeof(int) + 16;
                a.dM      = own ? ws.dM.get() : a.dM;
                m_valid   = own ? true : m_valid;
                g_from_gt = own ? true : g_from_gt;
                hipLaunchKernelGGL((ekf_factor_mfma_big_f32<128>), dim3(1), dim3(256), lds, st, a, du);
            }
        }
        else
        {
            size_t mat   = (size_t)k * (k + 1) * sizeof(T);
            size_t small = ((size_t)m * 10 + k) * sizeof(T) + ((size_t)m + 4) * sizeof(int) + 64;
            a.lds_S      = (mat + small <= kLdsBudget) ? 1 : 0;
            a.lds_G      = (a.lds_S && 2 * mat + small <= kLdsBudget) ? 1 : 0;
            size_t lds   = small + (a.lds_S ? mat : 0) + (a.lds_G ? mat : 0);
            hipLaunchKernelGGL(ekf_factor_kernel<T>, dim3(1), dim3(kFactorThreads), lds, st, a);
        }
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    // W1 of this update goes to `slot` (n_pad x k8 columns of the pending store); then the pose stripe takes its share
    // of the downdate at once and the panel's pose rows are zeroed (ekf_pose_downdate_kernel)
    int launch_gain(int k, T* slot, const T* Gt = nullptr, const T* U = nullptr, const T* M = nullptr)
    {
        // (Gt / U / M: the factor outputs to apply -- the handle's own workspace unless a look-ahead window passes a slot's)
        const int n_pad    = round_up(n, kTile);
        pose_fused_in_gain = false;
        if (Gt == nullptr)
        {
            Gt = ws.dGt.get();
            U  = ws.dU.get();
            M  = m_valid ? ws.dM.get() : nullptr;
        }
        if (!launch_gain_fast(k, n_pad, slot, Gt, U, M))
        {
            // the general vector-unit form (f32 beyond k = 128, f64 beyond k = 64): no X vector u, no fused pose downdate
            hipLaunchKernelGGL(ekf_gain_kernel<T>, dim3(n_pad / 64), dim3(256), 0, stream, ws.dPHT.get(), ldp, n, n_pad,
                               k, ws.dGt.get(), ws.dt_.get(), slot, dX.get());
        }
        CSLAM_HIP_TRY(hipGetLastError());
        if (pose_fused_in_gain)
        {
            return CSLAM_OK; // ekf_panel_mfma_f32 applied the pose-stripe downdate and zeroed the panel's pose rows itself
        }
        hipLaunchKernelGGL(ekf_pose_downdate_kernel<T>, dim3((n + 63) / 64), dim3(256), 0, stream, slot, ldp, k,
                           round_up(k, 8), n, dPv.get(), ldp, ws.dWv.get(), dPoseDone.get() + 1);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }
    bool pose_fused_in_gain = false;

    int  launch_downdate(const T* W, int k, hipStream_t st);
    bool launch_corr_fast(int k, const T* Wp, int kc);          // PHT -= Wp*Y^T on MFMA (f32)
    int  ensure_tile_list(int tiles);
    int  pgemm_grid() const;
    bool launch_gain_fast(int k, int n_pad, T* slot, const T* Gt, const T* U, const T* M); // MFMA gain

    // one batch of m observations with device-resident Z / idf (slam.h:235-266 via EKF.cpp:93-129).
    // keep_pending: never start this update's (or any pending) P-GEMM inside the call (sequential mode).
    int batch_on_device(const T* dZ, const int* dIdf, int m, const T* R, bool keep_pending)
    {
        const int k  = 2 * m;
        int       rc = ensure_k(k);
        if (rc)
        {
            return rc;
        }
        // a few pending columns (heading observations) are corrected for inside the gather kernel: the fast path stays
        // ... and so is one deferred batch panel (up to kGatherCorrMax columns), by the kernel's wider form
        const bool small_corr = pend.kp > 0 && pend.kp <= (opt.gather_corr_wide ? kGatherCorrMax : kGatherCorr) && !opt.pipeline;
        const bool wide_corr  = small_corr && pend.kp > kGatherCorr;
        // a pending predict() rides along when this batch takes the (non-pipelined) fast path
        fuse_now = pp.valid && (sizeof(T) == 4 || opt.fuse_f64) && !opt.pipeline && !keep_pending && k > 16 && k <= 64;
        if ((rc = fuse_now ? launch_pose_queue() : resolve_predict())) // (queued control steps come first either way)
        {
            return rc;
        }
        if (fuse_now && !dPred.get() && (rc = dPred.alloc(16)))
        {
            return rc;
        }
        // the general gain kernels and ekf_pose_downdate_kernel write whole blocks of 8 columns of the slot: the slot starts
        // at column kp (heading columns make kp any number), so kp + round_up(k, 8) must stay inside the region
        const int k8w = round_up(k, 8);
        if ((rc = ensure_w(std::max(k8w, kp_call_limit)))) // (may flush and move the store)
        {
            return rc;
        }
        // Pipelined: the pending columns' P-GEMM starts right behind this update's gather and runs under its chain.
        // It is held back while an explicit deferral window (cslam_ekf_set_deferred) still has room for this panel.
        const bool overlap = opt.pipeline && !keep_pending && pend.kp > 0 && (defer_max == 0 || pend.kp + k > defer_max);
        // pending columns stay pending through this update while they fit the window: the explicit deferral window, the
        // sequential call's own columns, else the store (e.g. heading columns in immediate mode: applied together with
        // this update's panel by the flush below)
        const int window = std::min(pend.wcap, defer_max > 0 ? defer_max : (kp_call_limit > 0 ? kp_call_limit : pend.wcap));
        if (!overlap && pend.kp > 0 && (pend.kp + k > window || pend.kp + k8w > pend.wcap))
        {
            if ((rc = flush())) // no room to keep them pending: apply them first
            {
                return rc;
            }
        }
        if ((rc = wait_pgemm())) // Ps must be quiescent for the gather
        {
            return rc;
        }
        last_k = k;
        last_counted = false;
        dbgS = dbgGt = dbgV = nullptr; // (debug_last_update reads the handle's own workspace again)
        if ((rc = prof.begin(CSLAM_STAGE_GATHER, stream)))
        {
            return rc;
        }
        const dim3 ggrid((n + 255) / 256, (m + kGatherObs - 1) / kGatherObs);
        // the compact H-rows block for the MFMA factor kernel (f32, 16 < k <= 64, no pending panels to correct)
        sub_valid = (k > 16 && k <= 64 && (pend.kp == 0 || small_corr) && ws.dSub.get() != nullptr);
        PredictArgs<T> pnone{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, 0};
        {
            T*             sub  = sub_valid ? ws.dSub.get() : nullptr;
            PredictArgs<T> pa   = fuse_now ? pp : pnone;
            T*             pred = fuse_now ? dPred.get() : (T*)nullptr;
            const T*       Wg   = (pend.kp > 0 && !opt.pipeline) ? (const T*)wbase(pend.wcur) : (const T*)nullptr;
            const int      kg   = opt.pipeline ? 0 : pend.kp;
            const int*     sg =
                (pend.kp > 0 && !opt.pipeline && pend.hd_cols[pend.wcur] > 0) ? signs(pend.wcur) : (const int*)nullptr;
            T* yout = (pend.kp > 0 && !small_corr && !opt.pipeline) ? ws.dY.get() : (T*)nullptr;
            if (wide_corr)
            {
                const dim3 wgrid((n + 255) / 256, (m + kGatherObsWide - 1) / kGatherObsWide);
                hipLaunchKernelGGL((ekf_gather_kernel<T, kGatherCorrMax, kGatherObsWide>), wgrid, dim3(256), 0, stream,
                                   dX.get(), dP.get(), dPv.get(), ldp, n, dZ, dIdf, m, ws.dPHT.get(), ldp, opt.lower, sub,
                                   pa, pred, Wg, ldp, kg, sg, dFlags.get(), yout);
            }
            else
            {
                hipLaunchKernelGGL(ekf_gather_kernel<T>, ggrid, dim3(256), 0, stream, dX.get(), dP.get(), dPv.get(),
                                   ldp, n, dZ, dIdf, m, ws.dPHT.get(), ldp, opt.lower, sub, pa, pred, Wg, ldp, kg, sg,
                                   dFlags.get(), yout);
            }
        }
        CSLAM_HIP_TRY(hipGetLastError());
        // the panels this update's P*H^T must be corrected with, and where its own W1 goes
        const T*  Wc        = wbase(pend.wcur);
        const int kc        = pend.kp;
        const int rc_region = pend.wcur;
        if (overlap)
        {
            if ((rc = flush())) // P-GEMM of the pending columns on stream B, behind the gather; store -> other region
            {
                return rc;
            }
        }
        T* slot = wbase(pend.wcur) + (size_t)pend.kp * ldp;
        if ((rc = own_region(pend.wcur)))
        {
            return rc;
        }
        if (kc > 0 && !small_corr) // PHT -= Wp * (H*Wp)^T : the pending panels' share of P*H^T (their pose rows are zero)
        {
            if (opt.pipeline) // (single stream: the gather kernel has published Y = H*Wp already)
            {
                hipLaunchKernelGGL(ekf_pending_y_kernel<T>, dim3(m, (kc + 255) / 256), dim3(256), 0, stream, dX.get(), n, dZ, dIdf,
                                   m, Wc, ldp, kc, ws.dY.get(),
                                   pend.hd_cols[rc_region] > 0 ? signs(rc_region) : (const int*)nullptr);
                CSLAM_HIP_TRY(hipGetLastError());
            }
            if (!launch_corr_fast(k, Wc, kc))
            {
                hipLaunchKernelGGL(ekf_pending_corr_kernel<T>, ggrid, dim3(256), 0, stream, n, m, Wc, ldp, kc,
                                   ws.dY.get(), ws.dPHT.get(), ldp);
            }
            CSLAM_HIP_TRY(hipGetLastError());
        }
        if ((rc = prof.end(CSLAM_STAGE_GATHER, stream)) || (rc = prof.begin(CSLAM_STAGE_FACTOR, stream)) ||
            (rc = launch_factor(dZ, dIdf, m, R)) || (rc = prof.end(CSLAM_STAGE_FACTOR, stream)) ||
            (rc = prof.begin(CSLAM_STAGE_GAIN, stream)) || (rc = launch_gain(k, slot)) || (rc = prof.end(CSLAM_STAGE_GAIN, stream)))
        {
            return rc;
        }
        if (fuse_now) // the gain kernel committed the predicted pose, stripe and Pvv
        {
            pp.valid = 0;
            fuse_now = false;
        }
        last_slot = slot;
        pend.appended(k);
        const bool deferring = keep_pending || opt.pipeline || defer_max > 0;
        if (!deferring && (rc = flush()))
        {
            return rc;
        }
        if (sync_mode)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(hFlags.get(), dFlags.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            if (hFlags[1] & kFlagLltFailed)
            {
                return eigen_fallback(k, deferring);
            }
        }
        // explicit deferral without pipelining: once the window is full, apply it now rather than at the start of
        // the next update
        if (!opt.pipeline && !keep_pending && defer_max > 0 && pend.kp >= defer_max && (rc = flush()))
        {
            return rc;
        }
        return CSLAM_OK;
    }

    // ---------------------------------------------------------------- the counted update (ekf_counted_kernels.hpp)
    // batch_on_device(dZ, dIdf, c, R) with c = clamp(*d_count, 0, m_cap) read by every kernel in stream order: the host
    // never learns c.  It therefore plans for m_cap -- workspace, kernel class, grids, the room in the pending store, the
    // 2 m_cap columns it books -- and the gain kernel writes the columns beyond 2c as zeros.  The classic chain only:
    // queued work (a look-ahead window, the pose queue) and a held predict are launched first and nothing is fused.
    // Nothing in here waits for the device or copies from it.
    bool last_counted = false; // the last update was a counted one: debug_last_update cannot know its k
    int  update_counted(const void* dZv, int m_cap, const void* Rv, const int* dIdf, const int* d_count, int batch) override
    {
        const int m_max = sizeof(T) == 4 ? 64 : 32; // the ranges of the tuned factor and gain kernels
        if (m_cap < 0 || m_cap > m_max || !Rv || !dZv || !dIdf || !d_count || !batch || sync_mode || opt.pipeline)
        {
            return fail(CSLAM_ERR_BAD_ARG,
                        "update_counted: bad arguments (m_cap=%d of at most %d, batch=%d, sync_mode=%d, two streams=%d)", m_cap,
                        m_max, batch, sync_mode, (int)opt.pipeline);
        }
        if (m_cap == 0)
        {
            return CSLAM_OK;
        }
        const T*  dZ = static_cast<const T*>(dZv);
        const T*  R  = static_cast<const T*>(Rv);
        const int m = m_cap, k = 2 * m_cap;
        int       rc = use_device();
        if (rc || (rc = ensure_k(k)) || (rc = resolve_predict())) // (drains a queued look-ahead update as a window of one)
        {
            return rc;
        }
        fuse_now = false;
        const bool small_corr = pend.kp > 0 && pend.kp <= (opt.gather_corr_wide ? kGatherCorrMax : kGatherCorr);
        const bool wide_corr  = small_corr && pend.kp > kGatherCorr;
        const int  k8w        = round_up(k, 8);
        if ((rc = ensure_w(std::max(k8w, kp_call_limit)))) // (may flush and move the store)
        {
            return rc;
        }
        // the deferral window and the flush rules of batch_on_device with k = 2 m_cap
        const int window = std::min(pend.wcap, defer_max > 0 ? defer_max : (kp_call_limit > 0 ? kp_call_limit : pend.wcap));
        if (pend.kp > 0 && (pend.kp + k > window || pend.kp + k8w > pend.wcap) && (rc = flush()))
        {
            return rc;
        }
        if ((rc = wait_pgemm()))
        {
            return rc;
        }
        last_k       = k;
        last_counted = true;
        dbgS = dbgGt = dbgV = nullptr;
        if ((rc = prof.begin(CSLAM_STAGE_GATHER, stream)))
        {
            return rc;
        }
        sub_valid         = (k > 16 && k <= 64 && (pend.kp == 0 || small_corr) && ws.dSub.get() != nullptr);
        const int  kc     = pend.kp;
        const T*   Wc     = wbase(pend.wcur);
        const int* sg     = (kc > 0 && pend.hd_cols[pend.wcur] > 0) ? signs(pend.wcur) : (const int*)nullptr;
        const int  n_pad  = round_up(n, kTile);
        {
            T*       sub  = sub_valid ? ws.dSub.get() : nullptr;
            const PredictArgs<T> pnone{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, 0};
            const T* Wg   = kc > 0 ? Wc : (const T*)nullptr;
            T*       yout = (kc > 0 && !small_corr) ? ws.dY.get() : (T*)nullptr;
            if (wide_corr)
            {
                const dim3 wgrid((n + 255) / 256, (m + kGatherObsWide - 1) / kGatherObsWide);
                hipLaunchKernelGGL((ekf_gather_counted_kernel<T, kGatherCorrMax, kGatherObsWide>), wgrid, dim3(256), 0, stream,
                                   dX.get(), dP.get(), dPv.get(), ldp, n, dZ, dIdf, d_count, m_cap, ws.dPHT.get(), ldp,
                                   opt.lower, sub, pnone, (T*)nullptr, Wg, ldp, kc, sg, dFlags.get(), yout);
            }
            else
            {
                const dim3 ggrid((n + 255) / 256, (m + kGatherObs - 1) / kGatherObs);
                hipLaunchKernelGGL(ekf_gather_counted_kernel<T>, ggrid, dim3(256), 0, stream, dX.get(), dP.get(), dPv.get(),
                                   ldp, n, dZ, dIdf, d_count, m_cap, ws.dPHT.get(), ldp, opt.lower, sub, pnone, (T*)nullptr, Wg,
                                   ldp, kc, sg, dFlags.get(), yout);
            }
        }
        CSLAM_HIP_TRY(hipGetLastError());
        T* slot = wbase(pend.wcur) + (size_t)pend.kp * ldp;
        if ((rc = own_region(pend.wcur)))
        {
            return rc;
        }
        if (kc > 0 && !small_corr) // PHT -= Wp * (H*Wp)^T (the gather kernel has published Y = H*Wp)
        {
            if constexpr (std::is_same<T, float>::value)
            {
                hipLaunchKernelGGL(ekf_corr_mfma_f32_counted, dim3(n_pad / 32, (k + 31) / 32), dim3(64), 0, stream, Wc, ldp, n,
                                   kc, d_count, m_cap, (const T*)ws.dY.get(), ws.dPHT.get(), ldp);
            }
            else
            {
                hipLaunchKernelGGL(ekf_corr_mfma_f64_counted, dim3(n_pad / 16, (k + 15) / 16), dim3(64), 0, stream, Wc, ldp, n,
                                   kc, d_count, m_cap, (const T*)ws.dY.get(), ws.dPHT.get(), ldp);
            }
            CSLAM_HIP_TRY(hipGetLastError());
        }
        if ((rc = prof.end(CSLAM_STAGE_GATHER, stream)) || (rc = prof.begin(CSLAM_STAGE_FACTOR, stream)) ||
            (rc = launch_factor_counted(dZ, dIdf, d_count, m_cap, R)) || (rc = prof.end(CSLAM_STAGE_FACTOR, stream)) ||
            (rc = prof.begin(CSLAM_STAGE_GAIN, stream)))
        {
            return rc;
        }
        if constexpr (std::is_same<T, float>::value)
        {
            hipLaunchKernelGGL(ekf_gain_mfma_f32_counted, dim3(n_pad / 32, (k + 31) / 32), dim3(64), 0, stream,
                               (const T*)ws.dPHT.get(), ldp, n, d_count, m_cap, (const T*)ws.dGt.get(), (const T*)ws.dU.get(),
                               slot, ldp, dX.get(), dPv.get(), ldp, (const T*)ws.dM.get(), ws.dWv.get());
        }
        else
        {
            hipLaunchKernelGGL(ekf_gain_mfma_f64_counted, dim3(n_pad / 16, (k + 15) / 16), dim3(64), 0, stream,
                               (const T*)ws.dPHT.get(), ldp, n, d_count, m_cap, (const T*)ws.dGt.get(), (const T*)ws.dU.get(),
                               slot, ldp, dX.get(), dPv.get(), ldp, (const T*)ws.dM.get(), ws.dWv.get());
        }
        CSLAM_HIP_TRY(hipGetLastError());
        pose_fused_in_gain = true;
        if ((rc = prof.end(CSLAM_STAGE_GAIN, stream)))
        {
            return rc;
        }
        last_slot = slot;
        pend.appended(k);
        if (defer_max == 0 && (rc = flush()))
        {
            return rc;
        }
        if (defer_max > 0 && pend.kp >= defer_max && (rc = flush())) // the window is full: apply it now
        {
            return rc;
        }
        return CSLAM_OK;
    }

    // the factor kernel class of launch_factor_args for k = 2 m_cap, in its counted form (always on the handle's workspace)
    int launch_factor_counted(const T* dZ, const int* dIdf, const int* d_count, int m_cap, const T* R)
    {
        FactorArgs<T> a;
        a.X   = dX.get();
        a.n   = n;
        a.Z   = dZ;
        a.idf = dIdf;
        a.m   = m_cap; // (the kernel replaces it with the count)
        for (int i = 0; i < 4; i++)
        {
            a.R[i] = R[i];
        }
        a.PHT      = ws.dPHT.get();
        a.ldw      = ldp;
        a.dS       = ws.dS.get();
        a.dG       = ws.dG.get();
        a.dGt      = ws.dGt.get();
        a.dV       = ws.dV.get();
        a.dt       = ws.dt_.get();
        a.flags    = dFlags.get();
        a.scratchS = ws.dScrS.get();
        a.scratchG = ws.dScrG.get();
        a.textbook = (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1;
        a.stamps   = nullptr;
        a.sub      = sub_valid ? ws.dSub.get() : nullptr;
        a.dM       = ws.dM.get();
        a.pp       = PredictArgs<T>{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, 0};
        a.P3       = dPv.get();
        a.ldp3     = ldp;
        a.pred_out = dPred.get();
        a.lds_S    = 1;
        a.lds_G    = 1;
        m_valid    = true;
        const int k = 2 * m_cap;
        g_from_gt   = k > 16;
        T* du       = ws.dU.get();
        if (k <= 4)
        {
            hipLaunchKernelGGL((ekf_factor_small_counted_kernel<T, 4>), dim3(1), dim3(256), 0, stream, a, du, d_count, m_cap);
        }
        else if (k <= 16)
        {
            hipLaunchKernelGGL((ekf_factor_small_counted_kernel<T, 16>), dim3(1), dim3(256), 0, stream, a, du, d_count, m_cap);
        }
        else if constexpr (std::is_same<T, float>::value)
        {
            if (k <= 32)
            {
                hipLaunchKernelGGL((ekf_factor_mfma_f32_counted<32>), dim3(1), dim3(256), 0, stream, a, du, d_count, m_cap);
            }
            else if (k <= 64)
            {
                hipLaunchKernelGGL((ekf_factor_mfma_f32_counted<64>), dim3(1), dim3(256), 0, stream, a, du, d_count, m_cap);
            }
            else
            {
                constexpr int K   = 128;
                const size_t  lds = (size_t)(K * (K + 1) + (3 + K) * (K + 1) + (K / 2) * 10 + 6 * K) * sizeof(float) +
                                   (size_t)(K / 2 + 4) * sizeof(int) + 16;
                hipLaunchKernelGGL((ekf_factor_mfma_big_f32_counted<128>), dim3(1), dim3(256), lds, stream, a, du, d_count,
                                   m_cap);
            }
        }
        else
        {
            auto lds64 = [](int K) {
                return (size_t)(K * (K + 1) + (3 + K) * (K + 1) + (K / 2) * 10 + 6 * K) * sizeof(double) +
                       (size_t)(K / 2 + 4) * sizeof(int) + 16;
            };
            if (k <= 32)
            {
                hipLaunchKernelGGL((ekf_factor_mfma_f64_counted<32>), dim3(1), dim3(256), lds64(32), stream, a, du, d_count,
                                   m_cap);
            }
            else
            {
                hipLaunchKernelGGL((ekf_factor_mfma_f64_counted<64>), dim3(1), dim3(256), lds64(64), stream, a, du, d_count,
                                   m_cap);
            }
        }
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    // slam.h:425-429 on the host: the device left X and P untouched (G = 0, t = 0)
    int eigen_fallback(int k, bool still_pending)
    {
        sticky_host |= CSLAM_FACTOR_FALLBACK;
        std::vector<T> S((size_t)k * k), V((size_t)k), G;
        CSLAM_HIP_TRY(hipMemcpyAsync(S.data(), ws.dS.get(), S.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipMemcpyAsync(V.data(), ws.dV.get(), V.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        bool textbook = !(quirks & CSLAM_Q_LOWER_CHOL_GAIN);
        if (!host_eigen_fallback_gain(S.data(), k, textbook, G))
        {
            sticky_host |= CSLAM_FACTOR_ZEROED;
            return CSLAM_OK; // zeros: the update is a no-op, which is what the device already did
        }
        std::vector<T> Gt((size_t)k * k), t((size_t)k, (T)0);
        for (int c = 0; c < k; c++)
        {
            for (int r = 0; r < k; r++)
            {
                Gt[(size_t)r * k + c] = G[(size_t)c * k + r];
                t[c] += G[(size_t)c * k + r] * V[r];
            }
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(ws.dG.get(), G.data(), G.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        CSLAM_HIP_TRY(hipMemcpyAsync(ws.dGt.get(), Gt.data(), Gt.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        g_from_gt  = false; // (the fallback gain is a general matrix, uploaded as G and G^T)
        m_valid    = false; // (M belonged to the zeroed G: the separate pose downdate kernel runs)
        CSLAM_HIP_TRY(hipMemcpyAsync(ws.dt_.get(), t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        std::vector<T> u((size_t)k, (T)0);
        for (int q = 0; q < k; q++)
        {
            for (int c = 0; c < k; c++)
            {
                u[q] += G[(size_t)c * k + q] * t[c];
            }
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(ws.dU.get(), u.data(), u.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        int rc;
        if ((rc = own_region(pend.wcur)))
        {
            return rc;
        }
        // the zero G made this update's W1 slot zero (a no-op wherever it was or will be applied): rewrite it
        // (the gain kernel's pose downdate runs again on the new panel: the first one subtracted zeros)
        if ((rc = launch_gain(k, last_slot)))
        {
            return rc;
        }
        if (!still_pending) // its P-GEMM already ran (with zeros): apply this panel alone
        {
            const int k8 = round_up(k, 8);
            if (k8 > k)
            {
                CSLAM_HIP_TRY(hipMemset2DAsync(last_slot + (size_t)k * ldp, (size_t)ldp * sizeof(T), 0,
                                               (size_t)round_up(n, kTile) * sizeof(T), (size_t)(k8 - k), stream));
            }
            if ((rc = launch_downdate(last_slot, k, stream)))
            {
                return rc;
            }
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }


    // ---------------------------------------------------------------- look-ahead windows (ekf_lookahead.hpp)
    // Asynchronous batch updates (16 < k <= 64) are collected two at a time.  For a window (a, b):
    //   stream   : rows / blocks kernels (small blocks of the current P for the factor chain)
    //   stream F : prefactor(a), factor(a), prefactor(b), factor(b) -- 1-workgroup kernels, ~60 us in all
    //   stream   : P-GEMM of the PREVIOUS window (k = 128), under which stream F runs;
    //              then gather(a), gain(a), gather(b) (corrected for W1_a in the kernel), gain(b) with the factors known.
    // The state the rest of the engine sees afterwards is the deferred engine's after two updates (k_a + k_b pending
    // columns in the store), so every other call simply drains the queue first (la_drain) and carries on.
    struct LaUpd
    {
        const T*       dZ;
        const int*     dIdf;
        int            m;
        T              R[4];
        PredictArgs<T> pp;
    };
    struct FactorOut
    {
        DevBuf<T>   S, G, Gt, V, t, U, M, sub, xloc;
        DevBuf<int> idloc;
    };
    // what the first window sets up, as a whole (la_ensure)
    struct LaSet
    {
        Event          ev_fb;  // the chain kernel of the last window has finished
        Event          ev_raw; // the blocks kernel of the last window has finished (several engines alive only)
        FactorOut      fo[2];
        DevBuf<T>      XL, PvL, PH, PvLb, Dbb;
        DevBuf<T>      Y;      // H_b * W1_a of the last window (for a fused wide kernel)
        DevBuf<LaModel<T>> model; // [2]: predict + observation model of update a / b
        DevBuf<unsigned>   done;  // device counter: workgroups of the blocks kernels that have finished
        DevBuf<long long>  stamps; // CSLAM_LA_STAMPS=1: phase stamps of factor(a) underneath the P-GEMM (diagnostics)
        DevBuf<int>        idf_keep; // update b's feature ids and ...
        DevBuf<T>          z_keep;   // ... Z, copied by the rows kernel (mirror form: the blocks kernel) of a window whose wide launch is held
    };
    // A window's wide launch, built but not yet submitted (la_launch_held_wide).  Everything on the host is already as if
    // it had been launched (kp, last_slot, sub_valid, the held predict): only the device has not been told.
    struct LaHeld
    {
        bool       valid = false;
        bool       k64   = false;
        unsigned   grid  = 0;
        LaWideArgs wa;
        float*     wt = nullptr; // != nullptr: the k = 64 kernel that also writes the row-major mirror
    };
    LaHeld      la_held;
    LaUpd       la_q[2];
    int         la_n = 0;
    LaSet       la;
    bool        la_ready = false;   // la_ensure has set `la` and stream F up
    hipStream_t stream_f = nullptr; // = stream_f_own.get() from then on
    DevBuf<T>   la_WR;
    int         la_kpad  = 0;
    int         la_cus = 0;        // compute units the persistent P-GEMM leaves to the chain kernel (0 until stream F exists)
    unsigned    la_target = 0;       // its value once every blocks kernel launched so far has finished
    unsigned    la_seq    = 0;       // windows whose chain kernel has been launched
    // != 0: the next P-GEMM launch (ekf_downdate_psym4_f32) adds this to la_done[0] -- the chain's go-ahead, in place of a
    // release fence + atomic in every workgroup of the blocks kernel (8.8 -> 6.6 us per window); see la_launch_window
    unsigned    la_sig_add = 0;
    // The row-major mirror of the pending panels (f32; written by ekf_la_wide_f32_k64m, read by the NEXT window's
    // ekf_la_blocks_mirror_kernel, which precedes the next wide kernel on the main stream: one buffer suffices).
    // What it covers is part of the pending store's bookkeeping (PendingCols::mirror_covers): a window takes the mirror
    // path only when that is all kp pending columns.
    DevBuf<float> la_WT;
    int           la_wt_rows     = 0;
    // what debug_last_update reads (the handle's workspace, or the factor slot of a window's last update)
    const T *dbgS = nullptr, *dbgGt = nullptr, *dbgV = nullptr;

    int la_ensure(int kp_cols)
    {
        constexpr int KM = 2 * kLaMaxObs;
        if (!la_ready)
        {
            // The chain kernel owns its compute unit by the LDS it asks for (see ekf_la_chain_kernel); the persistent
            // P-GEMM's grid is reduced by that unit's two workgroups (la_cus).
            int lo = 0, hi = 0;
            CSLAM_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
            Stream sf;
            LaSet  nl;
            int    rc = sf.create_with_priority(hipStreamNonBlocking, hi);
            if (rc || (rc = nl.ev_fb.create(hipEventDisableTiming)) || (rc = nl.ev_raw.create(hipEventDisableTiming)))
            {
                return rc;
            }
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_la_chain_kernel<T, 32>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)la_chain_lds<T>(32)));
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_la_chain_kernel<T, 64>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)la_chain_lds<T>(64)));
            // words 0..255: 16 counters (stride 16) of finished blocks-kernel workgroups; words 256..767: 32 copies
            // (stride 16) of the last window whose chain kernel has finished
            CSLAM_TRY(nl.done.alloc_zeroed_blocking(768));
            for (FactorOut& f : nl.fo)
            {
                const size_t kk = (size_t)KM * (KM + 1);
                if ((rc = f.S.alloc(kk)) || (rc = f.G.alloc(kk)) || (rc = f.Gt.alloc(kk)) || (rc = f.V.alloc(KM)) ||
                    (rc = f.t.alloc(KM)) || (rc = f.U.alloc(KM)) || (rc = f.M.alloc((size_t)3 * KM)) ||
                    (rc = f.sub.alloc((size_t)(3 + KM) * KM)) || (rc = f.xloc.alloc(3 + KM)) ||
                    (rc = f.idloc.alloc(kLaMaxObs)))
                {
                    return rc;
                }
            }
            if ((rc = nl.XL.alloc((size_t)2 * KM)) || (rc = nl.PvL.alloc((size_t)2 * KM * 3)) ||
                (rc = nl.PH.alloc((size_t)KM * KM)) || (rc = nl.PvLb.alloc((size_t)KM * 3)) ||
                (rc = nl.Dbb.alloc((size_t)KM * KM)) || (rc = nl.Y.alloc((size_t)KM * KM)) ||
                (rc = nl.model.alloc(2)) || (rc = nl.idf_keep.alloc(kLaMaxObs)) ||
                (rc = nl.z_keep.alloc(2 * kLaMaxObs)) ||
                (opt.la_stamps && (rc = nl.stamps.alloc_zeroed_blocking(32))))
            {
                return rc;
            }
            stream_f_own = std::move(sf);
            stream_f     = stream_f_own.get();
            la           = std::move(nl);
            la_cus       = 1;
            la_target    = 0;
            la_seq       = 0;
            la_ready     = true;
        }
        if (kp_cols > la_kpad)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream_f));
            const int kpad = round_up(std::max(kp_cols, 128), 64);
            DevBuf<T> wr;
            CSLAM_TRY(wr.alloc((size_t)2 * KM * kpad)); // [kpad columns][128 slots]
            la_WR   = std::move(wr);
            la_kpad = kpad;
        }
        if (opt.la_mirror && std::is_same<T, float>::value && round_up(n, kTile) > la_wt_rows)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream_f));
            const int     rows = round_up(n, kTile);
            DevBuf<float> wt;
            CSLAM_TRY(wt.alloc((size_t)rows * 128)); // [rows][128 columns]
            la_WT          = std::move(wt);
            la_wt_rows     = rows;
            pend.mirror_void();
        }
        return CSLAM_OK;
    }

    // may this batch join a look-ahead window?  (everything the window's fixed schedule does not cover stays classic)
    bool la_eligible(int m) const
    {
        const int k = 2 * m;
        // lookahead: 1 on, 0 off, -1 (default) where it pays: f32 and a P-GEMM long enough to hide the factor chain
        // (~70 us) underneath it -- about N >= 3500 landmarks; a short P-GEMM leaves the chain on the critical path
        // (measured: f64 N = 1000 12.9 k steps/s with windows against 15.8 k without)
        const bool on = opt.lookahead > 0 || (opt.lookahead < 0 && sizeof(T) == 4 && n >= 7000 && g_engines.load() == 1);
        return on && !sync_mode && !opt.pipeline && prof.mode != 1 && k > 16 && k <= 2 * kLaMaxObs && opt.gather_corr_wide &&
               opt.fuse_predict && (sizeof(T) == 4 || opt.fuse_f64) && defer_max >= k + (la_n ? 2 * la_q[0].m : k) &&
               pend.wcap >= k + (la_n ? 2 * la_q[0].m : k) && seq.count == 0 && pend.hd_cols[0] == 0 && pend.hd_cols[1] == 0 && n > 3 &&
               kp_call_limit == 0;
    }

    // The wide launch of a window is the last thing the window enqueues, and nothing waits for it until the next call on
    // the handle arrives.  With CSLAM_LA_HOLD_WIDE (default) the call that completes a window therefore stops after the
    // P-GEMM and keeps the wide launch, arguments ready, in la_held; the NEXT call that enqueues anything on the handle's
    // streams, waits for them, or ends the handle submits it first.  All of them pass through one of four places:
    // la_enqueue (below), la_drain (every other entry point: resolve_predict, queue_step, ensure_m, factor_status, ...),
    // update() in front of a host-staged copy, and the destructor.  A predict is held on the host and launches
    // nothing, so it leaves the wide held.  The order of the kernels on the main stream is exactly what it was.
    //   What a caller may conclude from the main stream (cslam_ekf_get_streams) is also what it was.  Without the hold,
    // the wide kernel at the end of b's call waits for the chain kernel on stream F, so a caller that has waited for the
    // main stream knows that every reader of b's buffers has finished.  A window whose wide launch is held therefore
    // reads b's caller buffers from main-stream kernels of b's call only (rows, blocks); the chain kernel and the held
    // wide kernel read the engine's copies (la.z_keep / la.idf_keep, written by the rows kernel or, where the mirror form
    // runs, by the blocks kernel: see la_launch_window).
    // `job`: the snapshot the launch carries (LaSnapJob), or nullptr.  On an error the launch stays held.
    int la_launch_held_wide(const LaSnapJob* job)
    {
        if (!la_held.valid)
        {
            return CSLAM_OK;
        }
        if constexpr (std::is_same<T, float>::value)
        {
            int rc = use_device();
            if (rc)
            {
                return rc;
            }
            if (g_engines.load() > 1) // (a second engine has appeared since: no unguarded wait inside the kernel, see g_engines)
            {
                CSLAM_HIP_TRY(hipStreamWaitEvent(stream, la.ev_fb.get(), 0));
            }
            LaWideArgs& wa = la_held.wa;
            unsigned    g  = la_held.grid;
            if (job != nullptr)
            {
                wa.snap = *job;
                g += 1; // the workgroup that does the copy (la_wide_snapshot)
            }
            if (la_held.k64 && la_held.wt != nullptr)
            {
                hipLaunchKernelGGL(ekf_la_wide_f32_k64m, dim3(g), dim3(128), 0, stream, wa, la_held.wt);
            }
            else if (la_held.k64)
            {
                hipLaunchKernelGGL(ekf_la_wide_f32_k64, dim3(g), dim3(128), 0, stream, wa);
            }
            else
            {
                hipLaunchKernelGGL(ekf_la_wide_f32, dim3(g), dim3(128), 0, stream, wa);
            }
            CSLAM_HIP_TRY(hipGetLastError());
        }
        la_held.valid = false;
        return CSLAM_OK;
    }

    int la_enqueue(const T* dZ, const int* dIdf, int m, const T* R, bool on_device)
    {
        // The first update of a window stays queued after this call returns, and the window reads its inputs when it
        // launches, during a later call.  Device-resident inputs are therefore snapshotted now, on the main stream, into
        // the staging ring: every read of a caller's dZ / d_idf is enqueued during that call (cslam.h).  The snapshot
        // reaches the window's readers like a host-staged copy does: the rows and blocks kernels follow it on the main
        // stream, and the chain kernel on stream F reads Z only after the blocks kernel has released it (or, with
        // several engines, behind that kernel's event).
        //   In the steady state the previous window's wide launch is held (la_launch_held_wide) and is submitted here: it
        // carries the snapshot as a side job of one extra workgroup, so the copy costs no launch of its own.  Only where
        // no wide is held -- the first window after a drain, a predecessor on the classic path, several engines alive,
        // CSLAM_LA_HOLD_WIDE=0 -- does ekf_stage_obs_kernel run (cslam_ekf_stage_launches counts those).  (The stage
        // kernel on stream F with an event wait on the main stream instead measured no faster: DESIGN.md.)
        //   The ring slot of a carried snapshot needs no event.  ring.ev[slot] protects the slot's PINNED HOST half, which
        // the CPU rewrites outside any stream; a carried copy does not touch it (a later host-staged use of the slot still
        // waits for the event of the slot's last host-staged use).  The DEVICE half is protected by stream order alone, as
        // it always was: a slot comes round again StageRing::kSlots stages -- at least 31 windows -- later; its readers were
        // the rows, blocks and wide kernels of its window on the main stream and that window's chain kernel on stream F,
        // which the window's wide kernel waits for (in the kernel, or behind ev_fb) before it ends; and the writer, this
        // window's predecessor's wide kernel, is enqueued on the main stream behind all of them.
        if (on_device && la_n == 0)
        {
            int rc = la_held.valid ? ensure_m(m) : CSLAM_OK; // (a ring that has to grow drains, and submits the held launch)
            if (rc)
            {
                return rc;
            }
            if constexpr (std::is_same<T, float>::value)
            {
                if (la_held.valid)
                {
                    unsigned char* ds = ring.dev_slot(ring.take_slot());
                    LaSnapJob      job;
                    job.Z       = dZ;
                    job.idf     = dIdf;
                    job.Z_out   = reinterpret_cast<T*>(ds);
                    job.idf_out = reinterpret_cast<int*>(ds + (size_t)m * 2 * sizeof(T));
                    job.m       = m;
                    if ((rc = la_launch_held_wide(&job)))
                    {
                        return rc;
                    }
                    dZ       = job.Z_out;
                    dIdf     = job.idf_out;
                    on_device = false; // (staged)
                }
            }
            if (on_device && (rc = stage_obs(dZ, dIdf, m, true, &dZ, &dIdf)))
            {
                return rc;
            }
        }
        // (otherwise nothing is held here: update() submits it in front of a host-staged copy, and a window's second
        // update follows a first one that has submitted it)
        LaUpd u;
        u.dZ   = dZ;
        u.dIdf = dIdf;
        u.m    = m;
        for (int i = 0; i < 4; i++)
        {
            u.R[i] = R[i];
        }
        u.pp     = pp; // the held predict belongs to this update
        pp.valid = 0;
        la_q[la_n++] = u;
        return la_n == 2 ? la_launch_window(true) : CSLAM_OK;
    }

    // the factor kernel's arguments for one update of a window: compact inputs (a local state vector of 3 + 2m entries with
    // local feature ids 1..m and the block sub), outputs into the factor slot f
    FactorArgs<T> la_factor_args(const LaUpd& u, FactorOut& f)
    {
        FactorArgs<T> a;
        a.X   = f.xloc.get();
        a.n   = 3 + 2 * u.m;
        a.Z   = u.dZ;
        a.idf = la.fo[0].idloc.get(); // 1, 2, ... (written once per window by the blocks kernel)
        a.m   = u.m;
        for (int i = 0; i < 4; i++)
        {
            a.R[i] = u.R[i];
        }
        a.PHT      = ws.dPHT.get(); // (not read: the compact block is supplied)
        a.ldw      = ldp;
        a.dS       = f.S.get();
        a.dG       = f.G.get();
        a.dGt      = f.Gt.get();
        a.dV       = f.V.get();
        a.dt       = f.t.get();
        a.flags    = dFlags.get();
        a.scratchS = ws.dScrS.get();
        a.scratchG = ws.dScrG.get();
        a.textbook = (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1;
        a.stamps   = (la.stamps.get() && &f == &la.fo[0]) ? la.stamps.get() : nullptr;
        a.sub      = f.sub.get();
        a.dM       = f.M.get();
        a.pp       = PredictArgs<T>{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, 0}; // (applied by blocks / carry)
        a.P3       = dPv.get();
        a.ldp3     = ldp;
        a.pred_out = nullptr;
        a.lds_S    = 1;
        a.lds_G    = 1;
        return a;
    }

    // gather + gain of one update of the window on the main stream, with the factor outputs of slot f
    int la_wide(const LaUpd& u, const FactorOut& f, hipEvent_t ev_factor)
    {
        const int k = 2 * u.m;
        pp          = u.pp;
        fuse_now    = pp.valid != 0;
        int rc      = CSLAM_OK;
        if (fuse_now && !dPred.get() && (rc = dPred.alloc(16)))
        {
            return rc;
        }
        last_k = k;
        last_counted = false;
        PredictArgs<T> pnone{0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, 0};
        PredictArgs<T> pa   = fuse_now ? pp : pnone;
        T*             pred = fuse_now ? dPred.get() : (T*)nullptr;
        const T*       Wg   = pend.kp > 0 ? (const T*)wbase(pend.wcur) : (const T*)nullptr;
        if (pend.kp > kGatherCorr)
        {
            const dim3 wgrid((n + 255) / 256, (u.m + kGatherObsWide - 1) / kGatherObsWide);
            hipLaunchKernelGGL((ekf_gather_kernel<T, kGatherCorrMax, kGatherObsWide>), wgrid, dim3(256), 0, stream,
                               dX.get(), dP.get(), dPv.get(), ldp, n, u.dZ, u.dIdf, u.m, ws.dPHT.get(), ldp, opt.lower,
                               (T*)nullptr, pa, pred, Wg, ldp, pend.kp, (const int*)nullptr, dFlags.get(), (T*)nullptr);
        }
        else
        {
            const dim3 ggrid((n + 255) / 256, (u.m + kGatherObs - 1) / kGatherObs);
            hipLaunchKernelGGL(ekf_gather_kernel<T>, ggrid, dim3(256), 0, stream, dX.get(), dP.get(), dPv.get(), ldp, n,
                               u.dZ, u.dIdf, u.m, ws.dPHT.get(), ldp, opt.lower, (T*)nullptr, pa, pred, Wg, ldp, pend.kp,
                               (const int*)nullptr, dFlags.get(), (T*)nullptr);
        }
        CSLAM_HIP_TRY(hipGetLastError());
        if (ev_factor != nullptr)
        {
            CSLAM_HIP_TRY(hipStreamWaitEvent(stream, ev_factor, 0));
        }
        T*  slot = wbase(pend.wcur) + (size_t)pend.kp * ldp;
        rc       = launch_gain(k, slot, f.Gt.get(), f.U.get(), f.M.get());
        if (rc)
        {
            return rc;
        }
        pp.valid  = 0;
        fuse_now  = false;
        last_slot = slot;
        pend.appended(k);
        dbgS      = f.S.get();
        dbgGt     = f.Gt.get();
        dbgV      = f.V.get();
        g_from_gt = true;
        sub_valid = false;
        return CSLAM_OK;
    }

    // A window is updates ua and ub; ub is ua again when the window has only one (nu == 1: nothing reads b's share).
    // hold: the wide launch waits for the next call (la_launch_held_wide); update b's caller buffers are then read by the
    // rows and blocks kernels only, the chain kernel and the wide kernel read the copies those keep.
    // The builders of the five argument structs of a window (ekf_lookahead.hpp).  They assign fields and nothing else: no
    // allocation, no HIP call, so none of them can fail (la_launch_window relies on it).
    LaChainArgs<T> la_chain_args(const LaUpd& ua, const LaUpd& ub, int nu, bool hold, unsigned target, unsigned seq)
    {
        LaChainArgs<T> ch;
        ch.fa = la_factor_args(ua, la.fo[0]);
        ch.fb = la_factor_args(ub, la.fo[1]);
        if (hold)
        {
            ch.fb.Z = la.z_keep.get();
        }
        ch.du_a       = la.fo[0].U.get();
        ch.du_b       = la.fo[1].U.get();
        ch.nu         = nu;
        ch.done       = la.done.get();
        ch.target     = target;
        ch.timeout    = 20000000ull; // 0.2 s of s_memrealtime ticks
        ch.chain_done = la.done.get() + 256;
        ch.seq        = seq;
        LaCarryArgs<T>& ca = ch.ca;
        ca.n       = n;
        ca.m_a     = ua.m;
        ca.m_b     = nu == 2 ? ub.m : 0;
        ca.idf_b   = hold ? la.idf_keep.get() : ub.dIdf;
        ca.pp_b    = ub.pp;
        ca.PH      = la.PH.get();
        ca.Dbb     = la.Dbb.get();
        ca.PvLb    = la.PvLb.get();
        ca.XLb     = la.XL.get() + 2 * ua.m;
        ca.model_a = la.model.get();
        ca.Gt_a    = la.fo[0].Gt.get();
        ca.u_a     = la.fo[0].U.get();
        ca.M_a     = la.fo[0].M.get();
        ca.sub_a   = la.fo[0].sub.get();
        ca.sub_b   = la.fo[1].sub.get();
        ca.xloc_b  = la.fo[1].xloc.get();
        ca.model_b = la.model.get() + 1;
        ca.Y_b     = la.Y.get();
        return ch;
    }
    LaRowsArgs<T> la_rows_args(const LaUpd& ua, const LaUpd& ub, int nu, bool hold)
    {
        LaRowsArgs<T> ra;
        ra.X     = dX.get();
        ra.Pv    = dPv.get();
        ra.ldp   = ldp;
        ra.n     = n;
        ra.idf_a = ua.dIdf;
        ra.ra    = 2 * ua.m;
        ra.idf_b = ub.dIdf;
        ra.rb    = nu == 2 ? 2 * ub.m : 0;
        ra.Wp    = wbase(pend.wcur);
        ra.ldw   = ldp;
        ra.kp    = pend.kp;
        ra.kpad  = la_kpad;
        ra.XL    = la.XL.get();
        ra.PvL   = la.PvL.get();
        ra.WR    = la_WR.get();
        ra.flags = dFlags.get();
        ra.idf_b_keep = hold ? la.idf_keep.get() : (int*)nullptr;
        ra.Z_b        = ub.dZ;
        ra.Z_b_keep   = hold ? la.z_keep.get() : (T*)nullptr;
        return ra;
    }
    // pg_signal: the P-GEMM launch that follows releases the chain, not the blocks kernel's own workgroups
    LaPrepArgs<T> la_prep_args(const LaUpd& ua, const LaUpd& ub, int nu, bool hold, bool pg_signal)
    {
        LaPrepArgs<T> pa;
        pa.P       = dP.get();
        pa.ldp     = ldp;
        pa.n       = n;
        pa.lower   = opt.lower;
        pa.X       = dX.get();
        pa.Pv      = dPv.get();
        pa.idf_a   = ua.dIdf;
        pa.idf_b   = ub.dIdf;
        pa.ra      = 2 * ua.m;
        pa.rb      = nu == 2 ? 2 * ub.m : 0;
        pa.pp_a    = ua.pp;
        pa.XL      = la.XL.get();
        pa.PvL     = la.PvL.get();
        pa.WR      = la_WR.get();
        pa.kp      = pend.kp;
        pa.kpad    = la_kpad;
        pa.sub_a   = la.fo[0].sub.get();
        pa.PH      = la.PH.get();
        pa.Dbb     = la.Dbb.get();
        pa.PvLb    = la.PvLb.get();
        pa.model_a = la.model.get();
        pa.xloc_a  = la.fo[0].xloc.get();
        pa.idloc   = la.fo[0].idloc.get();
        pa.done    = pg_signal ? (unsigned*)nullptr : la.done.get();
        return pa;
    }
    // (f32 only, as the two builders below: what the mirror form of the blocks kernel does in the rows kernel's place)
    LaMirrorArgs la_mirror_args(const LaUpd& ua, const LaUpd& ub, int nu, bool hold)
    {
        LaMirrorArgs mi;
        mi.WT         = la_WT.get();
        mi.XLb        = la.XL.get() + 2 * ua.m;
        mi.flags      = dFlags.get();
        mi.idf_b_keep = hold ? la.idf_keep.get() : (int*)nullptr;
        mi.Z_b        = ub.dZ;
        mi.Z_b_keep   = hold ? la.z_keep.get() : (float*)nullptr;
        return mi;
    }
    // (the window's panels go behind the pend.kp pending columns; la_seq is the window's chain kernel)
    LaWideArgs la_wide_args(const LaUpd& ua, const LaUpd& ub, int nu, bool hold)
    {
        LaWideArgs wa;
        wa.chain_done = la.done.get() + 256; // (waits for the chain kernel in the kernel: a stream event costs ~6 us here)
        wa.seq        = la_seq;
        wa.timeout    = 20000000ull;
        wa.flags      = dFlags.get();
        wa.stamps     = la.stamps.get() ? la.stamps.get() + 16 : nullptr;
        wa.wg_times   = nullptr;
        wa.P       = dP.get();
        wa.ldp     = ldp;
        wa.n       = n;
        wa.lower   = opt.lower;
        wa.X       = dX.get();
        wa.Pv      = dPv.get();
        wa.nu      = nu;
        wa.idf_a   = ua.dIdf;
        wa.idf_b   = hold ? la.idf_keep.get() : ub.dIdf;
        wa.ma      = ua.m;
        wa.mb      = nu == 2 ? ub.m : 0;
        wa.valid_a = ua.pp.valid;
        wa.valid_b = nu == 2 ? ub.pp.valid : 0;
        wa.w_a     = ua.pp.w;
        wa.w_b     = nu == 2 ? ub.pp.w : 0;
        wa.model_a = la.model.get();
        wa.model_b = la.model.get() + 1;
        wa.Gt_a    = la.fo[0].Gt.get();
        wa.u_a     = la.fo[0].U.get();
        wa.M_a     = la.fo[0].M.get();
        wa.sub_a   = la.fo[0].sub.get();
        wa.Gt_b    = la.fo[1].Gt.get();
        wa.u_b     = la.fo[1].U.get();
        wa.M_b     = la.fo[1].M.get();
        wa.sub_b   = la.fo[1].sub.get();
        wa.Y_b     = la.Y.get();
        wa.W1a     = wbase(pend.wcur) + (size_t)pend.kp * ldp;
        wa.W1b     = wa.W1a + (size_t)2 * ua.m * ldp;
        wa.ldw     = ldp;
        wa.wv_out  = ws.dWv.get();
        wa.snap    = LaSnapJob{nullptr, nullptr, nullptr, nullptr, 0};
        return wa;
    }

    // may_hold: the caller is the update that completes the window (la_enqueue), so the wide launch may wait for the next call
    int la_launch_window(bool may_hold = false)
    {
        if (la_n == 0)
        {
            return CSLAM_OK;
        }
        const int   nu = la_n;
        const LaUpd ua = la_q[0], ub = la_q[nu - 1]; // (one update: b is a again, and nothing reads b's share)
        const int   ka = 2 * ua.m, kb = nu == 2 ? 2 * ub.m : 0;
        la_n = 0; // (no wide launch is held here: the call that queued update a has submitted it)
        const PredictArgs<T> held = pp; // a predict accepted AFTER the queued updates stays held
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if (pend.kp > 256 && (rc = flush())) // (the blocks kernel stages one row of at most 256 pending columns)
        {
            return rc;
        }
        if ((rc = ensure_k(2 * kLaMaxObs)) || (rc = ensure_w(ka + kb)) || (rc = la_ensure(pend.kp)))
        {
            return rc;
        }
        // (the P-GEMM's tile list is (re)built here, not inside the launch below: building it waits for both streams, and
        // from the chain launch on stream F waits for a go-ahead that only that P-GEMM launch delivers)
        if (opt.lower && (rc = ensure_tile_list(round_up(n, kTile) / kTile)))
        {
            return rc;
        }
        // 1. the factor chain of the window on stream F, ONE launch, submitted first: it takes a compute unit for itself
        //    and waits there (on a counter) for the blocks kernel below.  (safe: several engines alive -- the chain kernel is
        //    launched behind the blocks kernel's event instead, see g_engines)
        const bool safe = g_engines.load() > 1;
        const unsigned n_blocks = (unsigned)(3 + ka + 2 * kb);
        const bool hold = may_hold && opt.la_hold_wide && opt.la_fused && !safe && nu == 2 && std::is_same<T, float>::value &&
                 !la.stamps.get();
        auto launch_chain = [&]() -> int {
            const LaChainArgs<T> ch = la_chain_args(ua, ub, nu, hold, la_target + n_blocks, ++la_seq);
            if (std::max(ka, kb) <= 32)
            {
                hipLaunchKernelGGL((ekf_la_chain_kernel<T, 32>), dim3(1), dim3(256), la_chain_lds<T>(32), stream_f, ch);
            }
            else
            {
                hipLaunchKernelGGL((ekf_la_chain_kernel<T, 64>), dim3(1), dim3(256), la_chain_lds<T>(64), stream_f, ch);
            }
            CSLAM_HIP_TRY(hipGetLastError());
            CSLAM_HIP_TRY(hipEventRecord(la.ev_fb.get(), stream_f));
            return CSLAM_OK;
        };
        if (!safe && (rc = launch_chain()))
        {
            return rc;
        }
        // 2. what the chain needs of the current covariance P = Ps - Wp Wp^T (before Ps changes): rows of the pending
        //    panels, then one workgroup per row of the small blocks; update a's compact block sub_a comes out of it ready
        //    for the factor step.  The chain kernel is waiting: nothing may fail from here to the blocks launch, and
        //    nothing can -- only argument builders stand in between.
        //    The mirror form of the blocks kernel needs no rows kernel: when the mirror covers every pending column, or
        //    there is none.
        bool use_mirror = false;
        if constexpr (std::is_same<T, float>::value)
        {
            use_mirror = opt.la_mirror &&
                         (pend.kp == 0 || (pend.mirror_covers(pend.kp, n) && pend.kp <= 128 && pend.kp % 4 == 0));
        }
        // the P-GEMM that follows signals the chain when it is the plain single-stream psym4 launch (always in the steady state);
        // otherwise the blocks kernel's workgroups release their rows themselves
        const int  k8f       = round_up(pend.kp, 8);
        const bool pg_signal = !opt.la_wg_signal && !safe && pend.kp > 0 && seq.count == 0 && sizeof(T) == 4 && k8f <= 128 &&
                               opt.lower && ldp < 32768 && !limbs_take(k8f) && stream_b == stream &&
                               pend.hd_cols[pend.wcur] == 0;
        if constexpr (std::is_same<T, float>::value)
        {
            if (use_mirror)
            {
                hipLaunchKernelGGL(ekf_la_blocks_mirror_kernel, dim3(n_blocks), dim3(256), 0, stream,
                                   la_prep_args(ua, ub, nu, hold, pg_signal), la_mirror_args(ua, ub, nu, hold));
            }
        }
        if (!use_mirror)
        {
            hipLaunchKernelGGL(ekf_la_rows_kernel<T>, dim3(ka + kb), dim3(128), 0, stream, la_rows_args(ua, ub, nu, hold));
            rows_launches++;
            hipLaunchKernelGGL(ekf_la_blocks_kernel<T>, dim3(n_blocks), dim3(64), 0, stream, la_prep_args(ua, ub, nu, hold, pg_signal));
        }
        CSLAM_HIP_TRY(hipGetLastError());
        if (safe)
        {
            CSLAM_HIP_TRY(hipEventRecord(la.ev_raw.get(), stream));
            CSLAM_HIP_TRY(hipStreamWaitEvent(stream_f, la.ev_raw.get(), 0));
            if ((rc = launch_chain())) // (its wait for the blocks kernel's counters passes at once)
            {
                return rc;
            }
        }
        la_target += n_blocks;
        // 3. the P-GEMM of everything pending (the previous window's panels): stream F works underneath it
        la_sig_add = pg_signal ? n_blocks : 0u;
        rc         = flush();
        if (la_sig_add != 0) // (the launch did not happen: release the chain from here -- it times out otherwise)
        {
            const unsigned add = la_sig_add;
            la_sig_add         = 0;
            hipLaunchKernelGGL(ekf_la_signal_kernel, dim3(1), dim3(64), 0, stream, la.done.get(), add);
        }
        if (rc)
        {
            return rc;
        }
        // 4. the wide half of both updates, factors known: ONE launch in f32 (ekf_la_wide_f32), gather + gain per update
        //    otherwise (CSLAM_LA_FUSED=0: A/B)
        bool fused = false;
        if constexpr (std::is_same<T, float>::value)
        {
            if (opt.la_fused)
            {
                fused = true;
                // (several engines alive: la_launch_held_wide puts the wait for ev_fb in front of the launch)
                la_held.wa  = la_wide_args(ua, ub, nu, hold);
                la_held.k64 = opt.la_k64 && ua.m == 32 && ub.m == 32;
                // (the mirror's column q is the store's column q: the panels must start at column 0 of the store)
                la_held.wt = (opt.la_mirror && la_held.k64 && pend.kp == 0) ? la_WT.get() : nullptr;
                pend.mirror_written(la_held.wt ? ka + kb : 0, n);
                la_held.grid  = (unsigned)(round_up(n, kTile) / 32);
                la_held.valid = true;
                if (!hold && (rc = la_launch_held_wide(nullptr)))
                {
                    return rc;
                }
                last_slot = nullptr; // (PHT is not materialised on this path: nothing for debug_last_update)
                last_k    = 0;
                pend.appended(ka + kb);
                sub_valid = false;
            }
        }
        if (!fused && ((rc = la_wide(ua, la.fo[0], la.ev_fb.get())) || (nu == 2 && (rc = la_wide(ub, la.fo[1], nullptr)))))
        {
            return rc;
        }
        pp = held;
        la_windows++;
        return (la.stamps.get() && la_windows == 300) ? la_report_stamps() : CSLAM_OK;
    }

    // CSLAM_LA_STAMPS: where factor(a) and the wide kernel spent their time, once, after 300 windows
    int la_report_stamps()
    {
        long long h[32];
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        CSLAM_HIP_TRY(hipMemcpy(h, la.stamps.get(), sizeof(h), hipMemcpyDeviceToHost));
        fprintf(stderr, "[cslam la wide stamps, 10 ns ticks] ids+columns issue:%lld poll+DMA wait:%lld pht_a:%lld gain_a:%lld store+share W1_a:%lld pht_b+corr:%lld share+G_b:%lld gain_b:%lld store_b:%lld\n",
                h[17] - h[16], h[18] - h[17], h[19] - h[18], h[20] - h[19], h[21] - h[20], h[22] - h[21], h[23] - h[22],
                h[24] - h[23], h[25] - h[24]);
        fprintf(stderr, "[cslam la stamps, cycles] load+observe:%lld sums:%lld symmetrise:%lld cholesky:%lld (first half %lld) inverse:%lld outputs:%lld total:%lld\n",
                h[6] - h[0], h[7] - h[6], h[1] - h[7], h[2] - h[1], h[5] ? h[5] - h[1] : 0, h[3] - h[2], h[4] - h[3], h[4] - h[0]);
        return CSLAM_OK;
    }

    // every call that needs the state as of the last update() goes through here first
    int la_drain() override { return la_n ? la_launch_window() : la_launch_held_wide(nullptr); }

    int update(const void* Zv, int m, const void* Rv, const int* idf, int batch, bool on_device) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Zv || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "update: bad arguments (m=%d)", m);
        }
        if (m == 0)
        {
            return CSLAM_OK; // EKF.cpp:101-123 with an empty Z: nothing changes
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        const T*   R    = static_cast<const T*>(Rv);
        const T*   dZ   = static_cast<const T*>(Zv);
        const int* dIdf = idf;
        if (!on_device)
        {
            const int nf = (n - 3) / 2;
            for (int i = 0; i < m; i++)
            {
                if (idf[i] < 1 || idf[i] > nf)
                {
                    return fail(CSLAM_ERR_BAD_ARG, "update: idf[%d]=%d outside 1..%d", i, idf[i], nf);
                }
            }
            // (a held wide launch keeps its place on the main stream: in front of this update's copy)
            if ((rc = la_launch_held_wide(nullptr)) || (rc = stage_obs(Zv, idf, m, false, &dZ, &dIdf)))
            {
                return rc;
            }
        }
        if (batch && la_eligible(m))
        {
            return la_enqueue(dZ, dIdf, m, R, on_device);
        }
        if ((rc = la_drain())) // (the held predict of THIS call survives the drain: la_launch_window keeps it)
        {
            return rc;
        }
        if (batch)
        {
            return batch_on_device(dZ, dIdf, m, R, false);
        }
        if ((rc = resolve_predict()))
        {
            return rc;
        }
        // EKF.cpp:457-479: m successive rank-2 updates, relinearised on the updated state each time.  Their m
        // rank-2 downdates stay pending and are applied by ONE P-GEMM with k = 2m: each observation reads the columns
        // it needs as Ps[:,c] - Wp*Wp[c,:]^T.
        if (opt.seq_defer)
        {
            // (every rank-2 slot is written as a block of 8 columns: the last one reaches column kp + 2m + 6)
            if ((rc = ensure_w(2 * m + 8)))
            {
                return rc;
            }
            if (pend.kp + 2 * m + 6 > pend.wcap && (rc = flush()))
            {
                return rc;
            }
        }
        kp_call_limit = opt.seq_defer ? pend.kp + 2 * m : 0;
        for (int i = 0; i < m; i++)
        {
            if ((rc = batch_on_device(dZ + 2 * i, dIdf + i, 1, R, opt.seq_defer != 0)))
            {
                kp_call_limit = 0;
                return rc;
            }
        }
        kp_call_limit = 0;
        if (!opt.pipeline && defer_max == 0 && (rc = flush()))
        {
            return rc;
        }
        return CSLAM_OK;
    }

    // ---------------------------------------------------------------- augment (EKF.cpp:9-91)
    int augment(const void* Zv, int q, const void* Rv) override
    {
        if (q < 0 || !Rv || (q > 0 && !Zv))
        {
            return fail(CSLAM_ERR_BAD_ARG, "augment: bad arguments (q=%d)", q);
        }
        if (n + 2 * q > ncap)
        {
            return fail(CSLAM_ERR_CAPACITY, "augment: %d features would exceed max_landmarks=%d", (n - 3) / 2 + q, nmax);
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if (q > 0 && (rc = wait_pgemm())) // the new rows / columns of Ps are written here: no P-GEMM may be sweeping it
        {
            return rc;
        }
        const T* Z = static_cast<const T*>(Zv);
        const T* R = static_cast<const T*>(Rv);
        for (int i = 0; i < q; i++)
        {
            // (pending panels: their rows for the new feature are zero, which is right -- the kernel writes values of
            // the true P, built from the pose stripe)
            hipLaunchKernelGGL(ekf_augment_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, stream, dX.get(), dP.get(),
                               dPv.get(), ldp, n, Z[2 * i], Z[2 * i + 1], R[0], R[1], R[2], R[3], opt.lower);
            CSLAM_HIP_TRY(hipGetLastError());
            augment_launches++;
            n += 2;
        }
        return CSLAM_OK;
    }

    // The same with Z in device memory, read in stream order: kAugChunk features per launch (ekf_augment_kernels.hpp).
    // A later chunk finds the rows of the earlier ones in the stripe, as a later call would.
    int augment_device(const void* dZv, int q, const void* Rv) override
    {
        if (q < 0 || !Rv || (q > 0 && !dZv))
        {
            return fail(CSLAM_ERR_BAD_ARG, "augment_device: bad arguments (q=%d)", q);
        }
        if (n + 2 * q > ncap)
        {
            return fail(CSLAM_ERR_CAPACITY, "augment_device: %d features would exceed max_landmarks=%d", (n - 3) / 2 + q,
                        nmax);
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if (q > 0 && (rc = wait_pgemm())) // (as augment)
        {
            return rc;
        }
        const T* dZ = static_cast<const T*>(dZv);
        const T* R  = static_cast<const T*>(Rv);
        for (int i = 0; i < q; i += kAugChunk)
        {
            const int qc = std::min(q - i, kAugChunk);
            hipLaunchKernelGGL(ekf_augment_many_kernel<T>, dim3((n + 3 * qc + 255) / 256), dim3(256), 0, stream, dX.get(),
                               dP.get(), dPv.get(), ldp, n, dZ + 2 * i, qc, R[0], R[1], R[2], R[3], opt.lower);
            CSLAM_HIP_TRY(hipGetLastError());
            augment_launches++;
            n += 2 * qc;
        }
        return CSLAM_OK;
    }

    // ---------------------------------------------------------------- heading (EKF.cpp:328-352)
    int observe_heading(double phi, int use) override
    {
        if (!use)
        {
            return CSLAM_OK; // EKF.cpp:332-335 (a pending predict stays pending)
        }
        // float sigmaPhi = 0.01F * pi / 180.0F; R = pow(sigmaPhi, 2)
        T   sigma = (T)(((double)0.01f * kPi) / 180.0);
        int rc    = queue_step(pp, HeadingArgs<T>{1, (T)phi, sigma * sigma}); // with the held predict, if any
        if (rc || opt.fuse_predict)
        {
            return rc;
        }
        return launch_pose_queue();
    }

    int factor_status(int* flags, int clear) override
    {
        if (!flags)
        {
            return fail(CSLAM_ERR_BAD_ARG, "factor_status: null");
        }
        int rc = use_device();
        if (rc || (rc = la_drain()))
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(hFlags.get(), dFlags.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        int f = sticky_host;
        if (hFlags[0] & kFlagZeroed)
        {
            f |= CSLAM_FACTOR_ZEROED;
        }
        if (hFlags[0] & kFlagBadIdf)
        {
            f |= CSLAM_FACTOR_BAD_IDF;
        }
        if (hFlags[0] & kFlagLaTimeout)
        {
            f |= CSLAM_FACTOR_INTERNAL;
        }
        if (hFlags[0] & kFlagCountClamped)
        {
            f |= CSLAM_FACTOR_COUNT_CLAMPED;
        }
        if ((hFlags[0] & kFlagLltFailed) && !(sticky_host & CSLAM_FACTOR_FALLBACK))
        {
            f |= CSLAM_FACTOR_SKIPPED; // async mode: the failed factorisation was not followed up
        }
        *flags = f;
        if (clear)
        {
            sticky_host = 0;
            CSLAM_HIP_TRY(hipMemsetAsync(dFlags.get(), 0, 2 * sizeof(int), stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        }
        return CSLAM_OK;
    }

    int set_deferred(int max_cols) override
    {
        if (max_cols < 0)
        {
            return fail(CSLAM_ERR_BAD_ARG, "set_deferred: negative");
        }
        int rc = flush();
        if (rc)
        {
            return rc;
        }
        defer_max = max_cols;
        return max_cols > 0 ? ensure_w(max_cols + 64) : CSLAM_OK;
    }

    int do_flush() override { return flush(); }

    int debug_last_update(void* PHT, void* S, void* G, void* W1, void* V, int* kout) override
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if (last_slot && last_counted) // (its k = 2 * count was only ever known on the device)
        {
            return fail(CSLAM_ERR_BAD_ARG, "debug_last_update: the last update was a counted one");
        }
        const int k = last_slot ? last_k : 0;
        if (kout)
        {
            *kout = k;
        }
        if (k == 0)
        {
            return CSLAM_OK;
        }
        if (PHT)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(PHT, (size_t)n * sizeof(T), ws.dPHT.get(), (size_t)ldp * sizeof(T),
                                           (size_t)n * sizeof(T), (size_t)k, hipMemcpyDeviceToHost, stream));
        }
        if (W1)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(W1, (size_t)n * sizeof(T), last_slot, (size_t)ldp * sizeof(T),
                                           (size_t)n * sizeof(T), (size_t)k, hipMemcpyDeviceToHost, stream));
            // its pose rows were zeroed in the store after the pose stripe took its share (ekf_pose_downdate_kernel
            // saved them): rows 0..2 <- dWv (3 x k, row c at c*k)
            CSLAM_HIP_TRY(hipMemcpy2DAsync(W1, (size_t)n * sizeof(T), ws.dWv.get(), sizeof(T), sizeof(T), (size_t)k,
                                           hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipMemcpy2DAsync(static_cast<T*>(W1) + 1, (size_t)n * sizeof(T), ws.dWv.get() + k, sizeof(T),
                                           sizeof(T), (size_t)k, hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipMemcpy2DAsync(static_cast<T*>(W1) + 2, (size_t)n * sizeof(T), ws.dWv.get() + 2 * k,
                                           sizeof(T), sizeof(T), (size_t)k, hipMemcpyDeviceToHost, stream));
        }
        if (S)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(S, dbgS ? dbgS : ws.dS.get(), (size_t)k * k * sizeof(T), hipMemcpyDeviceToHost,
                                         stream));
        }
        if (G && !g_from_gt)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(G, ws.dG.get(), (size_t)k * k * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        if (G && g_from_gt) // the tuned factor kernels publish only G^T (what the gain kernel reads)
        {
            std::vector<T> Gt((size_t)k * k);
            CSLAM_HIP_TRY(hipMemcpyAsync(Gt.data(), dbgGt ? dbgGt : ws.dGt.get(), Gt.size() * sizeof(T),
                                         hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            T* out = static_cast<T*>(G);
            for (int c = 0; c < k; c++)
            {
                for (int r = 0; r < k; r++)
                {
                    out[(size_t)c * k + r] = Gt[(size_t)r * k + c];
                }
            }
        }
        if (V)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(V, dbgV ? dbgV : ws.dV.get(), (size_t)k * sizeof(T), hipMemcpyDeviceToHost,
                                         stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }
};

// lower-triangular tile list (ti >= tj), column-of-tiles major so that consecutive entries share the column
// panel; rebuilt when the number of 128-row tiles changes (n grew past a tile boundary)
template <typename T>
int Ekf<T>::ensure_tile_list(int tiles)
{
    if (tiles != tiles_built)
    {
        std::vector<int2> h;
        h.reserve((size_t)tiles * (tiles + 1) / 2);
        for (int tj = 0; tj < tiles; tj++)
        {
            for (int ti = tj; ti < tiles; ti++)
            {
                h.push_back(make_int2(ti, tj));
            }
        }
        if (int rc = sync_all()) // (a P-GEMM in flight still reads the old list)
        {
            return rc;
        }
        DevBuf<int2> list;
        CSLAM_TRY(list.alloc(h.size()));
        dTiles = std::move(list);
        CSLAM_HIP_TRY(hipMemcpy(dTiles.get(), h.data(), h.size() * sizeof(int2), hipMemcpyHostToDevice));
        tiles_built = tiles;
        n_sym_tiles = (int)h.size();
    }
    // the tail phase's lists: they also depend on the grid and on how many 32-row strips of the last tile row hold
    // rows below n
    if (sizeof(T) != 4 || opt.pgemm_tail == 0 || !opt.lower)
    {
        return CSLAM_OK;
    }
    const int G     = pgemm_grid();
    const int valid = pgemm_valid_strips(tiles, n);
    if (tiles == work_tiles && valid == work_valid && G == work_grid)
    {
        return CSLAM_OK;
    }
    PgemmWork w[3];
    bool      any = false;
    for (int c = 0; c < 3; c++)
    {
        // (a forced count leaves one tile whole: a workgroup enters the tail phase from the whole-tile loop)
        w[c] = pgemm_build_work(tiles, n, G, c, std::min(opt.pgemm_tail, n_sym_tiles - 1));
        any  = any || w[c].strips > 0 || work_strips[c] > 0;
    }
    if (any)
    {
        if (int rc = sync_all()) // (a P-GEMM in flight still reads the old lists)
        {
            return rc;
        }
    }
    for (int c = 0; c < 3; c++)
    {
        static_assert(sizeof(PgemmEntry) == sizeof(int2), "a work-list entry is an int2");
        DevBuf<int2> list;
        if (w[c].strips > 0)
        {
            CSLAM_TRY(list.alloc(w[c].list.size()));
            CSLAM_HIP_TRY(hipMemcpy(list.get(), w[c].list.data(), w[c].list.size() * sizeof(int2), hipMemcpyHostToDevice));
        }
        dWork[c]       = std::move(list);
        work_whole[c]  = w[c].strips > 0 ? w[c].whole : 0;
        work_strips[c] = w[c].strips;
    }
    work_tiles = tiles;
    work_valid = valid;
    work_grid  = G;
    return CSLAM_OK;
}

// workgroups of the persistent P-GEMM grid: two per CU, minus `pgemm_spare` in two-stream mode -- a few CUs keep one
// workgroup (64 of 160 KB LDS) so that the one-workgroup factor kernel of the NEXT update (53 KB LDS, stream A) finds
// room while this P-GEMM fills the chip; look-ahead windows: the main stream's queue mask excludes the compute units
// of the factor chain's stream (la_cus, see la_ensure)
template <typename T>
int Ekf<T>::pgemm_grid() const
{
    int G = std::min(n_sym_tiles, std::max(1, 2 * (num_cus - la_cus) - (opt.pipeline ? opt.pgemm_spare : 0)));
    if (pgemm_wgs > 0)
    {
        G = std::min(G, pgemm_wgs);
    }
    return G;
}

template <>
int Ekf<float>::launch_downdate(const float* W, int k, hipStream_t stream)
{
    const int tiles = round_up(n, kTile) / kTile;
    const int k8    = round_up(k, 8); // W columns [k, k8) are zero where the kernel reads them (flush() clears the tail)
    // persistent symmetric kernels over the list of lower-triangular tiles; mirror stores only under full storage
    int rc = ensure_tile_list(tiles);
    if (rc)
    {
        return rc;
    }
    const dim3 block(256);
    int G = pgemm_grid(); // the persistent grid
    const bool nt = opt.psym_nt >= 0 ? opt.psym_nt != 0 : (size_t)n_sym_tiles * 65536 > ((size_t)230 << 20);
    if (limbs_take(k8))
    {
        // f32 products as exact bf16 limb products on the bf16 matrix cores (ekf_pgemm_limbs.hpp)
        const int    nch  = k8 <= 64 ? 4 : (k8 <= 96 ? 6 : (k8 <= 128 ? 8 : (k8 <= 192 ? 12 : 16)));
        const int    kgs  = 2 * nch;
        const int    rows = round_up(n, kTile);
        const size_t need = (size_t)2 * 3 * kgs * rows * 16;
        if (need > wb_bytes)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // (grows with n and the window: rare)
            const size_t  cap = (size_t)2 * 3 * 32 * round_up(ncap, kTile) * 16; // every window up to 256 columns
            DevBuf<uint4> wb;
            CSLAM_TRY(wb.alloc(cap / sizeof(uint4)));
            dWb      = std::move(wb);
            wb_bytes = cap;
        }
        if ((rc = ensure_tiles_morton(tiles, stream)))
        {
            return rc;
        }
        hipLaunchKernelGGL(ekf_limb_split_kernel, dim3((rows + 255) / 256, kgs), dim3(256), 0, stream, W, ldp, k, rows, kgs,
                           dWb.get());
        // (ring of 3 panel buffers, 72 KB: two workgroups per compute unit)
        limb_parity ^= 1;
#define CSLAM_LAUNCH_PSYM5(MODE, NCH, NP, RR)                                                                          \
    do                                                                                                                 \
    {                                                                                                                  \
        static bool attr_set = false;                                                                                  \
        if (!attr_set)                                                                                                 \
        {                                                                                                              \
            CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_downdate_psym5_bf16<MODE, NCH, NP, RR>), \
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));               \
            attr_set = true;                                                                                           \
        }                                                                                                              \
        hipLaunchKernelGGL((ekf_downdate_psym5_bf16<MODE, NCH, NP, RR>), dim3(G), block, (size_t)RR * 24576, stream, dP.get(), ldp, \
                           (const uint4*)dWb.get(), rows, (const int2*)dTilesM.get(), (const int*)dSegOff.get(), dTicketX.get() + 8 * limb_parity,  \
                           dTicketX.get() + 8 * (limb_parity ^ 1));                                                          \
    } while (0)
#define CSLAM_LAUNCH_PSYM5R(NCH, RR)                                                                                   \
    do                                                                                                                 \
    {                                                                                                                  \
        if (opt.pgemm_limbs == 6)                                                                                          \
        {                                                                                                              \
            if (nt) { CSLAM_LAUNCH_PSYM5(1, NCH, 6, RR); } else { CSLAM_LAUNCH_PSYM5(0, NCH, 6, RR); }                 \
        }                                                                                                              \
        else                                                                                                           \
        {                                                                                                              \
            if (nt) { CSLAM_LAUNCH_PSYM5(1, NCH, 9, RR); } else { CSLAM_LAUNCH_PSYM5(0, NCH, 9, RR); }                 \
        }                                                                                                              \
    } while (0)
        switch (nch)
        {
        case 4: CSLAM_LAUNCH_PSYM5R(4, 3); break;
        case 6: CSLAM_LAUNCH_PSYM5R(6, 3); break;
        case 8: CSLAM_LAUNCH_PSYM5R(8, 3); break;
        case 12: CSLAM_LAUNCH_PSYM5R(12, 3); break;
        default: CSLAM_LAUNCH_PSYM5R(16, 3); break;
        }
#undef CSLAM_LAUNCH_PSYM5R
#undef CSLAM_LAUNCH_PSYM5
    }
    else if (k8 <= 128 && opt.lower && ldp < 32768)
    {
        // the shipped P-GEMM: every memory operation interleaved with the MFMA loop; two chunks of 32 columns (k <= 64),
        // four of 24 (k <= 96) or four of 32 (k <= 128)
        launch_parity++;
        // per-XCD tile queues (see the kernel): env CSLAM_XCD_QUEUES (every queue needs workgroups: small grids stay on
        // the single queue)
        const bool xq = opt.xcd_queues != 0 && G >= 64;
        // the tail phase (single queue only): this chunk class's list of whole tiles and strips in place of dTiles
        const int   cc      = pgemm_chunk_class(k8);
        const bool  tail    = !xq && work_strips[cc] > 0;
        const int2* wl      = tail ? (const int2*)dWork[cc].get() : (const int2*)dTiles.get();
        const int   n_whole = tail ? work_whole[cc] : n_sym_tiles;
        const int   n_strip = tail ? work_strips[cc] : 0;
        if (tail)
        {
            G = std::min(G, n_whole); // (the list was built for pgemm_grid(); every workgroup starts with a whole tile)
        }
        split_whole         = n_whole;
        split_strips        = n_strip;
        if (xq)
        {
            if ((rc = ensure_tiles_morton(tiles, stream)))
            {
                return rc;
            }
            limb_parity ^= 1;
        }
#define CSLAM_LAUNCH_PSYM4(MODE, NCH, KC)                                                                             \
    hipLaunchKernelGGL((ekf_downdate_psym4_f32<MODE, NCH, KC>), dim3(G), block, 0, stream, dP.get(), ldp, W, ldp, k,         \
                       xq ? (const int2*)dTilesM.get() : wl, n_whole,                                                             \
                       xq ? dTicketX.get() + 8 * limb_parity : dTicket.get() + (launch_parity & 1),                              \
                       xq ? dTicketX.get() + 8 * (limb_parity ^ 1) : dTicket.get() + ((launch_parity + 1) & 1),                  \
                       (unsigned long long*)nullptr, xq ? (const int*)dSegOff.get() : (const int*)nullptr, 0u, 0u, 0u, 0u,           \
                       la_sig_add ? la.done.get() : (unsigned*)nullptr, la_sig_add, 1, 0, n_strip)
        if (k8 <= 64)
        {
            if (nt) { CSLAM_LAUNCH_PSYM4(1, 2, 32); } else { CSLAM_LAUNCH_PSYM4(0, 2, 32); }
        }
        else if (k8 <= 96)
        {
            if (nt) { CSLAM_LAUNCH_PSYM4(1, 4, 24); } else { CSLAM_LAUNCH_PSYM4(0, 4, 24); }
        }
        else
        {
            if (nt) { CSLAM_LAUNCH_PSYM4(1, 4, 32); } else { CSLAM_LAUNCH_PSYM4(0, 4, 32); }
        }
#undef CSLAM_LAUNCH_PSYM4
        la_sig_add = 0; // (delivered)
    }
    else if (opt.lower)
    {
        // any k, block-lower storage: the unpipelined persistent symmetric kernel (windows beyond 128 columns)
        hipLaunchKernelGGL((ekf_downdate_psym_f32<64, true, false>), dim3(G), block, 0, stream, dP.get(), ldp, W, ldp,
                           k8, dTiles.get(), n_sym_tiles, (long long*)nullptr);
    }
    else
    {
        // full storage (CSLAM_STORAGE=full): the same kernel with mirror stores
        hipLaunchKernelGGL((ekf_downdate_psym_f32<64, true, true>), dim3(G), block, 0, stream, dP.get(), ldp, W, ldp,
                           k8, dTiles.get(), n_sym_tiles, (long long*)nullptr);
    }
    CSLAM_HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

template <>
bool Ekf<float>::launch_gain_fast(int k, int n_pad, float* slot, const float* Gt, const float* U, const float* M)
{
    if (k > 128)
    {
        return false; // u is produced by the tuned factor kernels only
    }
    hipLaunchKernelGGL((ekf_panel_mfma_f32<false, true>), dim3(n_pad / 32, (k + 31) / 32), dim3(64), 0, stream,
                       ws.dPHT.get(), ldp, n, k, k, Gt, k, U, slot, ldp, dX.get(),
                       fuse_now ? (const float*)dPred.get() : (const float*)nullptr, pp.w, dPv.get(), ldp, M,
                       ws.dWv.get());
    pose_fused_in_gain = (M != nullptr);
    return true;
}

template <>
bool Ekf<float>::launch_corr_fast(int k, const float* Wp, int kc)
{
    const int n_pad = round_up(n, kTile);
    hipLaunchKernelGGL((ekf_panel_mfma_f32<true, false>), dim3(n_pad / 32, (k + 31) / 32), dim3(64), 0, stream, Wp, ldp, n,
                       kc, k, ws.dY.get(), k, nullptr, ws.dPHT.get(), ldp, nullptr);
    return true;
}

template <>
bool Ekf<double>::launch_corr_fast(int k, const double* Wp, int kc)
{
    const int n_pad = round_up(n, kTile);
    hipLaunchKernelGGL((ekf_panel_mfma_f64<true, false>), dim3(n_pad / 16, (k + 15) / 16), dim3(64), 0, stream, Wp, ldp, n, kc,
                       k, ws.dY.get(), k, nullptr, ws.dPHT.get(), ldp, nullptr);
    return true;
}

template <>
bool Ekf<double>::launch_gain_fast(int k, int n_pad, double* slot, const double* Gt, const double* U, const double* M)
{
    if (k > 64) // u (and M) come from the tuned factor kernels
    {
        return false;
    }
    hipLaunchKernelGGL((ekf_panel_mfma_f64<false, true>), dim3(n_pad / 16, (k + 15) / 16), dim3(64), 0, stream,
                       ws.dPHT.get(), ldp, n, k, k, Gt, k, U, slot, ldp, dX.get(), dPv.get(), ldp, M, ws.dWv.get(),
                       fuse_now ? (const double*)dPred.get() : (const double*)nullptr, pp.w);
    pose_fused_in_gain = (M != nullptr);
    return true;
}

template <>
int Ekf<double>::launch_downdate(const double* W, int k, hipStream_t stream)
{
    const int tiles_r = round_up(n, kTile) / kTile;
    const int kcm = opt.f64_kcm; // columns of W1 staged per pass
    // tile width: 64 columns, or 32 for small states where the launch would not fill the chip (opt.f64_cb overrides)
    const int cb = opt.f64_cb ? opt.f64_cb : ((tiles_r * (round_up(n, kTile) / 64) < 4 * num_cus) ? 2 : 4);
    const int tiles_c = round_up(n, kTile) / (16 * cb);
    const size_t lds  = (size_t)(kcm == 16 ? 2 : 1) * kcm * (128 + 16 * cb) * sizeof(double); // (16: two buffers)
    if (cb == 2)
    {
        hipLaunchKernelGGL(ekf_downdate_f64<2>, dim3(tiles_r * tiles_c), dim3(256), lds, stream, dP.get(), ldp, W, ldp,
                           k, tiles_r, opt.lower, kcm);
    }
    else
    {
        hipLaunchKernelGGL(ekf_downdate_f64<4>, dim3(tiles_r * tiles_c), dim3(256), lds, stream, dP.get(), ldp, W, ldp,
                           k, tiles_r, opt.lower, kcm);
    }
    CSLAM_HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

inline EkfBase* B(cslam_ekf_t h)
{
    return reinterpret_cast<EkfBase*>(h);
}

} // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* cslam_last_error(void)
{
    return last_error_buf();
}

int cslam_version(void)
{
    return CSLAM_VERSION;
}

int cslam_device_count(int* count)
{
    if (!count)
    {
        return fail(CSLAM_ERR_BAD_ARG, "device_count: null");
    }
    int        c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess)
    {
        *count = 0;
        return fail(CSLAM_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = c;
    return CSLAM_OK;
}

int cslam_ekf_create(int max_landmarks, int dtype, int device, int quirks, cslam_ekf_t* out)
{
    if (!out || max_landmarks < 0 || (dtype != CSLAM_F32 && dtype != CSLAM_F64) || (quirks & ~CSLAM_Q_REF_EXACT))
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_create: bad arguments");
    }
    *out  = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
    {
        return fail(CSLAM_ERR_NO_DEVICE, "ekf_create: no HIP device (this engine has no CPU fallback)");
    }
    if (device < 0)
    {
        if (hipGetDevice(&device) != hipSuccess)
        {
            device = 0;
        }
    }
    if (device >= c)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_create: device %d of %d", device, c);
    }
    const EkfOptions opt = EkfOptions::from_env(); // (the only read of the environment: ekf_options.hpp)
    EkfBase*         b   = nullptr;
    if (dtype == CSLAM_F32)
    {
        b = new (std::nothrow) Ekf<float>(opt);
    }
    else
    {
        b = new (std::nothrow) Ekf<double>(opt);
    }
    if (!b)
    {
        return fail(CSLAM_ERR_ALLOC, "ekf_create: out of host memory");
    }
    b->dtype  = dtype;
    b->device = device;
    b->quirks = quirks;
    b->nmax   = max_landmarks;
    b->ncap   = 3 + 2 * max_landmarks;
    b->ldp    = round_up(b->ncap, kTile);
    b->n      = 3;
    int rc    = b->init();
    if (rc)
    {
        delete b;
        return rc;
    }
    g_engines.fetch_add(1);
    *out = reinterpret_cast<cslam_ekf_t>(b);
    return CSLAM_OK;
}

int cslam_ekf_destroy(cslam_ekf_t h)
{
    if (!h)
    {
        return CSLAM_OK;
    }
    (void)hipSetDevice(B(h)->device);
    delete B(h);
    g_engines.fetch_sub(1);
    return CSLAM_OK;
}

#define CSLAM_NEED(h)                                                 \
    if (!(h))                                                         \
    {                                                                 \
        return fail(CSLAM_ERR_BAD_ARG, "%s: null handle", __func__);  \
    }

int cslam_ekf_set_sync_mode(cslam_ekf_t h, int sync_mode)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->la_drain()) // (queued look-ahead updates belong to the asynchronous mode they were accepted in)
    {
        return rc;
    }
    B(h)->sync_mode = sync_mode ? 1 : 0;
    return CSLAM_OK;
}

int cslam_ekf_set_state(cslam_ekf_t h, const void* X, int n, const void* P, int ldp)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->set_state(X, n, P, ldp);
}

int cslam_ekf_get_state(cslam_ekf_t h, void* X, void* P, int ldp)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->get_state(X, P, ldp);
}

int cslam_ekf_get_x(cslam_ekf_t h, void* X, int capacity)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->get_x(X, capacity);
}

int cslam_ekf_get_landmarks(cslam_ekf_t h, int first, int count, void* x, void* pll, void* pvl)
{
    CSLAM_NEED(h);
    const long long nl = (B(h)->n - 3) / 2;
    if ((!x && !pll && !pvl) || first < 1 || count < 0 || (long long)first - 1 + count > nl)
    {
        return fail(CSLAM_ERR_BAD_ARG, "get_landmarks: bad arguments (first %d, count %d, %lld landmarks)", first, count, nl);
    }
    if (count == 0)
    {
        return CSLAM_OK;
    }
    if (int rc = B(h)->resolve_predict()) // (as get_x: the held predict, the pose queue, a queued look-ahead update)
    {
        return rc;
    }
    return B(h)->get_landmarks(first, count, x, pll, pvl);
}

// The entry points of the pose read and the score answer a null handle as cslam_ekf_create answers its caller: without a
// usable GPU there is no handle to pass, and the status says so (CSLAM_ERR_NO_DEVICE); with one, a null handle is a bad
// argument.
#define CSLAM_NEED_OR_NO_DEVICE(h)                                                                              \
    if (!(h))                                                                                                   \
    {                                                                                                           \
        int c__ = 0;                                                                                            \
        if (hipGetDeviceCount(&c__) != hipSuccess || c__ == 0)                                                  \
        {                                                                                                       \
            return fail(CSLAM_ERR_NO_DEVICE, "%s: no HIP device (this engine has no CPU fallback)", __func__);  \
        }                                                                                                       \
        return fail(CSLAM_ERR_BAD_ARG, "%s: null handle", __func__);                                            \
    }

int cslam_ekf_get_pose(cslam_ekf_t h, void* x, void* pvv)
{
    CSLAM_NEED_OR_NO_DEVICE(h);
    if (!x || !pvv)
    {
        return fail(CSLAM_ERR_BAD_ARG, "get_pose: null output");
    }
    if (int rc = B(h)->resolve_predict()) // (as get_landmarks)
    {
        return rc;
    }
    return B(h)->get_pose(x, pvv);
}

int cslam_ekf_score_reset(cslam_ekf_t h, int series_capacity, double gate_pose, double gate_lm)
{
    CSLAM_NEED_OR_NO_DEVICE(h);
    return B(h)->score_reset(series_capacity, gate_pose, gate_lm);
}

int cslam_ekf_score_set_truth(cslam_ekf_t h, const double* lm_true, int count)
{
    CSLAM_NEED_OR_NO_DEVICE(h);
    return B(h)->score_set_truth(lm_true, count);
}

int cslam_ekf_score(cslam_ekf_t h, const double* xv_true, int with_map)
{
    CSLAM_NEED_OR_NO_DEVICE(h);
    if (!xv_true || !std::isfinite(xv_true[0]) || !std::isfinite(xv_true[1]) || !std::isfinite(xv_true[2]))
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_score: xv_true is null or not finite");
    }
    if (int rc = B(h)->resolve_predict()) // (as get_landmarks: the held predict, the pose queue, a queued look-ahead update)
    {
        return rc;
    }
    return B(h)->score(xv_true, with_map);
}

int cslam_ekf_get_scores(cslam_ekf_t h, double* totals, float* series, double* track, int capacity_records, int* records,
                         long long* calls)
{
    CSLAM_NEED_OR_NO_DEVICE(h);
    return B(h)->get_scores(totals, series, track, capacity_records, records, calls);
}

int cslam_ekf_get_n(cslam_ekf_t h, int* n)
{
    CSLAM_NEED(h);
    if (!n)
    {
        return fail(CSLAM_ERR_BAD_ARG, "get_n: null");
    }
    *n = B(h)->n;
    return CSLAM_OK;
}

int cslam_ekf_trace(cslam_ekf_t h, double* trace)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->trace(trace);
}

int cslam_ekf_synchronize(cslam_ekf_t h)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->sync_all();
}

int cslam_ekf_factor_status(cslam_ekf_t h, int* flags, int clear)
{
    CSLAM_NEED(h);
    return B(h)->factor_status(flags, clear);
}

int cslam_ekf_predict(cslam_ekf_t h, double v, double swa, const void* Q, double wb, double dt)
{
    CSLAM_NEED(h);
    return B(h)->predict(v, swa, Q, wb, dt);
}

int cslam_ekf_update(cslam_ekf_t h, const void* Z, int m, const void* R, const int* idf, int batch)
{
    CSLAM_NEED(h);
    return B(h)->update(Z, m, R, idf, batch, false);
}

int cslam_ekf_update_device(cslam_ekf_t h, const void* dZ, int m, const void* R, const int* d_idf, int batch)
{
    CSLAM_NEED(h);
    return B(h)->update(dZ, m, R, d_idf, batch, true);
}

int cslam_ekf_augment(cslam_ekf_t h, const void* Z, int q, const void* R)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->augment(Z, q, R);
}

int cslam_ekf_augment_device(cslam_ekf_t h, const void* dZ, int q, const void* R)
{
    CSLAM_NEED(h);
    if (q < 0 || !R || (q > 0 && !dZ)) // (before queued work is launched: on an error nothing changes)
    {
        return fail(CSLAM_ERR_BAD_ARG, "augment_device: bad arguments (q=%d)", q);
    }
    if (B(h)->n + 2 * q > B(h)->ncap)
    {
        return fail(CSLAM_ERR_CAPACITY, "augment_device: %d features would exceed max_landmarks=%d", (B(h)->n - 3) / 2 + q,
                    B(h)->nmax);
    }
    if (int rc = B(h)->resolve_predict()) // (as cslam_ekf_augment, also for q = 0, which launches no augment kernel)
    {
        return rc;
    }
    return B(h)->augment_device(dZ, q, R);
}

int cslam_ekf_augment_launches(cslam_ekf_t h, long long* launches)
{
    CSLAM_NEED(h);
    if (!launches)
    {
        return fail(CSLAM_ERR_BAD_ARG, "augment_launches: null");
    }
    *launches = B(h)->augment_launches;
    return CSLAM_OK;
}

int cslam_ekf_associate(cslam_ekf_t h, const void* Z, int m, const void* R, double gate1, double gate2, int* idf_out,
                        int* kind_out)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->associate(Z, m, R, gate1, gate2, idf_out, kind_out);
}

int cslam_ekf_associate_deferred(cslam_ekf_t h, const void* Z, int m, const void* R, double gate1, double gate2,
                                 int* idf_out, int* kind_out, int* counts_out)
{
    CSLAM_NEED(h);
    if (m < 0 || !R || (m > 0 && !Z))
    {
        return fail(CSLAM_ERR_BAD_ARG, "associate_deferred: bad arguments (m=%d)", m);
    }
    if (m == 0)
    {
        if (counts_out)
        {
            counts_out[0] = counts_out[1] = counts_out[2] = 0;
        }
        return CSLAM_OK;
    }
    if (int rc = B(h)->resolve_predict()) // (as get_landmarks: the held predict, the pose queue, a queued look-ahead update)
    {
        return rc;
    }
    return B(h)->associate_deferred(Z, m, R, gate1, gate2, idf_out, kind_out, counts_out);
}

int cslam_ekf_association_device_ptrs(cslam_ekf_t h, const void** dZF, const int** d_idf, const void** dZN,
                                      const int** d_counts)
{
    CSLAM_NEED(h);
    return B(h)->association_device_ptrs(dZF, d_idf, dZN, d_counts);
}

int cslam_ekf_associate_deferred_async(cslam_ekf_t h, const void* Z, int m, const void* R, double gate1, double gate2)
{
    CSLAM_NEED(h);
    if (m < 0 || !R || (m > 0 && !Z))
    {
        return fail(CSLAM_ERR_BAD_ARG, "associate_deferred_async: bad arguments (m=%d)", m);
    }
    if (m > 0)
    {
        if (int rc = B(h)->resolve_predict()) // (as cslam_ekf_associate_deferred)
        {
            return rc;
        }
    }
    return B(h)->associate_deferred_async(Z, m, R, gate1, gate2);
}

int cslam_ekf_association_wait(cslam_ekf_t h, int* idf_out, int* kind_out, int* counts_out)
{
    CSLAM_NEED(h);
    return B(h)->association_wait(idf_out, kind_out, counts_out);
}

int cslam_ekf_update_counted(cslam_ekf_t h, const void* dZ, int m_cap, const void* R, const int* d_idf, const int* d_count,
                             int batch)
{
    CSLAM_NEED(h);
    return B(h)->update_counted(dZ, m_cap, R, d_idf, d_count, batch);
}

int cslam_ekf_observe_heading(cslam_ekf_t h, double phi, int use_heading)
{
    CSLAM_NEED(h);
    return B(h)->observe_heading(phi, use_heading); // (a pending predict rides in the same launch)
}

int cslam_ekf_set_pgemm_workgroups(cslam_ekf_t h, int workgroups)
{
    CSLAM_NEED(h);
    if (workgroups < 0)
    {
        return fail(CSLAM_ERR_BAD_ARG, "set_pgemm_workgroups: negative");
    }
    B(h)->pgemm_wgs = workgroups;
    return CSLAM_OK;
}

int cslam_ekf_pgemm_split(cslam_ekf_t h, int* whole_tiles, int* strips)
{
    CSLAM_NEED(h);
    if (!whole_tiles || !strips)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pgemm_split: null");
    }
    *whole_tiles = B(h)->split_whole;
    *strips      = B(h)->split_strips;
    return CSLAM_OK;
}

int cslam_ekf_lookahead_windows(cslam_ekf_t h, long long* windows)
{
    CSLAM_NEED(h);
    if (!windows)
    {
        return fail(CSLAM_ERR_BAD_ARG, "lookahead_windows: null");
    }
    *windows = B(h)->la_windows;
    return CSLAM_OK;
}

int cslam_ekf_rows_launches(cslam_ekf_t h, long long* launches)
{
    CSLAM_NEED(h);
    if (!launches)
    {
        return fail(CSLAM_ERR_BAD_ARG, "rows_launches: null");
    }
    *launches = B(h)->rows_launches;
    return CSLAM_OK;
}

int cslam_ekf_stage_launches(cslam_ekf_t h, long long* launches)
{
    CSLAM_NEED(h);
    if (!launches)
    {
        return fail(CSLAM_ERR_BAD_ARG, "stage_launches: null");
    }
    *launches = B(h)->stage_launches;
    return CSLAM_OK;
}

int cslam_ekf_get_streams(cslam_ekf_t h, void** chain_stream, void** pgemm_stream)
{
    CSLAM_NEED(h);
    if (chain_stream)
    {
        *chain_stream = reinterpret_cast<void*>(B(h)->stream);
    }
    if (pgemm_stream)
    {
        *pgemm_stream = reinterpret_cast<void*>(B(h)->stream_b);
    }
    return CSLAM_OK;
}

int cslam_ekf_run_many(cslam_ekf_t* handles, int count, int steps, const double* v, const double* swa, const void* Q,
                       double wb, double dt, const void* const* dZ, const int* const* d_idf, int m, const void* R,
                       int batch)
{
    if (!handles || count < 0 || steps < 0 || m < 0 || !R || !Q || (steps > 0 && (!v || !swa)) || (m > 0 && (!dZ || !d_idf)))
    {
        return fail(CSLAM_ERR_BAD_ARG, "run_many: bad arguments");
    }
    for (int i = 0; i < count; i++)
    {
        if (!handles[i] || (m > 0 && (!dZ[i] || !d_idf[i])))
        {
            return fail(CSLAM_ERR_BAD_ARG, "run_many: null handle or input for instance %d", i);
        }
    }
    // one host thread per instance: every instance is an independent filter on its own stream pair, so the launches of
    // different instances are issued concurrently and their kernels interleave on the device (no ordering between them)
    std::vector<int>         rcs((size_t)count, CSLAM_OK);
    std::vector<std::string> msgs((size_t)count);
    auto                     body = [&](int i) {
        EkfBase*     e     = B(handles[i]);
        const size_t esz   = (e->dtype == CSLAM_F32) ? sizeof(float) : sizeof(double);
        const char*  zbase = m > 0 ? static_cast<const char*>(dZ[i]) : nullptr;
        for (int t = 0; t < steps; t++)
        {
            int rc = e->predict(v[t], swa[t], Q, wb, dt);
            if (!rc && m > 0)
            {
                rc = e->update(zbase + (size_t)t * 2 * m * esz, m, R, d_idf[i] + (size_t)t * m, batch, true);
            }
            if (rc)
            {
                rcs[(size_t)i]  = rc;
                msgs[(size_t)i] = last_error_buf(); // (thread-local: carried back to the caller's thread below)
                return;
            }
        }
    };
    if (count == 1)
    {
        body(0);
    }
    else
    {
        std::vector<std::thread> th;
        th.reserve((size_t)count);
        for (int i = 0; i < count; i++)
        {
            th.emplace_back(body, i);
        }
        for (auto& t : th)
        {
            t.join();
        }
    }
    for (int i = 0; i < count; i++)
    {
        if (rcs[(size_t)i])
        {
            return fail(rcs[(size_t)i], "run_many: instance %d: %s", i, msgs[(size_t)i].c_str());
        }
    }
    return CSLAM_OK;
}

int cslam_ekf_set_profiling(cslam_ekf_t h, int on)
{
    CSLAM_NEED(h);
    return B(h)->set_profiling(on);
}

int cslam_ekf_get_stage_times(cslam_ekf_t h, double* ms_sum, int* launches)
{
    CSLAM_NEED(h);
    return B(h)->get_stage_times(ms_sum, launches);
}

int cslam_ekf_set_deferred(cslam_ekf_t h, int max_pending_columns)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->set_deferred(max_pending_columns);
}

int cslam_ekf_flush(cslam_ekf_t h)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->do_flush();
}

int cslam_ekf_debug_last_update(cslam_ekf_t h, void* PHT, void* S, void* G, void* W1, void* V, int* k)
{
    CSLAM_NEED(h);
    if (int rc = B(h)->resolve_predict())
    {
        return rc;
    }
    return B(h)->debug_last_update(PHT, S, G, W1, V, k);
}

} // extern "C"
