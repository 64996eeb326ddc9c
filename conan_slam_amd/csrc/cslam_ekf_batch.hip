// cslam_ekf_batch.hip -- the batched Monte-Carlo engine: I independent f32 EKF-SLAM filters of the same size advance in
// lockstep on one GPU (BASELINE configs[4]; the unit that is replicated is the reference's filter loop,
// test/main.cpp:132-200: predict + batch update per control step, slam.h:235-266 via EKF.cpp:93-129, 406-455).
//
// One handle per filter (cslam_ekf_run_many) leaves the runs launch-bound: 8 co-resident instances of N = 2000 reach 2.0x
// one instance.  Here every stage of a look-ahead window (ekf_lookahead.hpp: two updates per window, their factor chain
// underneath the previous window's P-GEMM) is ONE launch for all instances:
//     stream F : ekf_la_chain_batch   I workgroups, each owning a compute unit (factor a -> carry -> factor b)
//     main     : ekf_la_rows_batch -> ekf_la_blocks_batch -> ekf_downdate_psym4_f32<BATCH> -> ekf_la_wide_batch
// The P-GEMM draws tickets over the union of the instances' lower-triangular tiles (instance-major: the workgroups of a
// launch work on one or two instances' panels at a time, which fit the L2s).  The device code of a window is the single
// filter's (the same *_body functions), so an instance's results are BITWISE those of a solo engine running look-ahead
// windows of the same pairs of updates (tests/test_batch_gpu.py).
//
// The reference's whole loop (predict + observeHeading per control step, update + augment per observation step) runs
// through cslam_ekf_batch_predict / observe_heading / update / augment: a batched pose queue (ekf_pose_step_batch_kernel),
// windows of one update, a batched augment (ekf_augment_batch_kernel) and a map that grows up to the handle's capacity
// ("The reference's loop through the batch").
//
// State lives in slabs with a fixed stride per instance: X [I][ldp], Pv [I][3 ldp], P [I][ldp ldp] (block-lower), the
// pending store W [2 regions][I][128][ldp] (P = Ps - Wp Wp^T, Wp = the previous window's panels), factor slots, the
// look-ahead scratch and the wait counters (labatch:: layout in ekf_lookahead.hpp).
#include <algorithm>
#include <cstdlib>
#include <new>
#include <utility>
#include <vector>

#include "cslam_common.hpp"
#include "device_owners.hpp"
#include "ekf_kernels.hpp"
#include "ekf_kernels_fast.hpp"
#include "ekf_landmark_kernels.hpp"
#include "ekf_lookahead.hpp"
#include "ekf_options.hpp"
#include "ekf_pgemm_tiles.hpp"
#include "ekf_pose_kernels.hpp"
#include "ekf_score_kernels.hpp"
#include "sim_scan_view.hpp"

using namespace cslam;

namespace cslam
{
// one launch per stage for all instances: blockIdx.y (the chain: blockIdx.x) is the instance
__global__ void __launch_bounds__(128) ekf_la_rows_batch(LaBatchWin w)
{
    const LaRowsArgs<float> a = la_batch_rows(w, blockIdx.y);
    ekf_la_rows_body<float>(a);
}
__global__ void __launch_bounds__(64) ekf_la_blocks_batch(LaBatchWin w)
{
    const LaPrepArgs<float> a = la_batch_prep(w, blockIdx.y);
    ekf_la_blocks_body<float>(a);
}
template <int K>
__global__ void __launch_bounds__(256) ekf_la_chain_batch(LaBatchWin w)
{
    const LaChainArgs<float> a = la_batch_chain(w, blockIdx.x); // (one workgroup per instance)
    ekf_la_chain_body<float, K>(a);
}
__global__ void __launch_bounds__(128) ekf_la_wide_batch1(LaBatchWin w) // (A/B: CSLAM_BATCH_WIDE_PAIRS=1)
{
    const LaWideArgs a = la_batch_wide(w, blockIdx.y);
    ekf_la_wide_body<1, 0>(a);
}
// (two pairs of waves per workgroup, 256 registers: 8 waves per compute unit instead of 4, see ekf_la_wide_body)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) ekf_la_wide_batch(LaBatchWin w)
{
    const LaWideArgs a = la_batch_wide(w, blockIdx.y);
    ekf_la_wide_body<2, 0>(a);
}
// ... with both updates of m = 32 observations (k = 64 known at compile time)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) ekf_la_wide_batch_k64(LaBatchWin w)
{
    const LaWideArgs a = la_batch_wide(w, blockIdx.y);
    ekf_la_wide_body<2, 64>(a);
}

// windows without a P-GEMM (nothing pending): the chains' go-ahead as a kernel of its own
__global__ void __launch_bounds__(256) ekf_la_signal_batch(unsigned* signal, unsigned add, int count, int stride)
{
    if ((int)threadIdx.x < count)
    {
        atomicAdd(signal + (size_t)threadIdx.x * stride, add);
    }
}

// batched engine (f32, block-lower): grid = (ceil(count / 256), I); instance i's slabs at the labatch strides (X ldp,
// Pv 3 ldp, P ldp^2, pending region sW) and its outputs at i * count landmarks
__global__ void __launch_bounds__(256) ekf_landmark_read_batch(const float* __restrict__ X, const float* __restrict__ Pv,
                                                               const float* __restrict__ P, int ldp,
                                                               const float* __restrict__ W, long sW, int kp, int first,
                                                               int count, float* __restrict__ x, float* __restrict__ pll,
                                                               float* __restrict__ pvl)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= count)
    {
        return;
    }
    const size_t i = blockIdx.y;
    const size_t L = (size_t)ldp;
    const size_t c = (size_t)count;
    landmark_read_body<float>(X + i * L, Pv + i * 3 * L, P + i * L * L, ldp, 1, W + i * (size_t)sW, ldp, kp, nullptr, first,
                              j, x ? x + i * 2 * c : nullptr, pll ? pll + i * 4 * c : nullptr, pvl ? pvl + i * 6 * c : nullptr);
}
} // namespace cslam

struct cslam_ekf_batch
{
    int device = 0, I = 0, n = 0, ldp = 0, quirks = 0, num_cus = 0;
    Stream      stream_own, stream_f_own; // (declared before the buffers and events: destroyed after them)
    hipStream_t stream = nullptr, stream_f = nullptr; // = stream_own.get(), stream_f_own.get()
    DevBuf<float>        dX, dPv, dP, dW, dFo, dLa, dWv;
    DevBuf<unsigned>     dDone;
    DevBuf<int>          dFlags, dIdloc;
    DevBuf<const float*> dZtab; // [2][I] (two generations: a run() may be enqueued while the previous one executes)
    DevBuf<const int*>   dIdftab;
    int                  tab_gen = 0;
    Event                ev_gen[2];                   // the last kernel that reads generation g has finished
    bool                 gen_used[2] = {false, false}; // ... and has been recorded
    // P-GEMM tile lists, one per row-tile count T (the map grows): list T is the union of the instances' lower-triangular
    // tiles (ti, tj) with ti < T, instance-major, at dTiles + tile_off[T].  All are built at create time and never
    // change, so a P-GEMM still in flight keeps reading the list it was launched with when n crosses a 128-row boundary.
    DevBuf<int2>     dTiles;
    DevBuf<int>      dTicket;
    std::vector<int> tile_off, tile_cnt;
    // the tail phase (CSLAM_PGEMM_TAIL != 0; ekf_pgemm_tiles.hpp): whole tiles + strips for every row-tile count T, every
    // number v = 1 .. 4 of strips of the last tile row that hold rows below n, and every chunk class c, at
    // dWork + work_off[(T * 4 + v - 1) * 3 + c].  Built at create like dTiles, for the same reason.
    DevBuf<int2>     dWork;
    std::vector<int> work_off, work_whole, work_strips;
    int              split_whole = 0, split_strips = 0; // the last launch (cslam_ekf_batch_pgemm_split)
    int              parity = 0;
    int              ncap   = 0; // n at max_landmarks
    // the calls of the reference's loop (cslam_ekf_batch_predict / observe_heading / update / augment): as the single
    // handle's queueing model (cslam_ekf.hip, "predict / heading"), one state for all instances
    PredictArgs<float> pp{0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0}; // the held predict
    PoseSeq<float>     pseq{};                                          // queued control steps
    DevBuf<float>      dHead;     // [I][ldp]: the column of heading steps without a map (n = 3)
    DevBuf<int>        dPoseDone; // [I]: ticket counters of ekf_pose_step_batch_kernel
    DevBuf<float>      dLm;       // landmark read outputs: 12 floats per instance and landmark of capacity
    // per-instance controls (cslam_ekf_batch_predict_each): the held predict's (v, swa) per instance, and a ring of
    // kCtlSlots slots [kPoseSeqMax][I][2] -- one per pose-queue launch -- filled in pinned host memory, copied in on the
    // main stream and read by ekf_pose_step_batch_each_kernel.  A slot is refilled only after ev_ctl says the launch that
    // read it has finished.  Allocated by the first predict_each.
    static constexpr int kCtlSlots = 4;
    bool                 pp_each  = false;
    std::vector<float>   each_v, each_swa;
    DevBuf<float>        dCtl;
    PinnedBuf<float>     hCtl;
    Event                ev_ctl[kCtlSlots];
    bool                 ctl_used[kCtlSlots] = {false, false, false, false}; // slot's event recorded, not waited for yet
    int                  ctl_slot = 0;
    unsigned             ctl_each = 0; // steps of pseq whose controls are in slot ctl_slot
    int           wcur = 0, kp = 0; // pending region and its columns
    unsigned      target = 0, seq = 0;
    long long     windows = 0;
    const EkfBatchOptions opt; // the engine switches, as the environment had them at create (ekf_options.hpp)
    DevBuf<long long> dStamps; // opt.stamps: see LaBatchWin::stamps (printed after 300 windows)
    // bench support: HIP events around one P-GEMM launch in `prof_every` (an event pair costs ~11 us of stream time)
    int                                          prof_every = 0;
    long long                                    prof_seen  = 0;
    std::vector<std::pair<Event, Event>>           prof_ev;
    size_t                                       prof_used = 0;

    // the score (cslam_ekf_batch_score_*, ekf_score_kernels.hpp): everything is allocated by the first score call or by
    // score_reset, nothing per call.  The call count lives on the host: a call's series record index is a kernel argument.
    DevBuf<double> dScore;      // totals [I][CSLAM_SCORE_FIELDS]
    DevBuf<double> dScoreParts; // [I][score_blocks()][kScoreParts]: the workgroups' partial sums of one call
    DevBuf<float>  dSeries;     // [series_cap][I][4]
    DevBuf<float>  dTruth;      // [max_landmarks][2]; NaN: no truth for this feature
    int            series_cap = 0;
    long long      score_calls = 0;
    double         gate_pose = 7.8147, gate_lm = 5.9915; // the 95 % chi-square points of 3 and 2 degrees of freedom
    int            truth_count = 0; // features scored: rows given by set_truth, or the batch's features in scan mode
    int            truth_scan  = 0; // rows the truth gather of score_scan has filled

    static constexpr int kWcols = 128; // columns per instance and region: one window's panels

    size_t sW() const { return (size_t)kWcols * ldp; }
    float* wregion(int r) const { return dW.get() + (size_t)r * I * sW(); }

    int use_device()
    {
        CSLAM_HIP_TRY(hipSetDevice(device));
        return CSLAM_OK;
    }

    explicit cslam_ekf_batch(const EkfBatchOptions& o) : opt(o) {}

    ~cslam_ekf_batch()
    {
        (void)hipSetDevice(device);
        if (stream)
        {
            (void)hipStreamSynchronize(stream);
        }
        if (stream_f)
        {
            (void)hipStreamSynchronize(stream_f);
        }
    }

    int init()
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if (opt.stamps)
        {
            // 32 phase stamps, then {start, end} of up to 128 wide-kernel workgroups per instance
            CSLAM_TRY(dStamps.alloc_zeroed_blocking(32 + (size_t)I * 256));
        }
        hipDeviceProp_t prop;
        CSLAM_HIP_TRY(hipGetDeviceProperties(&prop, device));
        num_cus = prop.multiProcessorCount;
        if (I >= num_cus / 2)
        {
            return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_create: %d instances need %d compute units for their factor chains", I, I);
        }
        int lo = 0, hi = 0;
        CSLAM_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        if ((rc = stream_own.create(hipStreamNonBlocking)) || (rc = stream_f_own.create_with_priority(hipStreamNonBlocking, hi)) ||
            (rc = ev_gen[0].create(hipEventDisableTiming)) || (rc = ev_gen[1].create(hipEventDisableTiming)))
        {
            return rc;
        }
        stream   = stream_own.get();
        stream_f = stream_f_own.get();
        const size_t L = (size_t)ldp;
        if ((rc = dX.alloc_zeroed_blocking(I * L)) || (rc = dPv.alloc_zeroed_blocking(I * 3 * L)) ||
            (rc = dP.alloc_zeroed_blocking(I * L * L)) || (rc = dW.alloc_zeroed_blocking(2 * I * sW())) ||
            (rc = dFo.alloc_zeroed_blocking((size_t)I * labatch::kFoBlock)) ||
            (rc = dLa.alloc_zeroed_blocking((size_t)I * labatch::kLaBlock)) ||
            (rc = dWv.alloc_zeroed_blocking((size_t)I * 192)) ||
            (rc = dDone.alloc_zeroed_blocking((size_t)I * labatch::kDoneBlock)) ||
            (rc = dFlags.alloc_zeroed_blocking((size_t)I * 2)) || (rc = dIdloc.alloc((size_t)I * kLaMaxObs)) ||
            (rc = dZtab.alloc((size_t)2 * I)) || (rc = dIdftab.alloc((size_t)2 * I)) ||
            (rc = dTicket.alloc_zeroed_blocking(2)) || (rc = dHead.alloc(I * L)) ||
            (rc = dPoseDone.alloc_zeroed_blocking((size_t)I)))
        {
            return rc;
        }
        // the union of the instances' lower-triangular tiles, instance-major; x = row tile | instance << 16.  Tiles of
        // pure padding rows never change: list T holds the row tiles ti < T, for every T from today's n to capacity.
        const int         tiles = ldp / kTile;
        std::vector<int2> h;
        tile_off.assign((size_t)tiles + 1, 0);
        tile_cnt.assign((size_t)tiles + 1, 0);
        for (int T = std::max(1, row_tiles()); T <= tiles; T++)
        {
            tile_off[T] = (int)h.size();
            for (int i = 0; i < I; i++)
            {
                for (int tj = 0; tj < tiles; tj++)
                {
                    for (int ti = tj; ti < T; ti++)
                    {
                        h.push_back(make_int2(ti | (i << 16), tj));
                    }
                }
            }
            tile_cnt[T] = (int)h.size() - tile_off[T];
        }
        CSLAM_TRY(dTiles.alloc(h.size()));
        CSLAM_HIP_TRY(hipMemcpy(dTiles.get(), h.data(), h.size() * sizeof(int2), hipMemcpyHostToDevice));
        if (opt.pgemm_tail != 0)
        {
            static_assert(sizeof(PgemmEntry) == sizeof(int2), "a work-list entry is an int2");
            std::vector<PgemmEntry> wl;
            work_off.assign(((size_t)tiles + 1) * 12, 0);
            work_whole.assign(((size_t)tiles + 1) * 12, 0);
            work_strips.assign(((size_t)tiles + 1) * 12, 0);
            for (int T = std::max(1, row_tiles()); T <= tiles; T++)
            {
                const int G = std::min(tile_cnt[T], 2 * (num_cus - I));
                for (int v = 1; v <= 4; v++)
                {
                    for (int c = 0; c < 3; c++)
                    {
                        // (a forced count leaves one tile of every instance whole: a workgroup enters the tail phase from
                        // the whole-tile loop)
                        const PgemmWork w = pgemm_build_work_batch(I, T, (T - 1) * kTile + v * kPgemmStrip, G, c,
                                                                   std::min(opt.pgemm_tail, T * (T + 1) / 2 - 1));
                        const size_t    at = ((size_t)T * 4 + v - 1) * 3 + c;
                        work_off[at]       = (int)wl.size();
                        work_whole[at]     = w.whole;
                        work_strips[at]    = w.strips;
                        if (w.strips > 0)
                        {
                            wl.insert(wl.end(), w.list.begin(), w.list.end());
                        }
                    }
                }
            }
            if (!wl.empty())
            {
                CSLAM_TRY(dWork.alloc(wl.size()));
                CSLAM_HIP_TRY(hipMemcpy(dWork.get(), wl.data(), wl.size() * sizeof(int2), hipMemcpyHostToDevice));
            }
        }
        CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_la_chain_batch<16>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)la_chain_lds<float>(16)));
        CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_la_chain_batch<32>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)la_chain_lds<float>(32)));
        CSLAM_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ekf_la_chain_batch<64>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)la_chain_lds<float>(64)));
        return CSLAM_OK;
    }

    int row_tiles() const { return (n + kTile - 1) / kTile; }

    int sync()
    {
        CSLAM_HIP_TRY(hipStreamSynchronize(stream_f));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // P -= Wp Wp^T of every instance: one persistent launch over the union tile list.  sig_add != 0: the launch also tells
    // the waiting factor chains that the blocks kernel in front of it has finished (see ekf_la_blocks_body).
    int flush(unsigned sig_add = 0)
    {
        if (kp == 0)
        {
            if (sig_add)
            {
                hipLaunchKernelGGL(ekf_la_signal_batch, dim3(1), dim3(256), 0, stream, dDone.get(), sig_add, I,
                                   labatch::kDoneBlock);
                CSLAM_HIP_TRY(hipGetLastError());
            }
            return CSLAM_OK;
        }
        float*    W     = wregion(wcur);
        const int k8    = round_up(kp, 8);
        const int cover = k8 <= 64 ? 64 : (k8 <= 96 ? 96 : 128);
        if (kp < cover) // (the kernel reads `cover` columns of every instance's panel)
        {
            CSLAM_HIP_TRY(hipMemset2DAsync(W + (size_t)kp * ldp, sW() * sizeof(float), 0, (size_t)(cover - kp) * ldp * sizeof(float),
                                           (size_t)I, stream));
        }
        const int      T       = std::max(1, row_tiles());
        int            G       = std::min(tile_cnt[T], 2 * (num_cus - I));
        // the tail phase: this (T, valid strips, chunk class)'s list of whole tiles and strips in place of list T
        const size_t   wat     = ((size_t)T * 4 + pgemm_valid_strips(T, n) - 1) * 3 + pgemm_chunk_class(k8);
        const bool     tail    = !work_strips.empty() && work_strips[wat] > 0;
        const int2*    tl      = tail ? dWork.get() + work_off[wat] : dTiles.get() + tile_off[T];
        const int      n_tiles = tail ? work_whole[wat] : tile_cnt[T];
        const int      n_strip = tail ? work_strips[wat] : 0;
        if (tail)
        {
            G = std::min(G, n_tiles); // (every workgroup starts with a whole tile)
        }
        split_whole            = n_tiles;
        split_strips           = n_strip;
        const unsigned sPb    = (unsigned)((size_t)ldp * ldp * 4);
        const unsigned sWb    = (unsigned)(sW() * 4);
        const unsigned p_span = (unsigned)((size_t)I * ldp * ldp * 4);
        const unsigned w_span = (unsigned)((size_t)I * sW() * 4);
        parity ^= 1;
        const bool timed = prof_every > 0 && (prof_seen++ % prof_every) == 0 && prof_used < prof_ev.size();
        if (timed)
        {
            CSLAM_HIP_TRY(hipEventRecord(prof_ev[prof_used].first.get(), stream));
        }
#define CSLAM_LAUNCH_PSYM4B(NCH, KC)                                                                                  \
    hipLaunchKernelGGL((ekf_downdate_psym4_f32<0, NCH, KC, false, true>), dim3(G), dim3(256), 0, stream, dP.get(), ldp, W, ldp, \
                       kp, tl, n_tiles, dTicket.get() + parity, dTicket.get() + (parity ^ 1),                  \
                       (unsigned long long*)nullptr, (const int*)nullptr, sPb, sWb, p_span, w_span,                   \
                       sig_add ? dDone.get() : (unsigned*)nullptr, sig_add, I, (int)labatch::kDoneBlock, n_strip)
        if (k8 <= 64)
        {
            CSLAM_LAUNCH_PSYM4B(2, 32);
        }
        else if (k8 <= 96)
        {
            CSLAM_LAUNCH_PSYM4B(4, 24);
        }
        else
        {
            CSLAM_LAUNCH_PSYM4B(4, 32);
        }
#undef CSLAM_LAUNCH_PSYM4B
        CSLAM_HIP_TRY(hipGetLastError());
        if (timed)
        {
            CSLAM_HIP_TRY(hipEventRecord(prof_ev[prof_used++].second.get(), stream));
        }
        wcur ^= 1;
        kp = 0;
        return CSLAM_OK;
    }

    // ---------------------------------------------------------------- predict / heading queue
    // A held predict followed by an update rides inside that update's window (pp_a); observe_heading joins it into ONE
    // step of the pose queue; up to kPoseSeqMax steps run as one ekf_pose_step_batch_kernel launch for all instances.
    // Every heading step appends one pending column (the rank-1 downdate -p p^T / S of the map block) to the current
    // region; rows 0..2 and [n, n_pad) of that column are written as zeros, which keeps the invariant every pending
    // column has: its rows >= n are zero (the wide kernel's panels get theirs from the zero rows of Ps), so a feature
    // appended by augment() starts with nothing pending.
    // each: the predict of this step is the held predict_each (its controls go to the control ring)
    int queue_step(const PredictArgs<float>& p, const HeadingArgs<float>& hd, bool each = false)
    {
        int rc = CSLAM_OK;
        if (pseq.count == kPoseSeqMax && (rc = launch_pose_queue()))
        {
            return rc;
        }
        int col = -1;
        if (hd.valid && n > 3)
        {
            if (kp + 1 > kWcols && ((rc = launch_pose_queue()) || (rc = flush())))
            {
                return rc;
            }
            col = kp;
            kp += 1;
        }
        const int s = pseq.count++;
        pseq.pp[s]  = p;
        pseq.hd[s]  = hd;
        pseq.col[s] = col;
        if (each && p.valid)
        {
            if (ctl_each == 0 && ctl_used[ctl_slot]) // (the first step of this launch that uses the slot)
            {
                CSLAM_HIP_TRY(hipEventSynchronize(ev_ctl[ctl_slot].get()));
                ctl_used[ctl_slot] = false;
            }
            float* hs = hCtl.get() + ctl_slot_size() * ctl_slot + (size_t)s * I * 2;
            for (int i = 0; i < I; i++)
            {
                hs[2 * i]     = each_v[i];
                hs[2 * i + 1] = each_swa[i];
            }
            ctl_each |= 1u << s;
        }
        return CSLAM_OK;
    }

    size_t ctl_slot_size() const { return (size_t)kPoseSeqMax * I * 2; }

    int ensure_ctl()
    {
        if (dCtl.get())
        {
            return CSLAM_OK;
        }
        DevBuf<float>    d;
        PinnedBuf<float> h;
        Event            ev[kCtlSlots];
        int              rc = d.alloc(kCtlSlots * ctl_slot_size());
        if (rc || (rc = h.alloc(kCtlSlots * ctl_slot_size())))
        {
            return rc;
        }
        for (Event& e : ev)
        {
            CSLAM_TRY(e.create(hipEventDisableTiming));
        }
        each_v.assign((size_t)I, 0.f);
        each_swa.assign((size_t)I, 0.f);
        dCtl = std::move(d);
        hCtl = std::move(h);
        for (int i = 0; i < kCtlSlots; i++)
        {
            ev_ctl[i] = std::move(ev[i]);
        }
        return CSLAM_OK;
    }

    int launch_pose_queue()
    {
        if (pseq.count == 0)
        {
            return CSLAM_OK;
        }
        const int n_pad = round_up(n, kTile);
        if (ctl_each == 0)
        {
            hipLaunchKernelGGL(ekf_pose_step_batch_kernel<float>, dim3((n_pad + 255) / 256, I), dim3(256), 0, stream,
                               dX.get(), dPv.get(), ldp, n, n_pad, pseq, wregion(wcur), (long)sW(), dHead.get(),
                               dPoseDone.get(), dFlags.get());
            CSLAM_HIP_TRY(hipGetLastError());
        }
        else
        {
            float* dslot = dCtl.get() + ctl_slot_size() * ctl_slot;
            CSLAM_HIP_TRY(hipMemcpyAsync(dslot, hCtl.get() + ctl_slot_size() * ctl_slot,
                                         (size_t)pseq.count * I * 2 * sizeof(float), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(ekf_pose_step_batch_each_kernel<float>, dim3((n_pad + 255) / 256, I), dim3(256), 0,
                               stream, dX.get(), dPv.get(), ldp, n, n_pad, pseq, PoseCtl<float>{dslot, ctl_each},
                               wregion(wcur), (long)sW(), dHead.get(), dPoseDone.get(), dFlags.get());
            CSLAM_HIP_TRY(hipGetLastError());
            CSLAM_HIP_TRY(hipEventRecord(ev_ctl[ctl_slot].get(), stream)); // (after the copy and its reader)
            ctl_used[ctl_slot] = true;
            ctl_slot           = (ctl_slot + 1) % kCtlSlots;
            ctl_each           = 0;
        }
        pseq.count = 0;
        return CSLAM_OK;
    }

    // everything the calls of the reference's loop left queued (a held predict becomes a predict-only step) is launched;
    // nothing to do for a handle that never used them
    int drain()
    {
        int rc = CSLAM_OK;
        if (pp.valid)
        {
            if ((rc = queue_step(pp, HeadingArgs<float>{0, 0.f, 0.f}, pp_each)))
            {
                return rc;
            }
            pp.valid = 0;
            pp_each  = false;
        }
        return launch_pose_queue();
    }

    // The per-instance input pointers of a call go into the table generation the previous call does not use, with a
    // BLOCKING copy: the chain kernels read them on stream F, which is not ordered behind copies on the main stream.  The
    // generation was last used two calls ago: wait for that call's last kernel (the call in between stays in flight).
    int stage_inputs(const float* const* dZ, const int* const* d_idf, int* gen)
    {
        tab_gen ^= 1;
        const int g = tab_gen;
        if (gen_used[g])
        {
            CSLAM_HIP_TRY(hipEventSynchronize(ev_gen[g].get()));
        }
        CSLAM_HIP_TRY(hipMemcpy(dZtab.get() + (size_t)g * I, dZ, (size_t)I * sizeof(float*), hipMemcpyHostToDevice));
        CSLAM_HIP_TRY(hipMemcpy(dIdftab.get() + (size_t)g * I, d_idf, (size_t)I * sizeof(int*), hipMemcpyHostToDevice));
        *gen = g;
        return CSLAM_OK;
    }

    int inputs_done(int g)
    {
        CSLAM_HIP_TRY(hipEventRecord(ev_gen[g].get(), stream)); // (the chains of a window finish before its wide kernel does)
        gen_used[g] = true;
        return CSLAM_OK;
    }

    // what cslam_ekf_batch_update launches ahead of its window: a held predict_each never rides inside the window (its
    // rows, chain and wide kernels take the predict by value), it is launched first as a predict-only pose step
    int launch_before_update() { return (pp.valid && pp_each) ? drain() : launch_pose_queue(); }

    // one window of ONE update at once (pairing updates across calls would hold the caller's buffers); the held predict,
    // if any, rides inside it.  Ztab / idftab: device tables of one pointer per instance.
    int update_window(const float* const* Ztab, const int* const* idftab, int m, const float* R)
    {
        LaBatchWin w;
        memset(&w, 0, sizeof(w));
        w.nu     = 1;
        w.ma     = m;
        w.mb     = m;
        w.Ztab   = Ztab;
        w.idftab = idftab;
        w.pp_a   = pp;
        w.pp_b   = pp;
        for (int e = 0; e < 4; e++)
        {
            w.R[e] = R[e];
        }
        pp.valid = 0;
        return window(w);
    }

    // q new features per instance from za.z[i] (device).  Everything is on the main stream: the P-GEMM that may sweep Ps
    // has run by the time the new rows are written, and the pending panels have zero rows for the new features (see
    // queue_step), so the kernel writes values of the true P.
    int augment_features(AugBatchArgs& za, int q, const float* R)
    {
        int rc = drain(); // (the new rows are built from the pose and the stripe: they must be current)
        if (rc)
        {
            return rc;
        }
        for (int f = 0; f < q; f++)
        {
            za.f = f;
            hipLaunchKernelGGL(ekf_augment_batch_kernel<float>, dim3((n + 255) / 256, I), dim3(256), 0, stream,
                               dX.get(), dP.get(), dPv.get(), ldp, n, za, R[0], R[1], R[2], R[3]);
            CSLAM_HIP_TRY(hipGetLastError());
            n += 2;
        }
        return CSLAM_OK;
    }

    int predict_width() const { return std::max((quirks & CSLAM_Q_PREDICT_NM4) ? (n - 4) : (n - 3), 0); }

    // ---------------------------------------------------------------- the score
    int max_landmarks() const { return (ncap - 3) / 2; }
    int score_blocks() const { return (std::max(max_landmarks(), 1) + 255) / 256; }

    // the buffers every score call needs; all-or-nothing (device_owners.hpp)
    int ensure_score()
    {
        if (dScore.get())
        {
            return CSLAM_OK;
        }
        DevBuf<double> t, p;
        DevBuf<float>  tr;
        const size_t   rows = (size_t)std::max(max_landmarks(), 1);
        int            rc   = t.alloc_zeroed((size_t)I * CSLAM_SCORE_FIELDS, stream);
        if (rc || (rc = p.alloc((size_t)I * score_blocks() * kScoreParts)) || (rc = tr.alloc(2 * rows)))
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemsetAsync(tr.get(), 0xFF, 2 * rows * sizeof(float), stream)); // (all bits set: a NaN)
        dScore      = std::move(t);
        dScoreParts = std::move(p);
        dTruth      = std::move(tr);
        return CSLAM_OK;
    }

    // one score step of what is on the main stream now; the caller has drained the queue
    int score_launch(const float* xv)
    {
        const int count  = std::min(truth_count, (n - 3) / 2);
        const int blocks = (count + 255) / 256;
        if (count > 0)
        {
            hipLaunchKernelGGL(ekf_score_landmarks_batch, dim3(blocks, I), dim3(256), 0, stream, dX.get(), dPv.get(),
                               dP.get(), ldp, wregion(wcur), (long)sW(), kp, count, dTruth.get(), gate_lm,
                               dScoreParts.get());
        }
        const int record = score_calls < (long long)series_cap ? (int)score_calls : -1;
        hipLaunchKernelGGL(ekf_score_finish_batch, dim3(I), dim3(64), 0, stream, dX.get(), dPv.get(), ldp,
                           dScoreParts.get(), blocks, xv[0], xv[1], xv[2], gate_pose, dScore.get(), dSeries.get(), record, I);
        CSLAM_HIP_TRY(hipGetLastError());
        score_calls++;
        return CSLAM_OK;
    }

    // one window: updates a (and b when nu == 2) of every instance, with their held predicts
    int window(const LaBatchWin& w0)
    {
        LaBatchWin w = w0;
        const int  ka = 2 * w.ma, kb = w.nu == 2 ? 2 * w.mb : 0;
        const unsigned n_blocks = (unsigned)(3 + ka + 2 * kb);
        w.I        = I;
        w.n        = n;
        w.ldp      = ldp;
        w.lower    = 1;
        w.textbook = (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1;
        w.X        = dX.get();
        w.Pv       = dPv.get();
        w.P        = dP.get();
        w.Wp       = wregion(wcur);
        w.sW       = (long)sW();
        w.fo       = dFo.get();
        w.la       = dLa.get();
        w.wv       = dWv.get();
        w.done     = dDone.get();
        w.flags    = dFlags.get();
        w.idloc    = dIdloc.get();
        w.kp       = kp;
        w.target   = target + n_blocks;
        w.seq      = ++seq;
        w.wg_signal = opt.wg_signal;
        w.wide_direct = 0;
        w.stamps      = dStamps.get();
        w.timeout  = 20000000ull; // 0.2 s of s_memrealtime ticks: a stuck wait raises CSLAM_FACTOR_INTERNAL instead of hanging
        // 1. the factor chains first: each takes a compute unit and waits there for its instance's blocks
        if (std::max(ka, kb) <= 16)
        {
            hipLaunchKernelGGL(ekf_la_chain_batch<16>, dim3(I), dim3(256), la_chain_lds<float>(16), stream_f, w);
        }
        else if (std::max(ka, kb) <= 32)
        {
            hipLaunchKernelGGL(ekf_la_chain_batch<32>, dim3(I), dim3(256), la_chain_lds<float>(32), stream_f, w);
        }
        else
        {
            hipLaunchKernelGGL(ekf_la_chain_batch<64>, dim3(I), dim3(256), la_chain_lds<float>(64), stream_f, w);
        }
        // 2. rows of the pending panels, then the small blocks of the current covariance (nothing may fail in between:
        //    the chains are waiting)
        hipLaunchKernelGGL(ekf_la_rows_batch, dim3(ka + kb, I), dim3(128), 0, stream, w);
        hipLaunchKernelGGL(ekf_la_blocks_batch, dim3(n_blocks, I), dim3(64), 0, stream, w);
        CSLAM_HIP_TRY(hipGetLastError());
        target += n_blocks;
        // 3. the P-GEMM of the previous window's panels: its first workgroup gives the chains their go-ahead (the blocks
        //    kernel has finished by then), and they run underneath it
        int rc = flush(opt.wg_signal ? 0u : n_blocks);
        if (rc)
        {
            return rc;
        }
        // 4. the wide half of both updates (waits in the kernel for its instance's chain); its W1 panels become the pending
        //    columns of the region the P-GEMM has just left
        w.Wn = wregion(wcur);
        if (opt.wide_pairs == 1)
        {
            hipLaunchKernelGGL(ekf_la_wide_batch1, dim3(round_up(n, kTile) / 32, I), dim3(128), 0, stream, w);
        }
        else
        {
            if (opt.la_k64 && w.ma == 32 && (w.nu == 1 || w.mb == 32))
            {
                hipLaunchKernelGGL(ekf_la_wide_batch_k64, dim3(round_up(n, kTile) / 64, I), dim3(256), 0, stream, w);
            }
            else
            {
                hipLaunchKernelGGL(ekf_la_wide_batch, dim3(round_up(n, kTile) / 64, I), dim3(256), 0, stream, w);
            }
        }
        CSLAM_HIP_TRY(hipGetLastError());
        kp = ka + kb;
        windows++;
        if (dStamps.get() && windows == 300)
        {
            long long h[32];
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            CSLAM_HIP_TRY(hipMemcpy(h, dStamps.get(), sizeof(h), hipMemcpyDeviceToHost));
            fprintf(stderr, "[cslam batch wide stamps, 10 ns ticks] ids+columns issue:%lld poll+DMA wait:%lld pht_a:%lld gain_a:%lld "
                            "store+share W1_a:%lld pht_b+corr:%lld share+G_b:%lld gain_b:%lld store_b:%lld\n",
                    h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[5] - h[4], h[6] - h[5], h[7] - h[6], h[8] - h[7], h[9] - h[8]);
            std::vector<long long> wt((size_t)I * 256);
            CSLAM_HIP_TRY(hipMemcpy(wt.data(), dStamps.get() + 32, wt.size() * sizeof(long long),
                                    hipMemcpyDeviceToHost));
            const int nwg = std::min(128, round_up(n, kTile) / (32 * opt.wide_pairs));
            long long t0  = wt[0];
            for (int i = 0; i < I; i++)
            {
                for (int b = 0; b < nwg; b++)
                {
                    t0 = std::min(t0, wt[(size_t)i * 256 + 2 * b]);
                }
            }
            fprintf(stderr, "[cslam batch wide workgroups] instance 0, duration by block of rows (10 ns ticks):");
            for (int b = 0; b < nwg; b++)
            {
                fprintf(stderr, " %lld", wt[2 * b + 1] - wt[2 * b]);
            }
            fprintf(stderr, "\n");
            for (int i = 0; i < I; i++)
            {
                long long s0 = 1ll << 62, s1 = 0, e0 = 1ll << 62, e1 = 0, dsum = 0;
                for (int b = 0; b < nwg; b++)
                {
                    const long long st = wt[(size_t)i * 256 + 2 * b] - t0, en = wt[(size_t)i * 256 + 2 * b + 1] - t0;
                    s0 = std::min(s0, st), s1 = std::max(s1, st), e0 = std::min(e0, en), e1 = std::max(e1, en);
                    dsum += en - st;
                }
                fprintf(stderr, "[cslam batch wide workgroups, 10 ns ticks] instance %d: start %lld..%lld end %lld..%lld mean duration %lld\n",
                        i, s0, s1, e0, e1, dsum / nwg);
            }
        }
        return CSLAM_OK;
    }
};

extern "C" {

int cslam_ekf_batch_create(int instances, int n_landmarks, int device, int quirks, cslam_ekf_batch_t* out)
{
    return cslam_ekf_batch_create_capacity(instances, n_landmarks, n_landmarks, device, quirks, out);
}

int cslam_ekf_batch_create_capacity(int instances, int max_landmarks, int n_landmarks, int device, int quirks,
                                    cslam_ekf_batch_t* out)
{
    if (!out || instances < 1 || instances > 255 || max_landmarks < 1 || n_landmarks < 0 || n_landmarks > max_landmarks ||
        (quirks & ~CSLAM_Q_REF_EXACT))
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_create: bad arguments");
    }
    *out  = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
    {
        return fail(CSLAM_ERR_NO_DEVICE, "ekf_batch_create: no HIP device (this engine has no CPU fallback)");
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
    {
        device = 0;
    }
    if (device >= c)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_create: device %d of %d", device, c);
    }
    const int    ncap = 3 + 2 * max_landmarks;
    const int    ldp  = round_up(ncap, kTile);
    const size_t pb   = (size_t)instances * ldp * ldp * 4;
    if (pb >= ((size_t)1 << 32))
    {
        // (the P-GEMM addresses the slab through one buffer resource with 32-bit offsets)
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_create: %d instances x %d landmarks exceed the 4 GiB covariance slab", instances,
                    max_landmarks);
    }
    cslam_ekf_batch* b = new (std::nothrow) cslam_ekf_batch(EkfBatchOptions::from_env());
    if (!b)
    {
        return fail(CSLAM_ERR_ALLOC, "ekf_batch_create: out of host memory");
    }
    b->device = device;
    b->I      = instances;
    b->n      = 3 + 2 * n_landmarks;
    b->ncap   = ncap;
    b->ldp    = ldp;
    b->quirks = quirks;
    int rc    = b->init();
    if (rc)
    {
        delete b;
        return rc;
    }
    live_engines().fetch_add(1); // (a single-filter handle created beside this one keeps its kernels free of waits)
    *out = b;
    return CSLAM_OK;
}

int cslam_ekf_batch_destroy(cslam_ekf_batch_t h)
{
    if (!h)
    {
        return CSLAM_OK;
    }
    live_engines().fetch_sub(1);
    delete h;
    return CSLAM_OK;
}

int cslam_ekf_batch_set_state(cslam_ekf_batch_t h, int instance, const float* X, int n, const float* P, int ldp)
{
    if (!h || !X || !P || instance < 0 || instance >= h->I || n != h->n || ldp < n)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_set_state: bad arguments (instance %d, n %d)", instance, n);
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()) || (rc = h->sync()))
    {
        return rc;
    }
    const size_t L  = (size_t)h->ldp;
    float*       dX = h->dX.get() + instance * L;
    float*       dP = h->dP.get() + instance * L * L;
    float*       dV = h->dPv.get() + instance * 3 * L;
    CSLAM_HIP_TRY(hipMemcpyAsync(dX, X, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CSLAM_HIP_TRY(hipMemcpy2DAsync(dP, L * sizeof(float), P, (size_t)ldp * sizeof(float), (size_t)n * sizeof(float), (size_t)n,
                                   hipMemcpyHostToDevice, h->stream));
    CSLAM_HIP_TRY(hipMemcpyAsync(dV, dP, 3 * L * sizeof(float), hipMemcpyDeviceToDevice, h->stream)); // the pose stripe
    // a new state discards this instance's pending panels (the other instances' stay)
    for (int r = 0; r < 2; r++)
    {
        CSLAM_HIP_TRY(hipMemsetAsync(h->wregion(r) + instance * h->sW(), 0, h->sW() * sizeof(float), h->stream));
    }
    CSLAM_HIP_TRY(hipMemsetAsync(h->dFlags.get() + 2 * instance, 0, 2 * sizeof(int), h->stream));
    CSLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return CSLAM_OK;
}

int cslam_ekf_batch_flush(cslam_ekf_batch_t h)
{
    if (!h)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_flush: null handle");
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()))
    {
        return rc;
    }
    return h->flush();
}

int cslam_ekf_batch_synchronize(cslam_ekf_batch_t h)
{
    if (!h)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_synchronize: null handle");
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()))
    {
        return rc;
    }
    return h->sync();
}

int cslam_ekf_batch_get_state(cslam_ekf_batch_t h, int instance, float* X, float* P, int ldp)
{
    if (!h || instance < 0 || instance >= h->I || (P && ldp < h->n))
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_get_state: bad arguments (instance %d)", instance);
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()) || (P && (rc = h->flush())))
    {
        return rc;
    }
    const size_t L = (size_t)h->ldp;
    const int    n = h->n;
    if (X)
    {
        CSLAM_HIP_TRY(hipMemcpyAsync(X, h->dX.get() + instance * L, (size_t)n * sizeof(float), hipMemcpyDeviceToHost,
                                     h->stream));
    }
    if (P)
    {
        float*    dP = h->dP.get() + instance * L * L;
        const int g  = (n + 31) / 32;
        hipLaunchKernelGGL(ekf_mirror_upper_kernel<float>, dim3(g, g), dim3(256), 0, h->stream, dP, h->ldp, n);
        hipLaunchKernelGGL(ekf_patch_pose_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, h->stream, dP,
                           h->dPv.get() + instance * 3 * L, h->ldp, n);
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipMemcpy2DAsync(P, (size_t)ldp * sizeof(float), dP, L * sizeof(float), (size_t)n * sizeof(float), (size_t)n,
                                       hipMemcpyDeviceToHost, h->stream));
    }
    CSLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return CSLAM_OK;
}

int cslam_ekf_batch_get_poses(cslam_ekf_batch_t h, float* x, float* pvv)
{
    if (!h || (!x && !pvv))
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_get_poses: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()))
    {
        return rc;
    }
    // The pose and the 3 x 3 pose block are exact once the queue has drained: pending panels hold zeros in rows 0..2, and
    // the block lives in the stripe (P[r, c] = Pv[c ldp + r]).  No P-GEMM, no mirroring: 48 bytes per instance.
    const size_t L = (size_t)h->ldp;
    if (x)
    {
        CSLAM_HIP_TRY(hipMemcpy2DAsync(x, 3 * sizeof(float), h->dX.get(), L * sizeof(float), 3 * sizeof(float),
                                       (size_t)h->I, hipMemcpyDeviceToHost, h->stream));
    }
    if (pvv) // (the stripe's columns of instance i are rows 3 i .. 3 i + 2 of the slab seen with pitch ldp)
    {
        CSLAM_HIP_TRY(hipMemcpy2DAsync(pvv, 3 * sizeof(float), h->dPv.get(), L * sizeof(float), 3 * sizeof(float),
                                       (size_t)3 * h->I, hipMemcpyDeviceToHost, h->stream));
    }
    CSLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return CSLAM_OK;
}

int cslam_ekf_batch_get_landmarks(cslam_ekf_batch_t h, int first, int count, float* x, float* pll, float* pvl)
{
    if (!h || (!x && !pll && !pvl) || first < 1 || count < 0 || (long long)first - 1 + count > (h->n - 3) / 2)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_get_landmarks: bad arguments (first %d, count %d)", first, count);
    }
    if (count == 0)
    {
        return CSLAM_OK;
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()))
    {
        return rc;
    }
    // P = Ps - Wp Wp^T over the kp columns of region wcur, read as it stands (ekf_landmark_kernels.hpp): no flush, so
    // the pending columns stay pending and every later result is the one the run would give without this read.  Every
    // writer of X, Pv, Ps and the pending store runs on the main stream (the chains on stream F hand over to the wide
    // kernel there), so the read is ordered behind them.
    if (!h->dLm.get() && (rc = h->dLm.alloc((size_t)h->I * std::max((h->ncap - 3) / 2, 1) * 12)))
    {
        return rc;
    }
    const size_t c  = (size_t)h->I * count;
    float*       ox = h->dLm.get(), *opll = h->dLm.get() + 2 * c, *opvl = h->dLm.get() + 6 * c;
    hipLaunchKernelGGL(ekf_landmark_read_batch, dim3((count + 255) / 256, h->I), dim3(256), 0, h->stream, h->dX.get(),
                       h->dPv.get(), h->dP.get(), h->ldp, h->wregion(h->wcur), (long)h->sW(), h->kp, first, count,
                       x ? ox : nullptr, pll ? opll : nullptr, pvl ? opvl : nullptr);
    CSLAM_HIP_TRY(hipGetLastError());
    if (x)
    {
        CSLAM_HIP_TRY(hipMemcpyAsync(x, ox, 2 * c * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    if (pll)
    {
        CSLAM_HIP_TRY(hipMemcpyAsync(pll, opll, 4 * c * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    if (pvl)
    {
        CSLAM_HIP_TRY(hipMemcpyAsync(pvl, opvl, 6 * c * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    CSLAM_HIP_TRY(hipStreamSynchronize(h->stream));
    return CSLAM_OK;
}

int cslam_ekf_batch_score_reset(cslam_ekf_batch_t h, int series_capacity, double gate_pose, double gate_lm)
{
    if (!h || series_capacity < 0 || gate_pose != gate_pose || gate_lm != gate_lm)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_score_reset: bad arguments (series_capacity %d)", series_capacity);
    }
    int rc = h->use_device();
    if (rc || (rc = h->ensure_score()))
    {
        return rc;
    }
    if ((size_t)series_capacity * h->I * 4 > h->dSeries.count())
    {
        DevBuf<float> sr;
        if ((rc = sr.alloc((size_t)series_capacity * h->I * 4)))
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(h->stream)); // (a score kernel in flight may still write the old series)
        h->dSeries = std::move(sr);
    }
    // behind the score kernels already on the stream
    CSLAM_HIP_TRY(hipMemsetAsync(h->dScore.get(), 0, (size_t)h->I * CSLAM_SCORE_FIELDS * sizeof(double), h->stream));
    if (series_capacity > 0)
    {
        CSLAM_HIP_TRY(hipMemsetAsync(h->dSeries.get(), 0, (size_t)series_capacity * h->I * 4 * sizeof(float), h->stream));
    }
    h->series_cap  = series_capacity;
    h->score_calls = 0;
    h->gate_pose   = gate_pose > 0.0 ? gate_pose : 7.8147;
    h->gate_lm     = gate_lm > 0.0 ? gate_lm : 5.9915;
    return CSLAM_OK;
}

int cslam_ekf_batch_score_set_truth(cslam_ekf_batch_t h, const float* lm_true, int count)
{
    if (!h || count < 0 || (count > 0 && !lm_true) || count > h->max_landmarks())
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_score_set_truth: bad arguments (count %d, max_landmarks %d)", count,
                    h ? h->max_landmarks() : 0);
    }
    int rc = h->use_device();
    if (rc || (rc = h->ensure_score()))
    {
        return rc;
    }
    const size_t rows = (size_t)std::max(h->max_landmarks(), 1);
    if (count > 0)
    {
        CSLAM_HIP_TRY(hipMemcpyAsync(h->dTruth.get(), lm_true, 2 * (size_t)count * sizeof(float), hipMemcpyHostToDevice,
                                     h->stream));
    }
    if ((size_t)count < rows)
    {
        CSLAM_HIP_TRY(hipMemsetAsync(h->dTruth.get() + 2 * (size_t)count, 0xFF, 2 * (rows - count) * sizeof(float), h->stream));
    }
    CSLAM_HIP_TRY(hipStreamSynchronize(h->stream)); // (lm_true is pageable host memory: consumed before the call returns)
    h->truth_count = count;
    h->truth_scan  = 0;
    return CSLAM_OK;
}

int cslam_ekf_batch_score(cslam_ekf_batch_t h, const float* xv_true)
{
    if (!h || !xv_true)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_score: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->ensure_score()) || (rc = h->drain()))
    {
        return rc;
    }
    return h->score_launch(xv_true);
}

int cslam_ekf_batch_get_scores(cslam_ekf_batch_t h, double* totals, float* series, int capacity_records, int* records,
                               long long* calls)
{
    if (!h || capacity_records < 0)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_get_scores: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()) || (rc = h->sync()))
    {
        return rc;
    }
    const int held = (int)std::min<long long>(h->score_calls, h->series_cap);
    if (totals)
    {
        if (h->dScore.get())
        {
            CSLAM_HIP_TRY(hipMemcpy(totals, h->dScore.get(), (size_t)h->I * CSLAM_SCORE_FIELDS * sizeof(double),
                                    hipMemcpyDeviceToHost));
        }
        else // (never scored)
        {
            std::fill(totals, totals + (size_t)h->I * CSLAM_SCORE_FIELDS, 0.0);
        }
    }
    const int take = std::min(held, capacity_records);
    if (series && take > 0)
    {
        CSLAM_HIP_TRY(hipMemcpy(series, h->dSeries.get(), (size_t)take * h->I * 4 * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (records)
    {
        *records = held;
    }
    if (calls)
    {
        *calls = h->score_calls;
    }
    return CSLAM_OK;
}

int cslam_ekf_batch_trace(cslam_ekf_batch_t h, double* traces)
{
    if (!h || !traces)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_trace: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()) || (rc = h->flush()))
    {
        return rc;
    }
    const size_t       L = (size_t)h->ldp;
    const int          n = h->n;
    std::vector<float> diag((size_t)n);
    for (int i = 0; i < h->I; i++)
    {
        CSLAM_HIP_TRY(hipMemcpy2DAsync(diag.data(), sizeof(float), h->dP.get() + i * L * L, (L + 1) * sizeof(float),
                                       sizeof(float), (size_t)n, hipMemcpyDeviceToHost, h->stream));
        CSLAM_HIP_TRY(hipMemcpy2DAsync(diag.data(), sizeof(float), h->dPv.get() + i * 3 * L, (L + 1) * sizeof(float), sizeof(float),
                                       (size_t)3, hipMemcpyDeviceToHost, h->stream)); // the pose block lives in the stripe
        CSLAM_HIP_TRY(hipStreamSynchronize(h->stream));
        double s = 0.0;
        for (float d : diag)
        {
            s += (double)d;
        }
        traces[i] = s;
    }
    return CSLAM_OK;
}

int cslam_ekf_batch_factor_status(cslam_ekf_batch_t h, int* flags)
{
    if (!h || !flags)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_factor_status: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->drain()) || (rc = h->sync()))
    {
        return rc;
    }
    std::vector<int> f((size_t)2 * h->I);
    CSLAM_HIP_TRY(hipMemcpy(f.data(), h->dFlags.get(), f.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->I; i++)
    {
        flags[i] = f[2 * i];
    }
    return CSLAM_OK;
}

int cslam_ekf_batch_run(cslam_ekf_batch_t h, int steps, const double* v, const double* swa, const float* Q, double wb, double dt,
                        const float* const* dZ, const int* const* d_idf, int m, const float* R)
{
    if (!h || steps < 0 || !v || !swa || !Q || !dZ || !d_idf || !R)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_run: bad arguments");
    }
    // run() keeps its 9..32 floor (an established part of its contract that callers and tests rely on); scans of 1..8
    // observations go through cslam_ekf_batch_update, whose windows of one update take the k <= 16 chain
    if (2 * m <= 16 || m > kLaMaxObs)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_run: m=%d outside the batched engine's 9..%d observations per update", m, kLaMaxObs);
    }
    for (int i = 0; i < h->I; i++)
    {
        if (!dZ[i] || !d_idf[i])
        {
            return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_run: instance %d has no inputs", i);
        }
    }
    if (steps == 0)
    {
        return CSLAM_OK;
    }
    int rc = h->use_device();
    if (rc)
    {
        return rc;
    }
    int g = 0;
    if ((rc = h->drain()) || (rc = h->stage_inputs(dZ, d_idf, &g)))
    {
        return rc;
    }
    const float** zt = h->dZtab.get() + (size_t)g * h->I;
    const int**   it = h->dIdftab.get() + (size_t)g * h->I;
    const int     pw = h->predict_width();
    auto          pp = [&](int t) {
        return PredictArgs<float>{1, (float)v[t], (float)swa[t], Q[0], Q[1], Q[2], Q[3], (float)wb, (float)dt, pw};
    };
    for (int t = 0; t < steps; t += 2)
    {
        LaBatchWin w;
        memset(&w, 0, sizeof(w));
        w.nu     = (t + 1 < steps) ? 2 : 1;
        w.ma     = m;
        w.mb     = m;
        w.Ztab   = zt;
        w.idftab = it;
        w.zoff_a = (long)t * 2 * m;
        w.ioff_a = (long)t * m;
        w.zoff_b = (long)(t + 1) * 2 * m;
        w.ioff_b = (long)(t + 1) * m;
        w.pp_a   = pp(t);
        w.pp_b   = w.nu == 2 ? pp(t + 1) : pp(t);
        for (int e = 0; e < 4; e++)
        {
            w.R[e] = R[e];
        }
        if ((rc = h->window(w)))
        {
            return rc;
        }
    }
    return h->inputs_done(g);
}

int cslam_ekf_batch_set_profiling(cslam_ekf_batch_t h, int every)
{
    if (!h || every < 0)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_set_profiling: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->sync()))
    {
        return rc;
    }
    h->prof_every = every;
    h->prof_seen  = 0;
    h->prof_used  = 0;
    while (every > 0 && h->prof_ev.size() < 256)
    {
        Event a, b;
        if ((rc = a.create(hipEventDefault)) || (rc = b.create(hipEventDefault)))
        {
            return rc;
        }
        h->prof_ev.emplace_back(std::move(a), std::move(b));
    }
    return CSLAM_OK;
}

int cslam_ekf_batch_get_pgemm_time(cslam_ekf_batch_t h, double* ms_sum, int* launches)
{
    if (!h || !ms_sum || !launches)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_get_pgemm_time: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->sync()))
    {
        return rc;
    }
    double s = 0.0;
    for (size_t i = 0; i < h->prof_used; i++)
    {
        float ms = 0.f;
        CSLAM_HIP_TRY(hipEventElapsedTime(&ms, h->prof_ev[i].first.get(), h->prof_ev[i].second.get()));
        s += ms;
    }
    *ms_sum   = s;
    *launches = (int)h->prof_used;
    return CSLAM_OK;
}

int cslam_ekf_batch_pgemm_split(cslam_ekf_batch_t h, int* whole_tiles, int* strips)
{
    if (!h || !whole_tiles || !strips)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_pgemm_split: bad arguments");
    }
    *whole_tiles = h->split_whole;
    *strips      = h->split_strips;
    return CSLAM_OK;
}

int cslam_ekf_batch_info(cslam_ekf_batch_t h, int* instances, int* n, long long* windows)
{
    if (!h)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_info: null handle");
    }
    if (instances)
    {
        *instances = h->I;
    }
    if (n)
    {
        *n = h->n;
    }
    if (windows)
    {
        *windows = h->windows;
    }
    return CSLAM_OK;
}

int cslam_ekf_batch_predict(cslam_ekf_batch_t h, double v, double swa, const float* Q, double wb, double dt)
{
    if (!h || !Q)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_predict: bad arguments");
    }
    int rc = h->use_device();
    if (rc)
    {
        return rc;
    }
    if (h->pp.valid && (rc = h->queue_step(h->pp, HeadingArgs<float>{0, 0.f, 0.f}, h->pp_each))) // two predicts in a row
    {
        return rc;
    }
    h->pp      = PredictArgs<float>{1, (float)v, (float)swa, Q[0], Q[1], Q[2], Q[3], (float)wb, (float)dt, h->predict_width()};
    h->pp_each = false;
    return CSLAM_OK;
}

int cslam_ekf_batch_predict_each(cslam_ekf_batch_t h, const double* v, const double* swa, const float* Q, double wb, double dt)
{
    if (!h || !v || !swa || !Q)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_predict_each: bad arguments");
    }
    int rc = h->use_device();
    if (rc || (rc = h->ensure_ctl()))
    {
        return rc;
    }
    if (h->pp.valid && (rc = h->queue_step(h->pp, HeadingArgs<float>{0, 0.f, 0.f}, h->pp_each))) // two predicts in a row
    {
        return rc;
    }
    // (v, swa) per instance; the rest of the step is common.  The held values wait in each_v / each_swa until the step is
    // queued (observe_heading joins it, anything else launches it as a predict-only step).
    h->pp      = PredictArgs<float>{1, 0.f, 0.f, Q[0], Q[1], Q[2], Q[3], (float)wb, (float)dt, h->predict_width()};
    h->pp_each = true;
    for (int i = 0; i < h->I; i++)
    {
        h->each_v[i]   = (float)v[i];
        h->each_swa[i] = (float)swa[i];
    }
    return CSLAM_OK;
}

int cslam_ekf_batch_observe_heading(cslam_ekf_batch_t h, double phi, int use_heading)
{
    if (!h)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_observe_heading: null handle");
    }
    if (!use_heading)
    {
        return CSLAM_OK; // EKF.cpp:332-335 (a held predict stays held)
    }
    int rc = h->use_device();
    if (rc)
    {
        return rc;
    }
    // float sigmaPhi = 0.01F * pi / 180.0F; R = pow(sigmaPhi, 2) -- as the single handle
    const float              sigma = (float)(((double)0.01f * kPi) / 180.0);
    const PredictArgs<float> p     = h->pp;
    if ((rc = h->queue_step(p, HeadingArgs<float>{1, (float)phi, sigma * sigma}, h->pp_each)))
    {
        return rc;
    }
    h->pp.valid = 0;
    h->pp_each  = false;
    return CSLAM_OK;
}

int cslam_ekf_batch_update(cslam_ekf_batch_t h, const float* const* dZ, const int* const* d_idf, int m, const float* R)
{
    if (!h || m < 0 || (m > 0 && (!dZ || !d_idf || !R)))
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_update: bad arguments");
    }
    if (m == 0)
    {
        return CSLAM_OK;
    }
    if (m > kLaMaxObs)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_update: m=%d outside the batched engine's 1..%d observations per update", m,
                    kLaMaxObs);
    }
    if ((h->n - 3) / 2 < 1)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_update: the map is empty");
    }
    for (int i = 0; i < h->I; i++)
    {
        if (!dZ[i] || !d_idf[i])
        {
            return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_update: instance %d has no inputs", i);
        }
    }
    int rc = h->use_device();
    int g  = 0;
    if (rc || (rc = h->launch_before_update()) || (rc = h->stage_inputs(dZ, d_idf, &g)))
    {
        return rc;
    }
    if ((rc = h->update_window(h->dZtab.get() + (size_t)g * h->I, h->dIdftab.get() + (size_t)g * h->I, m, R)))
    {
        return rc;
    }
    return h->inputs_done(g);
}

int cslam_ekf_batch_augment(cslam_ekf_batch_t h, const float* const* dZn, int q, const float* R)
{
    if (!h || q < 0 || (q > 0 && (!dZn || !R)))
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_augment: bad arguments (q=%d)", q);
    }
    if (q == 0)
    {
        return CSLAM_OK;
    }
    if (h->n + 2 * q > h->ncap)
    {
        return fail(CSLAM_ERR_CAPACITY, "ekf_batch_augment: %d features would exceed max_landmarks=%d", (h->n - 3) / 2 + q,
                    (h->ncap - 3) / 2);
    }
    AugBatchArgs za;
    for (int i = 0; i < h->I; i++)
    {
        if (!dZn[i])
        {
            return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_augment: instance %d has no inputs", i);
        }
        za.z[i] = dZn[i];
    }
    int rc = h->use_device();
    if (rc)
    {
        return rc;
    }
    return h->augment_features(za, q, R);
}

// The two calls of an observation step (test/main.cpp:188-189) fed from the batched scan generator's current scan
// (cslam_sim_batch.hip): the pointer tables are resident in the scan slot, so nothing is staged; the slot's event is
// recorded behind the last kernel that reads it (the chains of a window finish before its wide kernel does).
static int scan_view_for(const char* who, cslam_ekf_batch_t b, cslam_sim_batch_t s, SimScanView* v)
{
    if (!b || !s)
    {
        return fail(CSLAM_ERR_BAD_ARG, "%s: null handle", who);
    }
    int rc = sim_batch_current(s, v);
    if (rc)
    {
        return rc;
    }
    if (v->instances != b->I || v->device != b->device)
    {
        return fail(CSLAM_ERR_BAD_ARG, "%s: the scan is for %d instances on device %d, the batch has %d on device %d", who,
                    v->instances, v->device, b->I, b->device);
    }
    return CSLAM_OK;
}

int cslam_ekf_batch_update_scan(cslam_ekf_batch_t b, cslam_sim_batch_t s, const float* R)
{
    SimScanView v;
    int         rc = scan_view_for("ekf_batch_update_scan", b, s, &v);
    if (rc)
    {
        return rc;
    }
    if (v.updated)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_update_scan: this scan has been consumed by an update already");
    }
    if (v.mf == 0)
    {
        return sim_batch_mark(s, kScanUpdated, false);
    }
    if (v.augmented)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_update_scan: the update of a scan comes before its augment");
    }
    if (!R || (b->n - 3) / 2 != v.nf)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_update_scan: the batch holds %d features, the scan was split against %d (or R is null)",
                    (b->n - 3) / 2, v.nf);
    }
    if ((rc = b->use_device()) || (rc = b->launch_before_update()) || (rc = b->update_window(v.Ztab, v.idftab, v.mf, R)))
    {
        return rc;
    }
    CSLAM_HIP_TRY(hipEventRecord(v.consumed, b->stream));
    return sim_batch_mark(s, kScanUpdated, true);
}

int cslam_ekf_batch_augment_scan(cslam_ekf_batch_t b, cslam_sim_batch_t s, const float* R)
{
    SimScanView v;
    int         rc = scan_view_for("ekf_batch_augment_scan", b, s, &v);
    if (rc)
    {
        return rc;
    }
    if (v.augmented)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_augment_scan: this scan has been consumed by an augment already");
    }
    if (v.mf > 0 && !v.updated)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_augment_scan: the update of a scan comes before its augment");
    }
    if (v.mn == 0)
    {
        return sim_batch_mark(s, kScanAugmented, false);
    }
    if (!R || (b->n - 3) / 2 != v.nf)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_augment_scan: the batch holds %d features, the scan was split against %d (or R is null)",
                    (b->n - 3) / 2, v.nf);
    }
    if (b->n + 2 * v.mn > b->ncap)
    {
        return fail(CSLAM_ERR_CAPACITY, "ekf_batch_augment_scan: %d features would exceed max_landmarks=%d", (b->n - 3) / 2 + v.mn,
                    (b->ncap - 3) / 2);
    }
    AugBatchArgs za;
    for (int i = 0; i < b->I; i++)
    {
        za.z[i] = v.ZN + (size_t)i * kScanStride;
    }
    if ((rc = b->use_device()) || (rc = b->augment_features(za, v.mn, R)))
    {
        return rc;
    }
    CSLAM_HIP_TRY(hipEventRecord(v.consumed, b->stream));
    return sim_batch_mark(s, kScanAugmented, true);
}

// The score of an observation step with the truth from the generator: the map and the table are resident, so the rows of
// the truth buffer the batch has grown into since the last call are gathered on the main stream (the table is ordered by
// the host: cslam_sim_batch_scan has waited for its kernels), then the score kernels run as for cslam_ekf_batch_score.
int cslam_ekf_batch_score_scan(cslam_ekf_batch_t b, cslam_sim_batch_t s, const float* xv_true)
{
    SimScanView v;
    int         rc = scan_view_for("ekf_batch_score_scan", b, s, &v);
    if (rc)
    {
        return rc;
    }
    if (!xv_true)
    {
        return fail(CSLAM_ERR_BAD_ARG, "ekf_batch_score_scan: null pose");
    }
    if ((rc = b->use_device()) || (rc = b->ensure_score()) || (rc = b->drain()))
    {
        return rc;
    }
    const int nf = (b->n - 3) / 2;
    if (b->truth_scan < nf && v.nlm > 0)
    {
        hipLaunchKernelGGL(ekf_score_gather_truth, dim3((v.nlm + 255) / 256), dim3(256), 0, b->stream, v.LM, v.table, v.nlm,
                           b->truth_scan, nf, b->dTruth.get());
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipEventRecord(v.consumed, b->stream)); // (the generator's destructor waits for its readers)
        if ((rc = sim_batch_mark(s, 0, true)))
        {
            return rc;
        }
        b->truth_scan = nf;
    }
    b->truth_count = nf;
    return b->score_launch(xv_true);
}

} // extern "C"
