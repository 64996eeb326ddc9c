// cslam_pf.hip -- host side of the FastSLAM-2 particle store behind the C ABI of include/cslam.h.
//
// One handle owns np particles (one shard of the global particle set) in structure-of-arrays form in HBM
// and launches one lane per particle (or per particle x observation).  The only step of the reference that
// couples particles -- resampleParticles, PF.cpp:473-500 -- is exposed in pieces (weight sums, scaling,
// pack / unpack of particle records, local gather) so that a multi-GPU driver can put its collectives
// between them (conan_slam_amd/pf.py does that with torch.distributed over RCCL).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h> // types only: the library itself is bound with dlopen (see Rccl below)

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "cslam_common.hpp"
#include "device_owners.hpp"
#include "pf_assoc_kernels.hpp"
#include "pf_draw_kernels.hpp"
#include "pf_estimate_kernels.hpp"
#include "pf_kernels.hpp"

using namespace cslam;

namespace
{

// ------------------------------------------------------------------------------------------------
// RCCL, bound at run time.  One process must hold ONE copy of librccl (PyTorch wheels bundle their own, as they do
// libamdhip64): dlopen by SONAME returns the copy the process already has, else the system one.
// ------------------------------------------------------------------------------------------------
struct Rccl
{
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*)                                                            = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int)                                     = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t)                                                               = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)        = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)               = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)                     = nullptr;
    ncclResult_t (*GroupStart)()                                                                          = nullptr;
    ncclResult_t (*GroupEnd)()                                                                            = nullptr;
    const char* (*GetErrorString)(ncclResult_t)                                                           = nullptr;
};

inline Rccl* rccl()
{
    static Rccl r;
    static bool tried = false;
    if (!tried)
    {
        tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        {
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib)
            {
                break;
            }
        }
        if (r.lib)
        {
#define CSLAM_RCCL_SYM(field, sym) r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.lib, sym))
            CSLAM_RCCL_SYM(GetUniqueId, "ncclGetUniqueId");
            CSLAM_RCCL_SYM(CommInitRank, "ncclCommInitRank");
            CSLAM_RCCL_SYM(CommDestroy, "ncclCommDestroy");
            CSLAM_RCCL_SYM(AllReduce, "ncclAllReduce");
            CSLAM_RCCL_SYM(AllGather, "ncclAllGather");
            CSLAM_RCCL_SYM(Send, "ncclSend");
            CSLAM_RCCL_SYM(Recv, "ncclRecv");
            CSLAM_RCCL_SYM(GroupStart, "ncclGroupStart");
            CSLAM_RCCL_SYM(GroupEnd, "ncclGroupEnd");
            CSLAM_RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef CSLAM_RCCL_SYM
            if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.AllGather || !r.Send || !r.Recv ||
                !r.GroupStart || !r.GroupEnd)
            {
                r.lib = nullptr;
            }
        }
    }
    return r.lib ? &r : nullptr;
}

#define CSLAM_RCCL_TRY(expr)                                                                                         \
    do                                                                                                               \
    {                                                                                                                \
        ncclResult_t r__ = (expr);                                                                                   \
        if (r__ != ncclSuccess)                                                                                      \
        {                                                                                                            \
            return ::cslam::fail(CSLAM_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                                      \
                                 rccl()->GetErrorString ? rccl()->GetErrorString(r__) : "rccl error", __FILE__, __LINE__); \
        }                                                                                                            \
    } while (0)

// ------------------------------------------------------------------------------------------------
// The communicator of the sharded resample.  Two back-ends behind one interface:
//   RCCL      one process (rank) per GPU, collectives over xGMI -- production;
//   loopback  `world` ranks that live in ONE process on ONE device, one host thread per rank (RCCL refuses the same device
//             twice in a communicator, SURVEY 7 "hard parts"): all-reduce / all-gather / send-recv are device-to-device
//             copies ordered by a host barrier.  It exists so that the multi-rank code paths of
//             cslam_pf_resample_sharded (ranks > 0, the exchange plan, the receive ordering) can run under test on a
//             one-GPU box; it is slow on purpose (every collective synchronises the calling rank's stream twice).
// ------------------------------------------------------------------------------------------------
constexpr int kLoopMaxWorld = 16;

struct LoopPtrs
{
    const double* p[kLoopMaxWorld];
};

__global__ void comm_loop_sum_kernel(LoopPtrs ptrs, int world, double* __restrict__ out, int count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count)
    {
        double s = 0.0;
        for (int r = 0; r < world; r++) // rank order: the same sum on every rank
        {
            s += ptrs.p[r][i];
        }
        out[i] = s;
    }
}

struct LoopShared
{
    int                     world = 1;
    int                     refs  = 0;
    std::mutex              mu;
    std::condition_variable cv;
    int                     arrived = 0;
    unsigned                gen     = 0;
    bool                    broken  = false; // a rank gave up (error / timeout): every later barrier fails at once
    std::vector<const void*> src;            // [rank] buffer registered for the collective in flight
    struct P2P
    {
        const void* ptr   = nullptr;
        size_t      bytes = 0;
    };
    std::vector<P2P> sends; // [from * world + to] of the group in flight

    // all `world` ranks arrive, or false after `seconds` (a peer failed and never came)
    bool barrier(double seconds = 60.0)
    {
        std::unique_lock<std::mutex> lk(mu);
        if (broken)
        {
            return false;
        }
        const unsigned g = gen;
        if (++arrived == world)
        {
            arrived = 0;
            gen++;
            cv.notify_all();
            return true;
        }
        const bool ok = cv.wait_for(lk, std::chrono::duration<double>(seconds), [&] { return gen != g || broken; });
        if (!ok || broken)
        {
            broken = true;
            cv.notify_all();
            return false;
        }
        return true;
    }
    void poison()
    {
        std::lock_guard<std::mutex> lk(mu);
        broken = true;
        cv.notify_all();
    }
};

struct Comm
{
    ncclComm_t  comm   = nullptr; // RCCL back-end
    LoopShared* loop   = nullptr; // loopback back-end
    int         rank   = 0;
    int         world  = 1;
    int         device = 0;
    bool        in_group = false;
    struct Rv
    {
        void*  ptr;
        size_t bytes;
        int    peer;
    };
    std::vector<Rv> recvs; // loopback: receives of the open group

    int loop_fail(const char* what)
    {
        loop->poison();
        return ::cslam::fail(CSLAM_ERR_HIP, "loopback communicator: %s (rank %d of %d)", what, rank, world);
    }

    // recv[i] = sum over ranks of send[i], i < count doubles; identical on every rank
    int all_reduce_sum_f64(const double* send, double* recv, int count, hipStream_t st)
    {
        if (!loop)
        {
            CSLAM_RCCL_TRY(rccl()->AllReduce(send, recv, (size_t)count, ncclDouble, ncclSum, comm, st));
            return CSLAM_OK;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(st)); // `send` is complete
        loop->src[(size_t)rank] = send;
        if (!loop->barrier())
        {
            return loop_fail("all-reduce: a peer never arrived");
        }
        LoopPtrs ptrs{};
        for (int r = 0; r < world; r++)
        {
            ptrs.p[r] = static_cast<const double*>(loop->src[(size_t)r]);
        }
        hipLaunchKernelGGL(comm_loop_sum_kernel, dim3((count + 63) / 64), dim3(64), 0, st, ptrs, world, recv, count);
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipStreamSynchronize(st)); // every peer's `send` has been read before anybody moves on
        if (!loop->barrier())
        {
            return loop_fail("all-reduce: a peer never finished");
        }
        return CSLAM_OK;
    }

    // recv[r * bytes .. (r+1) * bytes) = rank r's send
    int all_gather(const void* send, void* recv, size_t count, ncclDataType_t dt, size_t elt, hipStream_t st)
    {
        if (!loop)
        {
            CSLAM_RCCL_TRY(rccl()->AllGather(send, recv, count, dt, comm, st));
            return CSLAM_OK;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(st));
        loop->src[(size_t)rank] = send;
        if (!loop->barrier())
        {
            return loop_fail("all-gather: a peer never arrived");
        }
        const size_t bytes = count * elt;
        for (int r = 0; r < world; r++)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(static_cast<char*>(recv) + (size_t)r * bytes, loop->src[(size_t)r], bytes,
                                         hipMemcpyDeviceToDevice, st));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(st));
        if (!loop->barrier())
        {
            return loop_fail("all-gather: a peer never finished");
        }
        return CSLAM_OK;
    }

    int group_start()
    {
        in_group = true;
        if (!loop)
        {
            CSLAM_RCCL_TRY(rccl()->GroupStart());
            return CSLAM_OK;
        }
        recvs.clear();
        for (int r = 0; r < world; r++)
        {
            loop->sends[(size_t)rank * world + r] = LoopShared::P2P{};
        }
        return CSLAM_OK;
    }
    int send(const void* buf, size_t count, ncclDataType_t dt, size_t elt, int peer, hipStream_t st)
    {
        if (!loop)
        {
            CSLAM_RCCL_TRY(rccl()->Send(buf, count, dt, peer, comm, st));
            return CSLAM_OK;
        }
        loop->sends[(size_t)rank * world + peer] = LoopShared::P2P{buf, count * elt};
        return CSLAM_OK;
    }
    int recv(void* buf, size_t count, ncclDataType_t dt, size_t elt, int peer, hipStream_t st)
    {
        if (!loop)
        {
            CSLAM_RCCL_TRY(rccl()->Recv(buf, count, dt, peer, comm, st));
            return CSLAM_OK;
        }
        recvs.push_back(Rv{buf, count * elt, peer});
        return CSLAM_OK;
    }
    // closes the group on every path (a group left open would swallow the next collective)
    int group_end(hipStream_t st)
    {
        if (!in_group)
        {
            return CSLAM_OK;
        }
        in_group = false;
        if (!loop)
        {
            CSLAM_RCCL_TRY(rccl()->GroupEnd());
            return CSLAM_OK;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(st)); // the send buffers are packed
        if (!loop->barrier())
        {
            return loop_fail("send/recv: a peer never arrived");
        }
        for (const Rv& rv : recvs)
        {
            const LoopShared::P2P& sp = loop->sends[(size_t)rv.peer * world + rank];
            if (sp.ptr == nullptr || sp.bytes != rv.bytes)
            {
                return loop_fail("send/recv: a receive has no matching send of the same size");
            }
            CSLAM_HIP_TRY(hipMemcpyAsync(rv.ptr, sp.ptr, rv.bytes, hipMemcpyDeviceToDevice, st));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(st));
        if (!loop->barrier()) // nobody reuses a send buffer before its receiver has copied it
        {
            return loop_fail("send/recv: a peer never finished");
        }
        return CSLAM_OK;
    }
};

struct PfBase
{
    virtual ~PfBase() {}
    int         dtype  = CSLAM_F32;
    int         device = 0;
    int         quirks = CSLAM_Q_REF_EXACT;
    int         np     = 0;
    int         nfcap  = 0;
    int         nf     = 0;
    Stream      stream_own;       // (in the base: destroyed after the buffers and events of Pf<T>)
    hipStream_t stream = nullptr; // = stream_own.get()

    virtual int init()                                                                       = 0;
    virtual int set_uniform_weight(double w0)                                                 = 0;
    virtual int predict(double v, double swa, const void* Q, double wb, double dt)            = 0;
    virtual int observe_heading(double phi, int use)                                          = 0;
    virtual int sample_proposal(const void* Z, int m, const int* idf, const void* R, const void* normals) = 0;
    virtual int feature_update(const void* Z, int m, const int* idf, const void* R)           = 0;
    virtual int add_features(const void* Z, int q, const void* R)                             = 0;
    virtual int weight_sums(double* sums)                                                     = 0;
    virtual int scale_weights(double scale)                                                   = 0;
    virtual int weights_ptr(void** p)                                                         = 0;
    virtual int get_weights(void* w)                                                          = 0;
    virtual int set_weights(const void* w)                                                    = 0;
    virtual int record_bytes(long long* b)                                                    = 0;
    virtual int pack(const int* idx, int count, void* drec)                                   = 0;
    virtual int unpack(const int* idx, int count, const void* drec)                           = 0;
    virtual int gather_local(const int* keep, double w_new)                                   = 0;
    virtual int resample_local(const void* select, double n_eff, int status, double* neff, int* did) = 0;
    virtual int resample_sharded(Comm* c, const void* select, double n_eff, int status, double* neff, int* did) = 0;
    virtual int debug_last_exchange(int* counts, int* send_idx, int cap, int* n_send)                = 0;
    virtual int observation_step(double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                                 const int* idf, const void* R, const void* normals, const void* select, double n_eff,
                                 int status) = 0;
    virtual int resample_stats(double* calls, double* resamples, double* last_neff) = 0;
    virtual int get_particle(int i, void* w, void* Xv, void* Pv, void* XF, void* PF)          = 0;
    virtual int set_particle(int i, const void* w, const void* Xv, const void* Pv, const void* XF, const void* PF,
                             int nf)                                                          = 0;
    // the read path (pf_estimate_kernels.hpp); c == nullptr: this handle alone
    virtual int best_particle(Comm* c, int pick, long long* index, void* w, void* Xv, void* Pv, void* XF, void* PF) = 0;
    virtual int estimate(Comm* c, double* w_sum, double* neff, void* Xv, void* Pv, void* XF, void* PF)              = 0;
    virtual int get_all_features(void* XF_all)                                                                      = 0;
    // per-particle data association (pf_assoc_kernels.hpp) and the consumers of its table
    virtual int associate(const void* Z, int m, const void* R, double gate1, double gate2)                          = 0;
    virtual int get_association(int* idf, int* kind, double* summary)                                               = 0;
    virtual int sample_proposal_assoc(const void* Z, int m, const void* R, const void* normals, const int* use,
                                      double miss_likelihood)                                                       = 0;
    virtual int feature_update_assoc(const void* Z, int m, const void* R, const int* use)                           = 0;
    // the random inputs drawn on the device (pf_draw_kernels.hpp) and the calls that consume them
    virtual int seed_draws(long long seed, long long first_global, long long n_global)                              = 0;
    virtual int get_draws(long long step, void* normals, void* select)                                              = 0;
    virtual int sample_proposal_drawn(const void* Z, int m, const int* idf, const void* R, long long step)          = 0;
    virtual int sample_proposal_assoc_drawn(const void* Z, int m, const void* R, const int* use, double miss_likelihood,
                                            long long step)                                                         = 0;
    virtual int resample_local_drawn(long long step, double n_eff, int status, double* neff, int* did)              = 0;
    virtual int resample_sharded_drawn(Comm* c, long long step, double n_eff, int status, double* neff, int* did)   = 0;
    virtual int observation_step_drawn(double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                                       const int* idf, const void* R, long long step, double n_eff, int status)     = 0;
    virtual int get_stage_copies(long long* copies)                                                                 = 0;
};

template <typename T>
struct Pf : PfBase
{
    DevBuf<T>      dW, dXv, dPv, dXF, dPF;
    // the twin set the single-pass resample gathers into; the two sets are swapped after every resample call
    DevBuf<T>      dXv2, dPv2, dXF2, dPF2;
    DevBuf<T>      dObs; // staging: Z (2*mcap T) | idf (mcap int) | normals (3*np T), filled by one copy per call
    DevBuf<int>    dIdx; // index lists of pack/unpack (max(mcap, np))
    DevBuf<double> dSums;
    DevBuf<T>      dRec; // scratch for gather_local
    int            mcap = 0;

    // Pinned staging ring.  The small host inputs of a call (Z, idf, normals, select) are copied into the next slot and
    // sent with ONE asynchronous copy, so the call returns without waiting for the stream (the caller's arrays are
    // consumed before return all the same).  The stream is drained once per lap of the ring, never per call.
    static constexpr int kStageSlots = 16;
    PinnedBuf<char>   hStage;
    size_t            stage_slot     = 0;
    int               stage_pos      = 0;
    int               stage_inflight = 0;
    Event             stage_ev[kStageSlots]; // created (and recorded) by the first copy out of the slot
    int               stage_last = 0; // slot handed out by the last stage_slot_for()
    long long         stage_copies = 0; // host-to-device copy commands enqueued for per-step inputs (stage_commit)
    std::vector<char> staged; // Z || idf bytes currently in dObs (empty = unknown)
    PinnedBuf<double> hInfo;

    ~Pf() override
    {
        (void)hipSetDevice(device);
        if (stream)
        {
            (void)hipStreamSynchronize(stream);
        }
    }

    size_t off_idf() const
    {
        return (size_t)2 * mcap * sizeof(T);
    }
    size_t off_normals() const
    {
        return off_idf() + (size_t)mcap * sizeof(int);
    }
    int* dIdf() const
    {
        return reinterpret_cast<int*>(reinterpret_cast<char*>(dObs.get()) + off_idf());
    }
    T* dNormals() const
    {
        return reinterpret_cast<T*>(reinterpret_cast<char*>(dObs.get()) + off_normals());
    }

    int stage_slot_for(size_t bytes, char** out)
    {
        if (bytes > stage_slot)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            size_t          newsz = std::max((bytes + 4095) / 4096 * 4096, 2 * stage_slot);
            PinnedBuf<char> ring;
            CSLAM_TRY(ring.alloc(newsz * kStageSlots));
            hStage         = std::move(ring);
            stage_slot     = newsz;
            stage_pos      = 0;
            stage_inflight = 0; // (the slots' events are all complete after the synchronisation above)
        }
        // a slot is reused one lap later: wait for the copy that read it last (long done in the steady state) instead of
        // draining the stream once per lap (which cost a ~60 us bubble every 16 calls)
        if (stage_ev[stage_pos])
        {
            CSLAM_HIP_TRY(hipEventSynchronize(stage_ev[stage_pos].get()));
        }
        stage_last = stage_pos;
        *out      = hStage.get() + (size_t)stage_pos * stage_slot;
        stage_pos = (stage_pos + 1) % kStageSlots;
        stage_inflight++;
        return CSLAM_OK;
    }

    // the copy out of the slot handed out last has been enqueued: mark it
    int stage_commit()
    {
        if (!stage_ev[stage_last])
        {
            CSLAM_TRY(stage_ev[stage_last].create(hipEventDisableTiming));
        }
        CSLAM_HIP_TRY(hipEventRecord(stage_ev[stage_last].get(), stream));
        stage_copies++;
        return CSLAM_OK;
    }


    int use_device()
    {
        CSLAM_HIP_TRY(hipSetDevice(device));
        return CSLAM_OK;
    }

    PfStore<T> store() const
    {
        PfStore<T> s;
        s.w  = dW.get();
        s.xv = dXv.get();
        s.pv = dPv.get();
        s.xf = dXF.get();
        s.pf = dPF.get();
        s.np = np;
        s.nf = nf;
        return s;
    }

    int ensure_m(int m)
    {
        if (m <= mcap)
        {
            return CSLAM_OK;
        }
        int newm = (std::max(m, std::max(64, 2 * mcap)) + 3) / 4 * 4; // keeps the normals 16-byte aligned
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        DevBuf<T>   obs;
        DevBuf<int> idx;
        // (newm is a multiple of 4: its ints are a whole number of T)
        int rc = obs.alloc((size_t)2 * newm + (size_t)4 * np + (size_t)newm * sizeof(int) / sizeof(T));
        if (rc || (rc = idx.alloc((size_t)std::max(newm, np))))
        {
            return rc;
        }
        staged.clear();
        dObs = std::move(obs);
        dIdx = std::move(idx);
        mcap = newm;
        return CSLAM_OK;
    }

    int init() override
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        CSLAM_TRY(stream_own.create(hipStreamNonBlocking));
        stream    = stream_own.get();
        size_t n1 = (size_t)np;
        size_t cf = (size_t)std::max(nfcap, 1);
        // PF.cpp:319-341: X = 0, P = 0, empty map; w = 1/np until the driver sets the global value
        if ((rc = dW.alloc(n1)) || (rc = dXv.alloc_zeroed(3 * n1, stream)) || (rc = dPv.alloc_zeroed(9 * n1, stream)) ||
            (rc = dXF.alloc_zeroed(2 * cf * n1, stream)) || (rc = dPF.alloc_zeroed(4 * cf * n1, stream)) ||
            (rc = dSums.alloc(2)) || (rc = dRec.alloc(n1 * (13 + 6 * cf))) || (rc = dXv2.alloc_zeroed(3 * n1,
            stream)) || (rc = dPv2.alloc_zeroed(9 * n1, stream)) || (rc = dXF2.alloc_zeroed(2 * cf * n1, stream)) ||
            (rc = dPF2.alloc_zeroed(4 * cf * n1, stream)))
        {
            return rc;
        }
        rc = ensure_m(64);
        if (rc)
        {
            return rc;
        }
        rc = set_uniform_weight(1.0 / (double)np);
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int set_uniform_weight(double w0) override
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        hipLaunchKernelGGL(pf_scale_weights_kernel<T>, dim3((np + 255) / 256), dim3(256), 0, stream, dW.get(), np,
                           (T)w0, 1);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int predict(double v, double swa, const void* Qv, double wb, double dt) override
    {
        if (!Qv)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_predict: Q is null");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        const T* Q = static_cast<const T*>(Qv);
        hipLaunchKernelGGL(pf_predict_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), (T)v, (T)swa, Q[0],
                           Q[1], Q[2], Q[3], (T)wb, (T)dt);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int observe_heading(double phi, int use) override
    {
        if (!use)
        {
            return CSLAM_OK;
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        T sigma = (T)(((double)0.01f * kPi) / 180.0); // PF.cpp:391
        hipLaunchKernelGGL(pf_heading_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), (T)phi,
                           sigma * sigma);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int check_idf(const int* idf, int m, const char* who)
    {
        for (int i = 0; i < m; i++)
        {
            if (idf[i] < 1 || idf[i] > nf)
            {
                return fail(CSLAM_ERR_BAD_ARG, "%s: idf[%d]=%d outside 1..%d", who, i, idf[i], nf);
            }
        }
        return CSLAM_OK;
    }

    // stage Z (2*m) and idf (m) of one call, plus `extra` (the normals) when given; inputs are consumed before return.
    // A call whose Z/idf are byte-identical to what dObs already holds (featureUpdate right after sampleProposal,
    // PF.cpp:150-156) sends nothing.
    int stage(const void* Z, int m, const int* idf, const void* extra = nullptr, size_t extra_bytes = 0)
    {
        int rc = ensure_m(m);
        if (rc)
        {
            return rc;
        }
        const size_t zb = (size_t)2 * m * sizeof(T), ib = idf ? (size_t)m * sizeof(int) : 0;
        const bool   same = !extra && !staged.empty() && staged.size() == zb + ib && std::memcmp(staged.data(), Z, zb) == 0 &&
                          (ib == 0 || std::memcmp(staged.data() + zb, idf, ib) == 0);
        if (same)
        {
            return CSLAM_OK;
        }
        const size_t bytes = extra ? off_normals() + extra_bytes : (idf ? off_idf() + ib : zb);
        char*        slot  = nullptr;
        if ((rc = stage_slot_for(bytes, &slot)))
        {
            return rc;
        }
        if (zb)
        {
            std::memcpy(slot, Z, zb);
        }
        if (ib)
        {
            std::memcpy(slot + off_idf(), idf, ib);
        }
        if (extra)
        {
            std::memcpy(slot + off_normals(), extra, extra_bytes);
        }
        staged.clear();
        CSLAM_HIP_TRY(hipMemcpyAsync(dObs.get(), slot, bytes, hipMemcpyHostToDevice, stream));
        if ((rc = stage_commit()))
        {
            return rc;
        }
        staged.resize(zb + ib);
        if (zb)
        {
            std::memcpy(staged.data(), Z, zb);
        }
        if (ib)
        {
            std::memcpy(staged.data() + zb, idf, ib);
        }
        return CSLAM_OK;
    }

    int sample_proposal(const void* Z, int m, const int* idf, const void* Rv, const void* normals) override
    {
        if (m < 0 || !Rv || !normals || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal: bad arguments");
        }
        int rc = use_device();
        if (rc || (rc = check_idf(idf, m, "pf_sample_proposal")) ||
            (rc = stage(Z, m, idf, normals, (size_t)3 * np * sizeof(T))))
        {
            return rc;
        }
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_sample_proposal_kernel<T>, dim3((np * kPfSubLanes + 63) / 64), dim3(64), 0, stream,
                           store(), dObs.get(), dIdf(), m, R[0], R[1], R[2], R[3], dNormals(), PfPredict<T>{0, (T)0,
                           (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0}, 0);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int feature_update(const void* Z, int m, const int* idf, const void* Rv) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_feature_update: bad arguments");
        }
        if (m == 0)
        {
            return CSLAM_OK;
        }
        int rc = use_device();
        if (rc || (rc = check_idf(idf, m, "pf_feature_update")) || (rc = stage(Z, m, idf)))
        {
            return rc;
        }
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_feature_update_kernel<T>, dim3((np + 63) / 64, m), dim3(64), 0, stream, store(),
                           dObs.get(), dIdf(), m, R[0], R[1], R[2], R[3], (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int add_features(const void* Z, int q, const void* Rv) override
    {
        if (q < 0 || !Rv || (q > 0 && !Z))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_add_features: bad arguments");
        }
        if (q == 0)
        {
            return CSLAM_OK;
        }
        if (nf + q > nfcap)
        {
            return fail(CSLAM_ERR_CAPACITY, "pf_add_features: %d features would exceed max_features=%d", nf + q, nfcap);
        }
        int rc = use_device();
        if (rc || (rc = stage(Z, q, nullptr)))
        {
            return rc;
        }
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_add_features_kernel<T>, dim3((np + 63) / 64, q), dim3(64), 0, stream, store(), dObs.get(),
                           q, R[0], R[1], R[2], R[3]);
        CSLAM_HIP_TRY(hipGetLastError());
        nf += q;
        return CSLAM_OK;
    }

    int weight_sums(double* sums) override
    {
        if (!sums)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_weight_sums: null");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        hipLaunchKernelGGL(pf_weight_sums_kernel<T>, dim3(1), dim3(256), 0, stream, dW.get(), np, dSums.get());
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipMemcpyAsync(sums, dSums.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int scale_weights(double scale) override
    {
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        hipLaunchKernelGGL(pf_scale_weights_kernel<T>, dim3((np + 255) / 256), dim3(256), 0, stream, dW.get(), np,
                           (T)scale, 0);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int weights_ptr(void** p) override
    {
        if (!p)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_weights_device_ptr: null");
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // the caller will read it from another stream
        *p = dW.get();
        return CSLAM_OK;
    }

    int get_weights(void* w) override
    {
        if (!w)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_weights: null");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(w, dW.get(), (size_t)np * sizeof(T), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int set_weights(const void* w) override
    {
        if (!w)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_set_weights: null");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(dW.get(), w, (size_t)np * sizeof(T), hipMemcpyHostToDevice, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int record_bytes(long long* b) override
    {
        if (!b)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_record_bytes: null");
        }
        *b = (long long)(13 + 6 * nf) * (long long)sizeof(T);
        return CSLAM_OK;
    }

    int stage_idx(const int* idx, int count, const char* who)
    {
        if (count < 0 || (count > 0 && !idx))
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: bad index list", who);
        }
        for (int i = 0; i < count; i++)
        {
            if (idx[i] < 0 || idx[i] >= np)
            {
                return fail(CSLAM_ERR_BAD_ARG, "%s: index %d outside 0..%d", who, idx[i], np - 1);
            }
        }
        int rc = ensure_m(count);
        if (rc)
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(dIdx.get(), idx, (size_t)count * sizeof(int), hipMemcpyHostToDevice, stream));
        return CSLAM_OK;
    }

    int pack(const int* idx, int count, void* drec) override
    {
        if (count == 0)
        {
            return CSLAM_OK;
        }
        if (!drec)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_pack: null buffer");
        }
        int rc = use_device();
        if (rc || (rc = stage_idx(idx, count, "pf_pack")))
        {
            return rc;
        }
        hipLaunchKernelGGL(pf_pack_kernel<T>, dim3(count), dim3(256), 0, stream, store(), dIdx.get(), count,
                           static_cast<T*>(drec));
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // the buffer is handed to a collective on another stream
        return CSLAM_OK;
    }

    int unpack(const int* idx, int count, const void* drec) override
    {
        if (count == 0)
        {
            return CSLAM_OK;
        }
        if (!drec)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_unpack: null buffer");
        }
        int rc = use_device();
        if (rc || (rc = stage_idx(idx, count, "pf_unpack")))
        {
            return rc;
        }
        assoc_moved = true;
        hipLaunchKernelGGL(pf_unpack_kernel<T>, dim3(count), dim3(256), 0, stream, store(), dIdx.get(), count,
                           static_cast<const T*>(drec));
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // PF.cpp:490-499 for a single shard: slot i <- particle keep[i], weights = w_new
    int gather_local(const int* keep, double w_new) override
    {
        int rc = use_device();
        if (rc || (rc = stage_idx(keep, np, "pf_gather_local")))
        {
            return rc;
        }
        assoc_moved = true;
        hipLaunchKernelGGL(pf_pack_kernel<T>, dim3(np), dim3(256), 0, stream, store(), dIdx.get(), np, dRec.get());
        CSLAM_HIP_TRY(hipGetLastError());
        std::vector<int> ident((size_t)np);
        for (int i = 0; i < np; i++)
        {
            ident[i] = i;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        CSLAM_HIP_TRY(hipMemcpyAsync(dIdx.get(), ident.data(), (size_t)np * sizeof(int), hipMemcpyHostToDevice,
                                     stream));
        hipLaunchKernelGGL(pf_unpack_kernel<T>, dim3(np), dim3(256), 0, stream, store(), dIdx.get(), np, dRec.get());
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return set_uniform_weight(w_new);
    }

    // PF.cpp:473-500 for a single shard that holds the whole particle set, without leaving the device: plan
    // (sums, normalise, Neff, decision, keep[]) -> pack(keep) -> unpack(identity) -> w = 1/N, the last three gated by a
    // device flag.  One D2H of {Neff, flag} at the end, and only if the caller asks for them.
    DevBuf<T>      dSel, dCum;
    DevBuf<int>    dKeep, dEnable;
    DevBuf<double> dInfo;
    int resample_local(const void* select, double n_eff, int status, double* neff, int* did) override
    {
        if (!select)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_resample_local: null select");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        if ((rc = ensure_resample_buffers()))
        {
            return rc;
        }
        char* slot = nullptr;
        if ((rc = stage_slot_for((size_t)np * sizeof(T), &slot)))
        {
            return rc;
        }
        std::memcpy(slot, select, (size_t)np * sizeof(T));
        CSLAM_HIP_TRY(hipMemcpyAsync(dSel.get(), slot, (size_t)np * sizeof(T), hipMemcpyHostToDevice, stream));
        if ((rc = stage_commit()))
        {
            return rc;
        }
        if ((rc = launch_resample(dSel.get(), n_eff, status)))
        {
            return rc;
        }
        return resample_result(neff, did);
    }

    // {Neff, resampled} of the resample just launched, when the caller asks for either
    int resample_result(double* neff, int* did)
    {
        if (neff || did)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(hInfo.get(), dInfo.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            stage_inflight = 0;
            if (neff)
            {
                *neff = hInfo[0];
            }
            if (did)
            {
                *did = hInfo[1] != 0.0 ? 1 : 0;
            }
        }
        return CSLAM_OK;
    }

    // PF.cpp:473-500 over a particle set sharded across ranks (one rank per GPU): see cslam_pf_resample_sharded in
    // include/cslam.h.  Everything is ordered on the handle's stream; the host reads back the two global sums (the
    // decision must be the same on every rank and drives which collectives run) and, when it resamples, the
    // 2 x world record counts of the exchange.
    DevBuf<double>    dSumsG;
    DevBuf<T>         dWall, dSelG;
    DevBuf<T>         dCumG; // running sum of the gathered weights (pf_keep_kernel)
    DevBuf<int>       dKeepG, dSendIdx, dCounts;
    PinnedBuf<double> hCounts; // the two global sums first, later the record counts (ints from double 4 on)
    DevBuf<T>         dSendBuf, dRecvBuf;
    int     sh_world = 0;
    int     sh_nf    = -1;
    std::vector<int> last_counts; // 2 * world record counts of the last exchange (send per destination, receive per source)
    int              last_n_send = 0;

    // buffers of the sharded resample: everything that can fail is allocated BEFORE the first collective, so that a rank
    // never leaves its peers waiting inside one because a local allocation failed
    int ensure_sharded_buffers(int world)
    {
        const int N = np * world;
        if (sh_world != world)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            DevBuf<double>    sums;
            DevBuf<T>         wall, sel, cum;
            DevBuf<int>       keep, send_idx, counts;
            PinnedBuf<double> hcounts;
            int               rc = sums.alloc(2);
            if (rc || (rc = wall.alloc((size_t)N)) || (rc = sel.alloc((size_t)N)) || (rc = cum.alloc((size_t)N)) ||
                (rc = keep.alloc((size_t)N)) || (rc = send_idx.alloc((size_t)N)) ||
                (rc = counts.alloc((size_t)2 * world)) || (rc = hcounts.alloc((size_t)2 * world + 4)))
            {
                return rc;
            }
            dSumsG   = std::move(sums);
            dWall    = std::move(wall);
            dSelG    = std::move(sel);
            dCumG    = std::move(cum);
            dKeepG   = std::move(keep);
            dSendIdx = std::move(send_idx);
            dCounts  = std::move(counts);
            hCounts  = std::move(hcounts);
            sh_world = world;
            sh_nf    = -1; // (the record buffers below are sized by N as well)
        }
        if (sh_nf != nf)
        {
            const size_t rec = (size_t)(13 + 6 * nf);
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            DevBuf<T> send, recv;
            int       rc = send.alloc((size_t)N * rec); // worst case: every slot keeps a particle of this rank
            if (rc || (rc = recv.alloc((size_t)np * rec)))
            {
                return rc;
            }
            dSendBuf = std::move(send);
            dRecvBuf = std::move(recv);
            sh_nf    = nf;
        }
        return CSLAM_OK;
    }

    int resample_sharded(Comm* c, const void* select, double n_eff, int status, double* neff, int* did) override
    {
        if (!c || !select)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_resample_sharded: null communicator or select");
        }
        return resample_sharded_from(c, select, 0, n_eff, status, neff, did);
    }

    int resample_sharded_drawn(Comm* c, long long step, double n_eff, int status, double* neff, int* did) override
    {
        if (!c)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_resample_sharded_drawn: null communicator");
        }
        int rc = need_draws("pf_resample_sharded_drawn");
        if (rc)
        {
            return rc;
        }
        if (draw_nglobal != (long long)c->world * np || draw_first != (long long)c->rank * np)
        {
            return fail(CSLAM_ERR_BAD_ARG,
                        "pf_resample_sharded_drawn: the draws were seeded for slots %lld.. of %lld, rank %d of %d holds %lld.. of %lld",
                        draw_first, draw_nglobal, c->rank, c->world, (long long)c->rank * np, (long long)c->world * np);
        }
        return resample_sharded_from(c, nullptr, step, n_eff, status, neff, did);
    }

    // select != nullptr: the caller's strata positions (one staged copy); nullptr: those of `step`, drawn into dSelG
    int resample_sharded_from(Comm* c, const void* select, long long step, double n_eff, int status, double* neff, int* did)
    {
        if (!c->loop && !rccl())
        {
            return fail(CSLAM_ERR_HIP, "pf_resample_sharded: librccl could not be loaded");
        }
        const int world = c->world, rank = c->rank, L = np, N = np * world;
        assoc_moved = true;
        int rc = use_device();
        if (rc || (rc = ensure_sharded_buffers(world)))
        {
            return rc;
        }
        const ncclDataType_t dt = (sizeof(T) == 4) ? ncclFloat : ncclDouble;
        // the strata positions go to the device up front as well (staging can fail; the copy is cheap when unused)
        if (select)
        {
            char* slot = nullptr;
            if ((rc = stage_slot_for((size_t)N * sizeof(T), &slot)))
            {
                return rc;
            }
            std::memcpy(slot, select, (size_t)N * sizeof(T));
            CSLAM_HIP_TRY(hipMemcpyAsync(dSelG.get(), slot, (size_t)N * sizeof(T), hipMemcpyHostToDevice, stream));
            if ((rc = stage_commit()))
            {
                return rc;
            }
        }
        else if ((rc = launch_draw(step, nullptr, dSelG.get(), N, 0, nullptr, nullptr)))
        {
            return rc;
        }
        // 1. global weight sums
        hipLaunchKernelGGL(pf_weight_sums_kernel<T>, dim3(1), dim3(256), 0, stream, dW.get(), np, dSums.get());
        CSLAM_HIP_TRY(hipGetLastError());
        if ((rc = c->all_reduce_sum_f64(dSums.get(), dSumsG.get(), 2, stream)))
        {
            return rc;
        }
        double* hs = reinterpret_cast<double*>(hCounts.get()); // (pinned; the counts use it later)
        CSLAM_HIP_TRY(hipMemcpyAsync(hs, dSumsG.get(), 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        stage_inflight = 0;
        const double ws = hs[0], ws2 = hs[1];
        // 2. w /= ws (PF.cpp:482-487), Neff = 1 / sum (w/ws)^2 (PF.cpp:549-554), the decision (PF.cpp:490)
        hipLaunchKernelGGL(pf_scale_weights_kernel<T>, dim3((np + 255) / 256), dim3(256), 0, stream, dW.get(), np,
                           (T)(1.0 / ws), 0);
        CSLAM_HIP_TRY(hipGetLastError());
        const double ne = (ws2 > 0.0) ? (ws * ws) / ws2 : 0.0;
        const bool   go = (ne < n_eff) && status;
        if (neff)
        {
            *neff = ne;
        }
        if (did)
        {
            *did = go ? 1 : 0;
        }
        last_counts.assign((size_t)2 * world, 0);
        last_n_send = 0;
        if (!go)
        {
            return CSLAM_OK;
        }
        // 3. every rank plans the same keep[] from the gathered weights and the shared strata
        if ((rc = c->all_gather(dW.get(), dWall.get(), (size_t)L, dt, sizeof(T), stream)))
        {
            return rc;
        }
        hipLaunchKernelGGL(pf_keep_kernel<T>, dim3(1), dim3(256), 0, stream, dWall.get(), N, dSelG.get(), dKeepG.get(),
                           dCumG.get());
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_exchange_plan_kernel<0>, dim3(1), dim3(256), 0, stream, dKeepG.get(), N, L, rank, world,
                           dSendIdx.get(), dCounts.get());
        CSLAM_HIP_TRY(hipGetLastError());
        int* hc = reinterpret_cast<int*>(hCounts.get()) + 8;
        CSLAM_HIP_TRY(hipMemcpyAsync(hc, dCounts.get(), (size_t)2 * world * sizeof(int), hipMemcpyDeviceToHost,
                                     stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        stage_inflight = 0;
        int n_send = 0, n_recv = 0;
        for (int r = 0; r < world; r++)
        {
            n_send += hc[r];
            n_recv += hc[world + r];
        }
        last_counts.assign(hc, hc + 2 * world);
        last_n_send = n_send;
        // (every rank derives the plan from the same gathered weights, so these checks fail on all ranks or on none)
        if (n_recv != L || hc[rank] != hc[world + rank])
        {
            return fail(CSLAM_ERR_HIP, "pf_resample_sharded: inconsistent exchange plan (%d of %d slots filled, self %d / %d)",
                        n_recv, L, hc[rank], hc[world + rank]);
        }
        const size_t rec = (size_t)(13 + 6 * nf);
        // 4. records out of the store (before any slot is overwritten), exchange, records into the slots in order
        if (n_send > 0)
        {
            hipLaunchKernelGGL(pf_pack_kernel<T>, dim3(n_send), dim3(256), 0, stream, store(), dSendIdx.get(), n_send,
                               dSendBuf.get());
            CSLAM_HIP_TRY(hipGetLastError());
        }
        // the records that stay on this rank: a device copy, outside the group
        {
            size_t soff = 0, roff = 0;
            for (int r = 0; r < rank; r++)
            {
                soff += (size_t)hc[r];
                roff += (size_t)hc[world + r];
            }
            if (hc[rank] > 0)
            {
                CSLAM_HIP_TRY(hipMemcpyAsync(dRecvBuf.get() + roff * rec, dSendBuf.get() + soff * rec,
                                             (size_t)hc[rank] * rec * sizeof(T), hipMemcpyDeviceToDevice, stream));
            }
        }
        if ((rc = c->group_start()))
        {
            return rc;
        }
        size_t soff = 0, roff = 0;
        for (int r = 0; r < world && rc == CSLAM_OK; r++)
        {
            const size_t sc = (size_t)hc[r], rcv = (size_t)hc[world + r];
            if (r != rank)
            {
                if (sc > 0)
                {
                    rc = c->send(dSendBuf.get() + soff * rec, sc * rec, dt, sizeof(T), r, stream);
                }
                if (rcv > 0 && rc == CSLAM_OK)
                {
                    rc = c->recv(dRecvBuf.get() + roff * rec, rcv * rec, dt, sizeof(T), r, stream);
                }
            }
            soff += sc;
            roff += rcv;
        }
        const int rc_end = c->group_end(stream); // (closed on the failure path too)
        if (rc || rc_end)
        {
            return rc ? rc : rc_end;
        }
        hipLaunchKernelGGL(pf_unpack_kernel<T>, dim3(L), dim3(256), 0, stream, store(), (const int*)nullptr, L,
                           dRecvBuf.get());
        CSLAM_HIP_TRY(hipGetLastError());
        return set_uniform_weight(1.0 / (double)N); // PF.cpp:495-499
    }

    // test introspection: the record counts (2 * world) and the send list of the last sharded resample
    int debug_last_exchange(int* counts, int* send_idx, int cap, int* n_send) override
    {
        if (n_send)
        {
            *n_send = last_n_send;
        }
        if (counts)
        {
            for (size_t i = 0; i < last_counts.size(); i++)
            {
                counts[i] = last_counts[i];
            }
        }
        if (send_idx && last_n_send > 0)
        {
            if (cap < last_n_send)
            {
                return fail(CSLAM_ERR_BAD_ARG, "debug_last_exchange: capacity %d < %d", cap, last_n_send);
            }
            int rc = use_device();
            if (rc)
            {
                return rc;
            }
            CSLAM_HIP_TRY(hipMemcpyAsync(send_idx, dSendIdx.get(), (size_t)last_n_send * sizeof(int),
                                         hipMemcpyDeviceToHost, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            stage_inflight = 0;
        }
        return CSLAM_OK;
    }

    // plan (sums, normalise, Neff, decision, keep[]) -> gather -> copy back + w = 1/N, the last two gated by a device flag
    int launch_resample(const T* d_select, double n_eff, int status)
    {
        assoc_moved = true; // (whether it resamples is decided on the device)
        hipLaunchKernelGGL(pf_resample_plan_kernel<T>, dim3(1), dim3(256), 0, stream, dW.get(), np, d_select, n_eff,
                           status, dCum.get(), dKeep.get(), dInfo.get(), dEnable.get());
        CSLAM_HIP_TRY(hipGetLastError());
        const dim3 ggrid(13 + 6 * store().nf, (np + 255) / 256);
        const T    w_new = (T)(1.0 / (double)np);
        PfStore<T> twin  = store();
        twin.xv          = dXv2.get();
        twin.pv          = dPv2.get();
        twin.xf          = dXF2.get();
        twin.pf          = dPF2.get();
        hipLaunchKernelGGL(pf_gather_move_kernel<T>, ggrid, dim3(256), 0, stream, store(), twin, dKeep.get(),
                           dEnable.get(), w_new);
        CSLAM_HIP_TRY(hipGetLastError());
        std::swap(dXv, dXv2); // the twin set is the store now (whether particles moved or were copied in place)
        std::swap(dPv, dPv2);
        std::swap(dXF, dXF2);
        std::swap(dPF, dPF2);
        return CSLAM_OK;
    }

    int ensure_resample_buffers()
    {
        if (dSel.get())
        {
            return CSLAM_OK;
        }
        DevBuf<T>         sel, cum;
        DevBuf<int>       keep, enable;
        DevBuf<double>    info;
        PinnedBuf<double> hinfo;
        int               rc = sel.alloc((size_t)np);
        if (rc || (rc = cum.alloc((size_t)np)) || (rc = keep.alloc((size_t)np)) || (rc = enable.alloc(1)) ||
            (rc = info.alloc_zeroed(4, stream)) || (rc = hinfo.alloc(4)))
        {
            return rc;
        }
        dSel    = std::move(sel);
        dCum    = std::move(cum);
        dKeep   = std::move(keep);
        dEnable = std::move(enable);
        dInfo   = std::move(info);
        hInfo   = std::move(hinfo);
        return CSLAM_OK;
    }

    // One whole FastSLAM-2 observation step for a shard that holds every particle -- predict, sampleProposal,
    // featureUpdate, resampleParticles (PF.cpp:419-471, 502-544, 222-277, 473-500) -- with ONE staged host-to-device
    // copy for all its small inputs (Z | idf | normals | select) and nothing returned to the host.
    int observation_step(double v, double swa, const void* Qv, double wb, double dt, const void* Z, int m, const int* idf,
                         const void* Rv, const void* normals, const void* select, double n_eff, int status) override
    {
        if (!Qv || !Rv || m < 0 || (m > 0 && (!Z || !idf || !normals)) || !select)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_observation_step: bad arguments");
        }
        int rc = use_device();
        if (rc || (rc = check_idf(idf, m, "pf_observation_step")) || (rc = ensure_m(std::max(m, 1))) ||
            (rc = ensure_resample_buffers()))
        {
            return rc;
        }
        const size_t zb = (size_t)2 * m * sizeof(T), ib = (size_t)m * sizeof(int), nb = (size_t)3 * np * sizeof(T);
        const size_t off_sel = off_normals() + nb, bytes = off_sel + (size_t)np * sizeof(T);
        char*        slot    = nullptr;
        if ((rc = stage_slot_for(bytes, &slot)))
        {
            return rc;
        }
        if (m > 0)
        {
            std::memcpy(slot, Z, zb);
            std::memcpy(slot + off_idf(), idf, ib);
            std::memcpy(slot + off_normals(), normals, nb);
        }
        std::memcpy(slot + off_sel, select, (size_t)np * sizeof(T));
        // (zero-copy -- the kernels reading the pinned slot over the host link -- was tried instead of this staged copy:
        // 13.7 k instead of 15.0 k steps/s)
        staged.clear();
        // (a small kernel reading the pinned slot in place of this copy command: 19.6 k instead of 19.9 k steps/s)
        // (a second stream for this copy, double-buffered inputs and event hand-overs so that it runs under the previous
        // step's kernels was tried: 14.8 k instead of 16.7 k steps/s -- four more runtime calls per step cost more host
        // time than the 10 us of stream time they free)
        CSLAM_HIP_TRY(hipMemcpyAsync(dObs.get(), slot, bytes, hipMemcpyHostToDevice, stream));
        if ((rc = stage_commit()))
        {
            return rc;
        }
        return launch_observation_step(v, swa, Qv, wb, dt, m, idf, Rv, n_eff, status);
    }

    // the launches of one observation step behind its inputs in dObs (Z | idf | normals | select); idf: the host copy
    int launch_observation_step(double v, double swa, const void* Qv, double wb, double dt, int m, const int* idf,
                                const void* Rv, double n_eff, int status)
    {
        const size_t off_sel = off_normals() + (size_t)3 * np * sizeof(T);
        char*      base = reinterpret_cast<char*>(dObs.get());
        const T*   sZ   = reinterpret_cast<const T*>(base);
        const int* sIdf = reinterpret_cast<const int*>(base + off_idf());
        const T*   sNrm = reinterpret_cast<const T*>(base + off_normals());
        const T* Q = static_cast<const T*>(Qv);
        const T* R = static_cast<const T*>(Rv);
        if (m > 0) // predict rides inside the proposal kernel (which overwrites xv / Pv anyway)
        {
            const PfPredict<T> pr{1, (T)v, (T)swa, Q[0], Q[1], Q[2], Q[3], (T)wb, (T)dt};
            // ... and so does the feature update, unless an observation list names a feature twice (the separate kernel
            // then updates it twice from the same old value, last writer wins: kept as it was)
            bool dup = false;
            for (int a = 0; a < m && !dup; a++)
            {
                for (int c = a + 1; c < m; c++)
                {
                    if (idf[a] == idf[c])
                    {
                        dup = true;
                        break;
                    }
                }
            }
            const int fu = dup ? 0 : ((quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 1 : 2);
            hipLaunchKernelGGL(pf_sample_proposal_kernel<T>, dim3((np * kPfSubLanes + 63) / 64), dim3(64), 0, stream, store(), sZ, sIdf,
                               m, R[0], R[1], R[2], R[3], sNrm, pr, fu);
            CSLAM_HIP_TRY(hipGetLastError());
            if (fu == 0)
            {
                hipLaunchKernelGGL(pf_feature_update_kernel<T>, dim3((np + 63) / 64, m), dim3(64), 0, stream, store(), sZ,
                                   sIdf, m, R[0], R[1], R[2], R[3], (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1);
                CSLAM_HIP_TRY(hipGetLastError());
            }
        }
        else
        {
            hipLaunchKernelGGL(pf_predict_kernel<T>, dim3((np + 63) / 64), dim3(64), 0, stream, store(), (T)v, (T)swa, Q[0],
                               Q[1], Q[2], Q[3], (T)wb, (T)dt);
            CSLAM_HIP_TRY(hipGetLastError());
        }
        return launch_resample(reinterpret_cast<const T*>(base + off_sel), n_eff, status);
    }

    int resample_stats(double* calls, double* resamples, double* last_neff) override
    {
        int rc = use_device();
        if (rc || (rc = ensure_resample_buffers()))
        {
            return rc;
        }
        CSLAM_HIP_TRY(hipMemcpyAsync(hInfo.get(), dInfo.get(), 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        stage_inflight = 0;
        if (last_neff)
        {
            *last_neff = hInfo[0];
        }
        if (calls)
        {
            *calls = hInfo[2];
        }
        if (resamples)
        {
            *resamples = hInfo[3];
        }
        return CSLAM_OK;
    }

    int get_particle(int i, void* w, void* Xv, void* Pv, void* XF, void* PF) override
    {
        if (i < 0 || i >= np)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_particle: index %d", i);
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        const size_t s = sizeof(T), pitch = (size_t)np * s;
        if (w)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(w, dW.get() + i, s, hipMemcpyDeviceToHost, stream));
        }
        if (Xv)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(Xv, s, dXv.get() + i, pitch, s, 3, hipMemcpyDeviceToHost, stream));
        }
        if (Pv)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(Pv, s, dPv.get() + i, pitch, s, 9, hipMemcpyDeviceToHost, stream));
        }
        if (XF && nf > 0)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(XF, s, dXF.get() + i, pitch, s, (size_t)2 * nf, hipMemcpyDeviceToHost,
                                           stream));
        }
        if (PF && nf > 0)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(PF, s, dPF.get() + i, pitch, s, (size_t)4 * nf, hipMemcpyDeviceToHost,
                                           stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int set_particle(int i, const void* w, const void* Xv, const void* Pv, const void* XF, const void* PF,
                     int nfeat) override
    {
        if (i < 0 || i >= np || nfeat < 0 || nfeat > nfcap)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_set_particle: index %d / nf %d", i, nfeat);
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        const size_t s = sizeof(T), pitch = (size_t)np * s;
        assoc_moved    = true;
        if (w)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(dW.get() + i, w, s, hipMemcpyHostToDevice, stream));
        }
        if (Xv)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(dXv.get() + i, pitch, Xv, s, s, 3, hipMemcpyHostToDevice, stream));
        }
        if (Pv)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(dPv.get() + i, pitch, Pv, s, s, 9, hipMemcpyHostToDevice, stream));
        }
        if (XF && nfeat > 0)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(dXF.get() + i, pitch, XF, s, s, (size_t)2 * nfeat, hipMemcpyHostToDevice,
                                           stream));
        }
        if (PF && nfeat > 0)
        {
            CSLAM_HIP_TRY(hipMemcpy2DAsync(dPF.get() + i, pitch, PF, s, s, (size_t)4 * nfeat, hipMemcpyHostToDevice,
                                           stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        nf = nfeat; // every particle of the store carries the same number of features
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // The read path: best particle, mixture moments, all features.  Every call queues its launches behind whatever is
    // on the stream, brings ONE block back through hEst (pinned) and synchronises; the store is only read.
    // ------------------------------------------------------------------------------------------------
    DevBuf<double>  dEstPart;               // per-chunk partials of passes 1 and 2
    DevBuf<double>  dEstOut, dEstLocal;     // output block: kEstOutHdr doubles, then the T record [w, Xv, Pv, XF, PF]
    DevBuf<double>  dEstSum, dEstSumAll;    // this rank's summary / every rank's (sharded estimate)
    DevBuf<double>  dBestHdrAll;            // every rank's pick (sharded best particle)
    DevBuf<T>       dBestRecAll, dEstFeat;  // every rank's picked record; the transposed features
    PinnedBuf<char> hEst;

    template <typename B>
    int est_grow(B& buf, size_t count)
    {
        if (buf.count() >= count)
        {
            return CSLAM_OK;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still uses the old buffer
        B nb;
        CSLAM_TRY(nb.alloc(count));
        buf = std::move(nb);
        return CSLAM_OK;
    }
    int est_chunks() const
    {
        return (np + kEstChunk - 1) / kEstChunk;
    }
    size_t est_out_doubles() const
    {
        return (size_t)kEstOutHdr + ((size_t)(13 + 6 * nf) * sizeof(T) + 7) / 8;
    }
    static T* est_rec(double* block)
    {
        return reinterpret_cast<T*>(block + kEstOutHdr);
    }
    // header + the first rec_len scalars of the record of `block` -> hEst, one copy, synchronised
    int est_fetch(const double* block, size_t rec_len)
    {
        const size_t bytes = (size_t)kEstOutHdr * sizeof(double) + rec_len * sizeof(T);
        CSLAM_HIP_TRY(hipMemcpyAsync(hEst.get(), block, bytes, hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }
    void est_scatter(bool map, void* w, void* Xv, void* Pv, void* XF, void* PF) const
    {
        const T* rec = reinterpret_cast<const T*>(hEst.get() + (size_t)kEstOutHdr * sizeof(double));
        if (w)
        {
            std::memcpy(w, rec, sizeof(T));
        }
        if (Xv)
        {
            std::memcpy(Xv, rec + 1, 3 * sizeof(T));
        }
        if (Pv)
        {
            std::memcpy(Pv, rec + 4, 9 * sizeof(T));
        }
        if (map && XF)
        {
            std::memcpy(XF, rec + 13, (size_t)2 * nf * sizeof(T));
        }
        if (map && PF)
        {
            std::memcpy(PF, rec + 13 + 2 * nf, (size_t)4 * nf * sizeof(T));
        }
    }
    int est_comm_ok(Comm* c, const char* who)
    {
        if (c && !c->loop && !rccl())
        {
            return fail(CSLAM_ERR_HIP, "%s: librccl could not be loaded", who);
        }
        return CSLAM_OK;
    }

    int best_particle(Comm* c, int pick, long long* index, void* w, void* Xv, void* Pv, void* XF, void* PF) override
    {
        if (pick != kEstPickMax && pick != kEstPickMin)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_best_particle: pick %d is neither CSLAM_PF_PICK_MAX nor _MIN", pick);
        }
        int rc = use_device();
        if (rc || (rc = est_comm_ok(c, "pf_best_particle_sharded")))
        {
            return rc;
        }
        const int    nch = est_chunks(), len = 13 + 6 * nf, world = c ? c->world : 1;
        const size_t od  = est_out_doubles();
        // (everything that can fail is allocated before the first collective)
        if ((rc = est_grow(dEstPart, (size_t)nch * kEstP1)) || (rc = est_grow(dEstOut, od)) ||
            (rc = est_grow(hEst, od * sizeof(double))))
        {
            return rc;
        }
        if (c && ((rc = est_grow(dEstLocal, od)) || (rc = est_grow(dBestHdrAll, (size_t)world * kEstOutHdr)) ||
                  (rc = est_grow(dBestRecAll, (size_t)world * len))))
        {
            return rc;
        }
        double* local = c ? dEstLocal.get() : dEstOut.get();
        hipLaunchKernelGGL(pf_est_pass1_kernel<T>, dim3(nch), dim3(256), 0, stream, store(), dEstPart.get());
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_best_finish_kernel<T>, dim3(1), dim3(256), 0, stream, store(), dEstPart.get(), nch, pick,
                           c ? (long long)c->rank * np : 0LL, local, est_rec(local));
        CSLAM_HIP_TRY(hipGetLastError());
        if (c)
        {
            const ncclDataType_t dt = (sizeof(T) == 4) ? ncclFloat : ncclDouble;
            if ((rc = c->all_gather(local, dBestHdrAll.get(), (size_t)kEstOutHdr, ncclDouble, sizeof(double), stream)) ||
                (rc = c->all_gather(est_rec(local), dBestRecAll.get(), (size_t)len, dt, sizeof(T), stream)))
            {
                return rc;
            }
            hipLaunchKernelGGL(pf_best_combine_kernel<T>, dim3(1), dim3(256), 0, stream, dBestHdrAll.get(),
                               dBestRecAll.get(), world, len, pick, dEstOut.get(), est_rec(dEstOut.get()));
            CSLAM_HIP_TRY(hipGetLastError());
        }
        const bool map = nf > 0 && (XF || PF);
        if ((rc = est_fetch(dEstOut.get(), map ? (size_t)len : 13)))
        {
            return rc;
        }
        if (index)
        {
            *index = (long long)reinterpret_cast<const double*>(hEst.get())[2];
        }
        est_scatter(map, w, Xv, Pv, XF, PF);
        return CSLAM_OK;
    }

    int estimate(Comm* c, double* w_sum, double* neff, void* Xv, void* Pv, void* XF, void* PF) override
    {
        int rc = use_device();
        if (rc || (rc = est_comm_ok(c, "pf_estimate_sharded")))
        {
            return rc;
        }
        const bool   map = nf > 0 && (XF || PF);
        const int    nch = est_chunks(), world = c ? c->world : 1;
        const int    stride = kEstSumHdr + (map ? kEstSumFeat * nf : 0);
        const size_t od     = est_out_doubles();
        if ((rc = est_grow(dEstPart, (size_t)nch * (kEstP1 + kEstP2Pose + (map ? (size_t)kEstP2Feat * nf : 0)))) ||
            (rc = est_grow(dEstOut, od)) || (rc = est_grow(hEst, od * sizeof(double))))
        {
            return rc;
        }
        if (c && ((rc = est_grow(dEstSum, (size_t)stride)) || (rc = est_grow(dEstSumAll, (size_t)world * stride))))
        {
            return rc;
        }
        double* p1 = dEstPart.get();
        double* p2 = p1 + (size_t)nch * kEstP1;
        double* pm = map ? p2 + (size_t)nch * kEstP2Pose : nullptr;
        const int fgroups = map ? (nf + kEstFeatPerWg - 1) / kEstFeatPerWg : 0;
        const int fblocks = map ? (nf + 255) / 256 : 0;
        hipLaunchKernelGGL(pf_est_pass1_kernel<T>, dim3(nch), dim3(256), 0, stream, store(), p1);
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_est_pass2_kernel<T>, dim3(nch, 1 + fgroups), dim3(256), 0, stream, store(), p1, nch, p2, pm);
        CSLAM_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(pf_est_finish_kernel<T>, dim3(1 + fblocks), dim3(256), 0, stream, store(), p1, p2, pm, nch,
                           c ? dEstSum.get() : nullptr, dEstOut.get(), est_rec(dEstOut.get()));
        CSLAM_HIP_TRY(hipGetLastError());
        if (c)
        {
            if ((rc = c->all_gather(dEstSum.get(), dEstSumAll.get(), (size_t)stride, ncclDouble, sizeof(double), stream)))
            {
                return rc;
            }
            hipLaunchKernelGGL(pf_est_combine_kernel<T>, dim3(1 + fblocks), dim3(256), 0, stream, dEstSumAll.get(), world,
                               stride, nf, map ? 1 : 0, dEstOut.get(), est_rec(dEstOut.get()));
            CSLAM_HIP_TRY(hipGetLastError());
        }
        if ((rc = est_fetch(dEstOut.get(), map ? (size_t)(13 + 6 * nf) : 13)))
        {
            return rc;
        }
        const double* hdr = reinterpret_cast<const double*>(hEst.get());
        if (w_sum)
        {
            *w_sum = hdr[0];
        }
        if (neff)
        {
            *neff = hdr[1];
        }
        est_scatter(map, nullptr, Xv, Pv, XF, PF);
        return CSLAM_OK;
    }

    int get_all_features(void* XF_all) override
    {
        int rc = use_device();
        if (rc || nf == 0 || !XF_all)
        {
            return rc;
        }
        const size_t count = (size_t)2 * nf * np;
        if ((rc = est_grow(dEstFeat, count)) || (rc = est_grow(hEst, count * sizeof(T))))
        {
            return rc;
        }
        hipLaunchKernelGGL(pf_all_features_kernel<T>, dim3((np + 63) / 64, (2 * nf + 63) / 64), dim3(256), 0, stream,
                           store(), dEstFeat.get());
        CSLAM_HIP_TRY(hipGetLastError());
        CSLAM_HIP_TRY(hipMemcpyAsync(hEst.get(), dEstFeat.get(), count * sizeof(T), hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        std::memcpy(XF_all, hEst.get(), count * sizeof(T));
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // Per-particle gated nearest-neighbour association (EKF.cpp:131-144, 235-326 on each particle's own state) and the
    // consumers that read its table.  The tables belong to the handle and describe the LAST associate call: its
    // observations (kept on the host to recognise them again), the particle order and the map size of that moment.
    // ------------------------------------------------------------------------------------------------
    DevBuf<T>         dAPartNd, dAPartNis, dARawNd;
    DevBuf<int>       dAPartJ, dARawIdf, dARawKind, dAIdf, dAKind;
    DevBuf<double>    dASummary;
    size_t            assoc_part_cap = 0; // entries of the three partial tables
    int               assoc_mcap     = 0; // observations the (m x np) tables and the summary hold
    int               assoc_m        = -1; // -1: associate has not been called
    int               assoc_nf       = 0;
    bool              assoc_moved    = false; // particles changed slots (resample, unpack, set_particle) since associate
    std::vector<char> assoc_Z;            // the 2 * assoc_m observation scalars of the last associate

    // all-or-nothing growth (device_owners.hpp): new buffers into locals first, members replaced only when all exist
    int ensure_assoc(int m, int nchunks)
    {
        const size_t need_part = (size_t)std::max(nchunks, 1) * m * np;
        if (need_part > assoc_part_cap)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still reads the old partials
            DevBuf<T>   nd, nis;
            DevBuf<int> pj;
            int         rc = nd.alloc(need_part);
            if (rc || (rc = nis.alloc(need_part)) || (rc = pj.alloc(need_part)))
            {
                return rc;
            }
            dAPartNd       = std::move(nd);
            dAPartNis      = std::move(nis);
            dAPartJ        = std::move(pj);
            assoc_part_cap = need_part;
        }
        if (m > assoc_mcap)
        {
            const int    newm = std::max(m, std::max(64, 2 * assoc_mcap));
            const size_t cnt  = (size_t)newm * np;
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            DevBuf<T>      rnd;
            DevBuf<int>    ridf, rkind, idf, kind;
            DevBuf<double> sum;
            int            rc = rnd.alloc(cnt);
            if (rc || (rc = ridf.alloc(cnt)) || (rc = rkind.alloc(cnt)) || (rc = idf.alloc(cnt)) ||
                (rc = kind.alloc(cnt)) || (rc = sum.alloc((size_t)newm * 4)))
            {
                return rc;
            }
            dARawNd    = std::move(rnd);
            dARawIdf   = std::move(ridf);
            dARawKind  = std::move(rkind);
            dAIdf      = std::move(idf);
            dAKind     = std::move(kind);
            dASummary  = std::move(sum);
            assoc_mcap = newm;
            assoc_m    = -1; // the old tables are gone
        }
        return CSLAM_OK;
    }

    int associate(const void* Z, int m, const void* Rv, double gate1, double gate2) override
    {
        if (m < 0 || m > 65535 || !Rv || (m > 0 && !Z)) // (one grid row per observation)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_associate: bad arguments (m=%d)", m);
        }
        if (!std::isfinite(gate1) || !std::isfinite(gate2))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_associate: gates must be finite (gate1=%g, gate2=%g)", gate1, gate2);
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        const int nchunks = (nf + kPfAssocFeatChunk - 1) / kPfAssocFeatChunk;
        if (m > 0)
        {
            if ((rc = ensure_assoc(m, nchunks)) || (rc = stage(Z, m, nullptr)))
            {
                return rc;
            }
            const T*   R = static_cast<const T*>(Rv);
            const int  pb = (np + 63) / 64;
            if (nchunks > 0)
            {
                hipLaunchKernelGGL(pf_assoc_scan_kernel<T>, dim3(pb, nchunks, (m + kPfAssocObsChunk - 1) / kPfAssocObsChunk),
                                   dim3(64), 0, stream, store(), dObs.get(), m, R[0], R[1], R[2], R[3], (T)gate1,
                                   dAPartNd.get(), dAPartJ.get(), dAPartNis.get());
                CSLAM_HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(pf_assoc_merge_kernel<T>, dim3(pb, m), dim3(64), 0, stream, np, m, nchunks, dAPartNd.get(),
                               dAPartJ.get(), dAPartNis.get(), (T)gate2, dARawIdf.get(), dARawKind.get(), dARawNd.get());
            CSLAM_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(pf_assoc_resolve_kernel<T>, dim3(pb, m), dim3(64), 0, stream, np, m, dARawIdf.get(),
                               dARawKind.get(), dARawNd.get(), dAIdf.get(), dAKind.get());
            CSLAM_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(pf_assoc_summary_kernel<T>, dim3(m), dim3(256), 0, stream, dW.get(), np, dAKind.get(),
                               dASummary.get());
            CSLAM_HIP_TRY(hipGetLastError());
        }
        assoc_m     = m;
        assoc_nf    = nf;
        assoc_moved = false;
        assoc_Z.clear();
        if (m > 0)
        {
            assoc_Z.assign(static_cast<const char*>(Z), static_cast<const char*>(Z) + (size_t)2 * m * sizeof(T));
        }
        return CSLAM_OK;
    }

    int get_association(int* idf, int* kind, double* summary) override
    {
        if (assoc_m < 0)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_association: cslam_pf_associate has not been called");
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        const size_t cnt = (size_t)assoc_m * np;
        if (idf && cnt)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(idf, dAIdf.get(), cnt * sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        if (kind && cnt)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(kind, dAKind.get(), cnt * sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        if (summary && assoc_m)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(summary, dASummary.get(), (size_t)assoc_m * 4 * sizeof(double),
                                         hipMemcpyDeviceToHost, stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    // the consumers take the observations of the last associate: anything else would pair a table with the wrong scan
    int check_assoc_inputs(const void* Z, int m, const int* use, const char* who)
    {
        if (assoc_m < 0)
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: cslam_pf_associate has not been called", who);
        }
        if (assoc_moved)
        {
            return fail(CSLAM_ERR_BAD_ARG,
                        "%s: particles were resampled, unpacked or set since cslam_pf_associate (its table is per slot)", who);
        }
        if (m != assoc_m || (m > 0 && std::memcmp(assoc_Z.data(), Z, (size_t)2 * m * sizeof(T)) != 0))
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: Z / m (%d) are not those of the last cslam_pf_associate (m=%d)", who, m,
                        assoc_m);
        }
        if (nf < assoc_nf)
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: the map shrank (%d features) since cslam_pf_associate (%d)", who, nf,
                        assoc_nf);
        }
        for (int i = 0; i < m; i++)
        {
            if (use[i] != 0 && use[i] != 1)
            {
                return fail(CSLAM_ERR_BAD_ARG, "%s: use[%d]=%d is neither 0 nor 1", who, i, use[i]);
            }
        }
        return CSLAM_OK;
    }

    int sample_proposal_assoc(const void* Z, int m, const void* Rv, const void* normals, const int* use,
                              double miss_likelihood) override
    {
        if (m < 0 || !Rv || !normals || (m > 0 && (!Z || !use)) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_assoc: bad arguments");
        }
        int rc = use_device();
        // (the mask travels in the staging area's idf slot)
        if (rc || (rc = check_assoc_inputs(Z, m, use, "pf_sample_proposal_assoc")) ||
            (rc = stage(Z, m, use, normals, (size_t)3 * np * sizeof(T))))
        {
            return rc;
        }
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_sample_proposal_assoc_kernel<T>, dim3((np * kPfSubLanes + 63) / 64), dim3(64), 0, stream,
                           store(), dObs.get(), dAIdf.get(), dIdf(), m, R[0], R[1], R[2], R[3], dNormals(),
                           (T)miss_likelihood, (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 1 : 2);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int feature_update_assoc(const void* Z, int m, const void* Rv, const int* use) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !use)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_feature_update_assoc: bad arguments");
        }
        int rc = use_device();
        if (rc || (rc = check_assoc_inputs(Z, m, use, "pf_feature_update_assoc")))
        {
            return rc;
        }
        if (m == 0)
        {
            return CSLAM_OK;
        }
        if ((rc = stage(Z, m, use)))
        {
            return rc;
        }
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_feature_update_assoc_kernel<T>, dim3((np + 63) / 64, m), dim3(64), 0, stream, store(),
                           dObs.get(), dAIdf.get(), dIdf(), m, R[0], R[1], R[2], R[3],
                           (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 0 : 1);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    // ------------------------------------------------------------------------------------------------
    // The random inputs drawn on the device (pf_draw_kernels.hpp).  A _drawn call is its host-array twin with ONE
    // producer launch in place of the caller's normals / select: pf_stage_draw_kernel fills the staging area in the
    // layout the consumers read, and these are launched behind it with the arguments they always get.  Up to
    // kPfDrawObsMax observations Z / idf ride along as kernel arguments (no copy command at all); more take the staged copy.
    // ------------------------------------------------------------------------------------------------
    bool               draw_seeded  = false;
    unsigned long long draw_seed    = 0;
    long long          draw_first   = 0; // global slot of this handle's particle 0
    long long          draw_nglobal = 0; // particles of the whole set = strata of the resample
    T                  draw_k       = (T)0; // 1 / n_global in T (stratified_random's k)
    DevBuf<T>          dDrawDi;  // [n_global, none beyond 2^31 - 1] k/2, +k, +k, ...: the running sum of stratified_random, in T and in index order
    DevBuf<T>          dDrawOut; // [3 np + n_global] what cslam_pf_get_draws brings back (never the staging area)

    int seed_draws(long long seed, long long first_global, long long n_global) override
    {
        if (first_global < 0 || n_global >= (1LL << 32) || first_global > n_global - np)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_seed_draws: need 0 <= first_global, first_global + %d <= n_global < 2^32 (got %lld, %lld)",
                        np, first_global, n_global);
        }
        int rc = use_device();
        if (rc)
        {
            return rc;
        }
        // One launch draws at most 2^31 - 1 strata (and every resample form counts its particles in an int): a larger
        // set gets its normals -- the keys reach slot 2^32 - 1 -- and no strata table.
        const long long n_strata = (n_global <= 0x7fffffffLL) ? n_global : 0;
        // all-or-nothing (device_owners.hpp): new buffers into locals first, members replaced only when all exist
        DevBuf<T>      di, out;
        std::vector<T> h;
        try
        {
            h.resize((size_t)n_strata);
        }
        catch (const std::bad_alloc&)
        {
            return fail(CSLAM_ERR_ALLOC, "pf_seed_draws: out of host memory for %lld strata", n_global);
        }
        if ((rc = di.alloc((size_t)std::max(n_strata, 1LL))) || (rc = out.alloc((size_t)3 * np + (size_t)n_strata)))
        {
            return rc;
        }
        const T k = (T)1 / (T)n_global; // PF.cpp:579-596, as pf.py's stratified_random rounds it
        T       acc = k / (T)2;
        for (long long i = 0; i < n_strata; i++)
        {
            h[(size_t)i] = acc;
            acc          = acc + k;
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still reads the old table
        if (n_strata > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(di.get(), h.data(), (size_t)n_strata * sizeof(T), hipMemcpyHostToDevice, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        }
        dDrawDi      = std::move(di);
        dDrawOut     = std::move(out);
        draw_seed    = (unsigned long long)seed;
        draw_first   = first_global;
        draw_nglobal = n_global;
        draw_k       = k;
        draw_seeded  = true;
        return CSLAM_OK;
    }

    int need_draws(const char* who)
    {
        if (!draw_seeded)
        {
            return fail(CSLAM_ERR_BAD_ARG, "%s: cslam_pf_seed_draws has not been called", who);
        }
        return CSLAM_OK;
    }
    int need_whole_set(const char* who)
    {
        int rc = need_draws(who);
        if (rc == CSLAM_OK && (draw_first != 0 || draw_nglobal != np))
        {
            rc = fail(CSLAM_ERR_BAD_ARG, "%s: the draws were seeded for slots %lld.. of %lld, this handle resamples its own %d",
                      who, draw_first, draw_nglobal, np);
        }
        return rc;
    }

    // normals (3 np, or nullptr), select (n_sel strata, or nullptr with n_sel = 0) of `step`, and -- m > 0 -- Z | idf into
    // the staging area from the kernel's own arguments
    int launch_draw(long long step, T* normals, T* select, int n_sel, int m, const void* Z, const int* idf)
    {
        PfDrawObs<T> obs;
        std::memset(&obs, 0, sizeof(obs));
        if (m > 0)
        {
            std::memcpy(obs.z, Z, (size_t)2 * m * sizeof(T));
            std::memcpy(obs.idf, idf, (size_t)m * sizeof(int));
        }
        const int nn = normals ? np : 0;
        const int lanes = std::max(std::max(nn, n_sel), std::max(2 * m, 1));
        hipLaunchKernelGGL(pf_stage_draw_kernel<T>, dim3((lanes + 255) / 256), dim3(256), 0, stream, draw_seed,
                           (unsigned long long)step, (unsigned long long)draw_first, normals, nn, select, dDrawDi.get(),
                           n_sel, draw_k, dObs.get(), dIdf(), m, obs);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    // Z | idf (or the use[] mask) of a proposal call and the normals of `step` into the staging area
    int stage_drawn(const void* Z, int m, const int* idf, long long step)
    {
        int rc = ensure_m(m);
        if (rc)
        {
            return rc;
        }
        if (m > kPfDrawObsMax)
        {
            if ((rc = stage(Z, m, idf)))
            {
                return rc;
            }
            return launch_draw(step, dNormals(), nullptr, 0, 0, nullptr, nullptr);
        }
        staged.clear();
        if ((rc = launch_draw(step, dNormals(), nullptr, 0, m, Z, idf)))
        {
            return rc;
        }
        if (m > 0) // (what stage() remembers: a feature update right behind sends nothing)
        {
            const size_t zb = (size_t)2 * m * sizeof(T), ib = (size_t)m * sizeof(int);
            staged.resize(zb + ib);
            std::memcpy(staged.data(), Z, zb);
            std::memcpy(staged.data() + zb, idf, ib);
        }
        return CSLAM_OK;
    }

    int get_draws(long long step, void* normals, void* select) override
    {
        int rc = need_draws("pf_get_draws");
        if (rc || (rc = use_device()))
        {
            return rc;
        }
        if (select && draw_nglobal > 0x7fffffffLL)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_get_draws: a set of %lld has no strata (at most 2^31 - 1), only normals", draw_nglobal);
        }
        T* dn = dDrawOut.get();
        T* ds = dn + (size_t)3 * np;
        if ((rc = launch_draw(step, normals ? dn : nullptr, select ? ds : nullptr, select ? (int)draw_nglobal : 0, 0, nullptr,
                              nullptr)))
        {
            return rc;
        }
        if (normals)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(normals, dn, (size_t)3 * np * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        if (select)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(select, ds, (size_t)draw_nglobal * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }

    int sample_proposal_drawn(const void* Z, int m, const int* idf, const void* Rv, long long step) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_drawn: bad arguments");
        }
        int rc = need_draws("pf_sample_proposal_drawn");
        if (rc || (rc = use_device()) || (rc = check_idf(idf, m, "pf_sample_proposal_drawn")) ||
            (rc = stage_drawn(Z, m, idf, step)))
        {
            return rc;
        }
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_sample_proposal_kernel<T>, dim3((np * kPfSubLanes + 63) / 64), dim3(64), 0, stream,
                           store(), dObs.get(), dIdf(), m, R[0], R[1], R[2], R[3], dNormals(), PfPredict<T>{0, (T)0,
                           (T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0}, 0);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int sample_proposal_assoc_drawn(const void* Z, int m, const void* Rv, const int* use, double miss_likelihood,
                                    long long step) override
    {
        if (m < 0 || !Rv || (m > 0 && (!Z || !use)) || !std::isfinite(miss_likelihood))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_sample_proposal_assoc_drawn: bad arguments");
        }
        int rc = need_draws("pf_sample_proposal_assoc_drawn");
        // (the mask travels in the staging area's idf slot)
        if (rc || (rc = use_device()) || (rc = check_assoc_inputs(Z, m, use, "pf_sample_proposal_assoc_drawn")) ||
            (rc = stage_drawn(Z, m, use, step)))
        {
            return rc;
        }
        const T* R = static_cast<const T*>(Rv);
        hipLaunchKernelGGL(pf_sample_proposal_assoc_kernel<T>, dim3((np * kPfSubLanes + 63) / 64), dim3(64), 0, stream,
                           store(), dObs.get(), dAIdf.get(), dIdf(), m, R[0], R[1], R[2], R[3], dNormals(),
                           (T)miss_likelihood, (quirks & CSLAM_Q_LOWER_CHOL_GAIN) ? 1 : 2);
        CSLAM_HIP_TRY(hipGetLastError());
        return CSLAM_OK;
    }

    int resample_local_drawn(long long step, double n_eff, int status, double* neff, int* did) override
    {
        int rc = need_whole_set("pf_resample_local_drawn");
        if (rc || (rc = use_device()) || (rc = ensure_resample_buffers()) ||
            (rc = launch_draw(step, nullptr, dSel.get(), np, 0, nullptr, nullptr)) ||
            (rc = launch_resample(dSel.get(), n_eff, status)))
        {
            return rc;
        }
        return resample_result(neff, did);
    }

    // cslam_pf_observation_step with launches only: the producer writes normals | select (and Z | idf up to
    // kPfDrawObsMax observations) where the staged copy of the host-array form puts them
    int observation_step_drawn(double v, double swa, const void* Qv, double wb, double dt, const void* Z, int m,
                               const int* idf, const void* Rv, long long step, double n_eff, int status) override
    {
        if (!Qv || !Rv || m < 0 || (m > 0 && (!Z || !idf)))
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_observation_step_drawn: bad arguments");
        }
        int rc = need_whole_set("pf_observation_step_drawn");
        if (rc || (rc = use_device()) || (rc = check_idf(idf, m, "pf_observation_step_drawn")) ||
            (rc = ensure_m(std::max(m, 1))) || (rc = ensure_resample_buffers()))
        {
            return rc;
        }
        staged.clear();
        const bool by_copy = m > kPfDrawObsMax;
        if (by_copy && (rc = stage(Z, m, idf)))
        {
            return rc;
        }
        T* nrm = dNormals();
        if ((rc = launch_draw(step, m > 0 ? nrm : nullptr, nrm + (size_t)3 * np, np, by_copy ? 0 : m, Z, idf)))
        {
            return rc;
        }
        return launch_observation_step(v, swa, Qv, wb, dt, m, idf, Rv, n_eff, status);
    }

    int get_stage_copies(long long* copies) override
    {
        if (!copies)
        {
            return fail(CSLAM_ERR_BAD_ARG, "pf_stage_copies: null");
        }
        *copies = stage_copies;
        return CSLAM_OK;
    }
};

inline PfBase* B(cslam_pf_t h)
{
    return reinterpret_cast<PfBase*>(h);
}

} // namespace

extern "C" {

#define CSLAM_NEED(h)                                                \
    if (!(h))                                                        \
    {                                                                \
        return fail(CSLAM_ERR_BAD_ARG, "%s: null handle", __func__); \
    }

int cslam_pf_create(int n_particles, int max_features, int dtype, int device, int quirks, cslam_pf_t* out)
{
    if (!out || n_particles < 1 || max_features < 0 || (dtype != CSLAM_F32 && dtype != CSLAM_F64) ||
        (quirks & ~CSLAM_Q_REF_EXACT))
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_create: bad arguments");
    }
    *out  = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c == 0)
    {
        return fail(CSLAM_ERR_NO_DEVICE, "pf_create: no HIP device (this engine has no CPU fallback)");
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
    {
        device = 0;
    }
    if (device >= c)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_create: device %d of %d", device, c);
    }
    PfBase* b = (dtype == CSLAM_F32) ? static_cast<PfBase*>(new (std::nothrow) Pf<float>())
                                     : static_cast<PfBase*>(new (std::nothrow) Pf<double>());
    if (!b)
    {
        return fail(CSLAM_ERR_ALLOC, "pf_create: out of host memory");
    }
    b->dtype  = dtype;
    b->device = device;
    b->quirks = quirks;
    b->np     = n_particles;
    b->nfcap  = max_features;
    int rc    = b->init();
    if (rc)
    {
        delete b;
        return rc;
    }
    *out = reinterpret_cast<cslam_pf_t>(b);
    return CSLAM_OK;
}

int cslam_pf_destroy(cslam_pf_t h)
{
    if (!h)
    {
        return CSLAM_OK;
    }
    (void)hipSetDevice(B(h)->device);
    delete B(h);
    return CSLAM_OK;
}

int cslam_pf_synchronize(cslam_pf_t h)
{
    CSLAM_NEED(h);
    CSLAM_HIP_TRY(hipSetDevice(B(h)->device));
    CSLAM_HIP_TRY(hipStreamSynchronize(B(h)->stream));
    return CSLAM_OK;
}

int cslam_pf_get_stream(cslam_pf_t h, void** stream)
{
    CSLAM_NEED(h);
    if (!stream)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_get_stream: null");
    }
    *stream = reinterpret_cast<void*>(B(h)->stream);
    return CSLAM_OK;
}

int cslam_pf_get_counts(cslam_pf_t h, int* n_particles, int* n_features)
{
    CSLAM_NEED(h);
    if (n_particles)
    {
        *n_particles = B(h)->np;
    }
    if (n_features)
    {
        *n_features = B(h)->nf;
    }
    return CSLAM_OK;
}

int cslam_pf_set_uniform_weight(cslam_pf_t h, double w0)
{
    CSLAM_NEED(h);
    return B(h)->set_uniform_weight(w0);
}

int cslam_pf_predict(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt)
{
    CSLAM_NEED(h);
    return B(h)->predict(v, swa, Q, wb, dt);
}

int cslam_pf_observe_heading(cslam_pf_t h, double phi, int use_heading)
{
    CSLAM_NEED(h);
    return B(h)->observe_heading(phi, use_heading);
}

int cslam_pf_sample_proposal(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R, const void* normals)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal(Z, m, idf, R, normals);
}

int cslam_pf_feature_update(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R)
{
    CSLAM_NEED(h);
    return B(h)->feature_update(Z, m, idf, R);
}

int cslam_pf_add_features(cslam_pf_t h, const void* Z, int q, const void* R)
{
    CSLAM_NEED(h);
    return B(h)->add_features(Z, q, R);
}

int cslam_pf_weight_sums(cslam_pf_t h, double* sums)
{
    CSLAM_NEED(h);
    return B(h)->weight_sums(sums);
}

int cslam_pf_scale_weights(cslam_pf_t h, double scale)
{
    CSLAM_NEED(h);
    return B(h)->scale_weights(scale);
}

int cslam_pf_weights_device_ptr(cslam_pf_t h, void** dptr)
{
    CSLAM_NEED(h);
    return B(h)->weights_ptr(dptr);
}

int cslam_pf_get_weights(cslam_pf_t h, void* w_host)
{
    CSLAM_NEED(h);
    return B(h)->get_weights(w_host);
}

int cslam_pf_set_weights(cslam_pf_t h, const void* w_host)
{
    CSLAM_NEED(h);
    return B(h)->set_weights(w_host);
}

int cslam_pf_record_bytes(cslam_pf_t h, long long* bytes)
{
    CSLAM_NEED(h);
    return B(h)->record_bytes(bytes);
}

int cslam_pf_pack(cslam_pf_t h, const int* src_idx, int count, void* d_records)
{
    CSLAM_NEED(h);
    return B(h)->pack(src_idx, count, d_records);
}

int cslam_pf_unpack(cslam_pf_t h, const int* dst_idx, int count, const void* d_records)
{
    CSLAM_NEED(h);
    return B(h)->unpack(dst_idx, count, d_records);
}

int cslam_pf_resample_local(cslam_pf_t h, const void* select, double n_effective, int resample_status, double* neff,
                            int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_local(select, n_effective, resample_status, neff, resampled);
}

int cslam_pf_gather_local(cslam_pf_t h, const int* keep, double w_new)
{
    CSLAM_NEED(h);
    if (!keep)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_gather_local: null");
    }
    return B(h)->gather_local(keep, w_new);
}

int cslam_pf_get_particle(cslam_pf_t h, int index, void* w, void* Xv, void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    return B(h)->get_particle(index, w, Xv, Pv, XF, PF);
}

int cslam_pf_set_particle(cslam_pf_t h, int index, const void* w, const void* Xv, const void* Pv, const void* XF,
                          const void* PF, int nf)
{
    CSLAM_NEED(h);
    return B(h)->set_particle(index, w, Xv, Pv, XF, PF, nf);
}

int cslam_pf_observation_step(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt, const void* Z, int m,
                              const int* idf, const void* R, const void* normals, const void* select, double n_effective,
                              int resample_status)
{
    CSLAM_NEED(h);
    return B(h)->observation_step(v, swa, Q, wb, dt, Z, m, idf, R, normals, select, n_effective, resample_status);
}

int cslam_pf_resample_stats(cslam_pf_t h, double* calls, double* resamples, double* last_neff)
{
    CSLAM_NEED(h);
    return B(h)->resample_stats(calls, resamples, last_neff);
}

int cslam_comm_unique_id(void* id_bytes)
{
    if (!id_bytes)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_unique_id: null");
    }
    Rccl* R = rccl();
    if (!R)
    {
        return fail(CSLAM_ERR_HIP, "comm_unique_id: librccl could not be loaded");
    }
    static_assert(sizeof(ncclUniqueId) == CSLAM_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    CSLAM_RCCL_TRY(R->GetUniqueId(&id));
    std::memcpy(id_bytes, &id, sizeof(id));
    return CSLAM_OK;
}

int cslam_comm_create(const void* id_bytes, int rank, int world, int device, cslam_comm_t* out)
{
    if (!id_bytes || !out || world < 1 || rank < 0 || rank >= world)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_create: bad arguments");
    }
    *out    = nullptr;
    Rccl* R = rccl();
    if (!R)
    {
        return fail(CSLAM_ERR_HIP, "comm_create: librccl could not be loaded");
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
    {
        device = 0;
    }
    CSLAM_HIP_TRY(hipSetDevice(device));
    Comm* c = new (std::nothrow) Comm();
    if (!c)
    {
        return fail(CSLAM_ERR_ALLOC, "comm_create: out of host memory");
    }
    ncclUniqueId id;
    std::memcpy(&id, id_bytes, sizeof(id));
    ncclResult_t r = R->CommInitRank(&c->comm, world, id, rank);
    if (r != ncclSuccess)
    {
        delete c;
        return fail(CSLAM_ERR_HIP, "ncclCommInitRank failed: %s", R->GetErrorString ? R->GetErrorString(r) : "rccl error");
    }
    c->rank   = rank;
    c->world  = world;
    c->device = device;
    *out      = reinterpret_cast<cslam_comm_t>(c);
    return CSLAM_OK;
}

int cslam_comm_create_loopback(int world, int device, cslam_comm_t* out)
{
    if (!out || world < 1 || world > kLoopMaxWorld)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_create_loopback: world must be 1..%d", kLoopMaxWorld);
    }
    for (int r = 0; r < world; r++)
    {
        out[r] = nullptr;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess)
    {
        device = 0;
    }
    LoopShared* sh = new (std::nothrow) LoopShared();
    if (!sh)
    {
        return fail(CSLAM_ERR_ALLOC, "comm_create_loopback: out of host memory");
    }
    sh->world = world;
    sh->refs  = world;
    sh->src.assign((size_t)world, nullptr);
    sh->sends.assign((size_t)world * world, LoopShared::P2P{});
    for (int r = 0; r < world; r++)
    {
        Comm* c = new (std::nothrow) Comm();
        if (!c)
        {
            for (int q = 0; q < r; q++)
            {
                delete reinterpret_cast<Comm*>(out[q]);
                out[q] = nullptr;
            }
            delete sh;
            return fail(CSLAM_ERR_ALLOC, "comm_create_loopback: out of host memory");
        }
        c->loop   = sh;
        c->rank   = r;
        c->world  = world;
        c->device = device;
        out[r]    = reinterpret_cast<cslam_comm_t>(c);
    }
    return CSLAM_OK;
}

int cslam_comm_destroy(cslam_comm_t c)
{
    if (!c)
    {
        return CSLAM_OK;
    }
    Comm* cc = reinterpret_cast<Comm*>(c);
    if (cc->loop)
    {
        bool last = false;
        {
            std::lock_guard<std::mutex> lk(cc->loop->mu);
            last = (--cc->loop->refs == 0);
        }
        if (last)
        {
            delete cc->loop;
        }
    }
    else if (Rccl* R = rccl())
    {
        (void)R->CommDestroy(cc->comm);
    }
    delete cc;
    return CSLAM_OK;
}

int cslam_comm_info(cslam_comm_t c, int* rank, int* world)
{
    if (!c)
    {
        return fail(CSLAM_ERR_BAD_ARG, "comm_info: null communicator");
    }
    const Comm* cc = reinterpret_cast<const Comm*>(c);
    if (rank)
    {
        *rank = cc->rank;
    }
    if (world)
    {
        *world = cc->world;
    }
    return CSLAM_OK;
}

int cslam_pf_debug_last_exchange(cslam_pf_t h, int* counts, int* send_idx, int capacity, int* n_send)
{
    CSLAM_NEED(h);
    return B(h)->debug_last_exchange(counts, send_idx, capacity, n_send);
}

int cslam_pf_resample_sharded(cslam_pf_t h, cslam_comm_t comm, const void* select, double n_effective,
                              int resample_status, double* neff, int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_sharded(reinterpret_cast<Comm*>(comm), select, n_effective, resample_status, neff, resampled);
}

int cslam_pf_best_particle(cslam_pf_t h, int pick, int* index, void* w, void* Xv, void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    long long i  = 0;
    const int rc = B(h)->best_particle(nullptr, pick, &i, w, Xv, Pv, XF, PF);
    if (rc == CSLAM_OK && index)
    {
        *index = (int)i;
    }
    return rc;
}

int cslam_pf_estimate(cslam_pf_t h, double* w_sum, double* neff, void* Xv, void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    return B(h)->estimate(nullptr, w_sum, neff, Xv, Pv, XF, PF);
}

int cslam_pf_get_all_features(cslam_pf_t h, void* XF_all)
{
    CSLAM_NEED(h);
    return B(h)->get_all_features(XF_all);
}

/* EKF.cpp:131-144, 235-326 on every particle's own state */
int cslam_pf_associate(cslam_pf_t h, const void* Z, int m, const void* R, double gate1, double gate2)
{
    CSLAM_NEED(h);
    return B(h)->associate(Z, m, R, gate1, gate2);
}

/* the tables of the last associate (EKF.cpp:131-144, 235-326 per particle) */
int cslam_pf_get_association(cslam_pf_t h, int* idf_host, int* kind_host, double* summary_host)
{
    CSLAM_NEED(h);
    return B(h)->get_association(idf_host, kind_host, summary_host);
}

/* PF.cpp:502-544 + 222-277 with every particle's own correspondences (EKF.cpp:131-144, 235-326) */
int cslam_pf_sample_proposal_assoc(cslam_pf_t h, const void* Z, int m, const void* R, const void* normals, const int* use,
                                   double miss_likelihood)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_assoc(Z, m, R, normals, use, miss_likelihood);
}

/* PF.cpp:222-277 alone with every particle's own correspondences (EKF.cpp:131-144, 235-326) */
int cslam_pf_feature_update_assoc(cslam_pf_t h, const void* Z, int m, const void* R, const int* use)
{
    CSLAM_NEED(h);
    return B(h)->feature_update_assoc(Z, m, R, use);
}

/* slam.h:587-594: the seed of every draw the _drawn calls make */
int cslam_pf_seed_draws(cslam_pf_t h, long long seed, long long first_global, long long n_global)
{
    CSLAM_NEED(h);
    return B(h)->seed_draws(seed, first_global, n_global);
}

/* slam.h:753-764 and PF.cpp:557, 579-596 of one step, read back */
int cslam_pf_get_draws(cslam_pf_t h, long long step, void* normals, void* select)
{
    CSLAM_NEED(h);
    return B(h)->get_draws(step, normals, select);
}

/* PF.cpp:502-544 with the normals of slam.h:753-764 drawn on the device */
int cslam_pf_sample_proposal_drawn(cslam_pf_t h, const void* Z, int m, const int* idf, const void* R, long long step)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_drawn(Z, m, idf, R, step);
}

int cslam_pf_sample_proposal_assoc_drawn(cslam_pf_t h, const void* Z, int m, const void* R, const int* use,
                                         double miss_likelihood, long long step)
{
    CSLAM_NEED(h);
    return B(h)->sample_proposal_assoc_drawn(Z, m, R, use, miss_likelihood, step);
}

/* PF.cpp:473-500 with the strata of PF.cpp:557, 579-596 drawn on the device */
int cslam_pf_resample_local_drawn(cslam_pf_t h, long long step, double n_effective, int resample_status, double* neff,
                                  int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_local_drawn(step, n_effective, resample_status, neff, resampled);
}

int cslam_pf_resample_sharded_drawn(cslam_pf_t h, cslam_comm_t comm, long long step, double n_effective,
                                    int resample_status, double* neff, int* resampled)
{
    CSLAM_NEED(h);
    return B(h)->resample_sharded_drawn(reinterpret_cast<Comm*>(comm), step, n_effective, resample_status, neff, resampled);
}

int cslam_pf_observation_step_drawn(cslam_pf_t h, double v, double swa, const void* Q, double wb, double dt,
                                    const void* Z, int m, const int* idf, const void* R, long long step,
                                    double n_effective, int resample_status)
{
    CSLAM_NEED(h);
    return B(h)->observation_step_drawn(v, swa, Q, wb, dt, Z, m, idf, R, step, n_effective, resample_status);
}

int cslam_pf_stage_copies(cslam_pf_t h, long long* copies)
{
    CSLAM_NEED(h);
    return B(h)->get_stage_copies(copies);
}

int cslam_pf_best_particle_sharded(cslam_pf_t h, cslam_comm_t comm, int pick, long long* global_index, void* w, void* Xv,
                                   void* Pv, void* XF, void* PF)
{
    CSLAM_NEED(h);
    if (!comm)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_best_particle_sharded: null communicator");
    }
    return B(h)->best_particle(reinterpret_cast<Comm*>(comm), pick, global_index, w, Xv, Pv, XF, PF);
}

int cslam_pf_estimate_sharded(cslam_pf_t h, cslam_comm_t comm, double* w_sum, double* neff, void* Xv, void* Pv, void* XF,
                              void* PF)
{
    CSLAM_NEED(h);
    if (!comm)
    {
        return fail(CSLAM_ERR_BAD_ARG, "pf_estimate_sharded: null communicator");
    }
    return B(h)->estimate(reinterpret_cast<Comm*>(comm), w_sum, neff, Xv, Pv, XF, PF);
}

} // extern "C"
