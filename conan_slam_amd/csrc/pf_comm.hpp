// pf_comm.hpp -- the communicator of the sharded particle calls (host code and the one kernel of the loopback back-end);
// it knows nothing of the particle handle.  For cslam_pf.hip alone: it lives in that translation unit's unnamed namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h> // types only: the library itself is bound with dlopen (see Rccl below)

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "cslam_common.hpp"

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

} // namespace
