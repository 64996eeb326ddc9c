// ekf_staging.hpp -- the observation staging ring and the stage profiler of the single-filter handle (host code).
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "device_owners.hpp"
#include "ekf_kernels.hpp"

namespace cslam
{

// Observation staging: a pinned host ring + one device buffer, kSlots slots of mcap observations each (Z, then idf).
// A device slot per host slot: queued look-ahead updates read their inputs up to two calls later; a slot comes round
// again kSlots calls later, stream-ordered behind every kernel that read it.
template <typename T>
struct StageRing
{
    static constexpr int kSlots = 64;
    int                      mcap = 0;
    PinnedBuf<unsigned char> hStage;
    DevBuf<unsigned char>    dStage;
    Event                    ev[kSlots]; // created by the first call that takes the slot, recorded by every one
    int                      next = 0;

    size_t slot_bytes(int mc) const { return (size_t)mc * (2 * sizeof(T) + sizeof(int)); }
    unsigned char* dev_slot(int slot) const { return dStage.get() + slot_bytes(mcap) * slot; }

    // the next slot of the ring (room for m observations has been ensured)
    int take_slot()
    {
        const int slot = next;
        next           = (next + 1) % kSlots;
        return slot;
    }

    // room for m > mcap observations per slot (the caller has launched everything that reads the ring and waited for it)
    int grow(int m)
    {
        int newm = std::max(m, 2 * mcap);
        PinnedBuf<unsigned char> hs;
        DevBuf<unsigned char>    ds;
        int                      rc = hs.alloc(slot_bytes(newm) * kSlots);
        if (rc || (rc = ds.alloc(slot_bytes(newm) * kSlots)))
        {
            return rc;
        }
        hStage = std::move(hs);
        dStage = std::move(ds);
        mcap = newm;
        return CSLAM_OK;
    }

    // copies (Z, idf) of one call (m <= mcap) into the next slot of the ring on `stream`; returns device pointers.  Host
    // inputs go through the slot's pinned buffer (H2D copy); device inputs (on_device) are copied by one small kernel.
    int stage(const void* Z, const int* idf, int m, bool on_device, hipStream_t stream, long long& launches, const T** dZ,
              const int** dIdf)
    {
        int rc   = CSLAM_OK;
        int slot = take_slot();
        if (ev[slot])
        {
            CSLAM_HIP_TRY(hipEventSynchronize(ev[slot].get()));
        }
        else if ((rc = ev[slot].create(hipEventDisableTiming)))
        {
            return rc;
        }
        size_t         zb = (size_t)m * 2 * sizeof(T);
        unsigned char* ds = dev_slot(slot);
        if (on_device)
        {
            hipLaunchKernelGGL(ekf_stage_obs_kernel<T>, dim3((3 * m + 255) / 256), dim3(256), 0, stream,
                               static_cast<const T*>(Z), idf, m, reinterpret_cast<T*>(ds), reinterpret_cast<int*>(ds + zb));
            CSLAM_HIP_TRY(hipGetLastError());
            launches++;
        }
        else
        {
            unsigned char* hs = hStage.get() + slot_bytes(mcap) * slot;
            memcpy(hs, Z, zb);
            memcpy(hs + zb, idf, (size_t)m * sizeof(int));
            CSLAM_HIP_TRY(hipMemcpyAsync(ds, hs, zb + (size_t)m * sizeof(int), hipMemcpyHostToDevice, stream));
        }
        CSLAM_HIP_TRY(hipEventRecord(ev[slot].get(), stream));
        *dZ   = reinterpret_cast<const T*>(ds);
        *dIdf = reinterpret_cast<const int*>(ds + zb);
        return CSLAM_OK;
    }
};

// Stage profiler: HIP event pairs around launches, summed per stage (cslam_ekf_get_stage_times).
// mode 1: every stage; 2: every P-GEMM launch; 3: one P-GEMM launch in sixteen (an event pair costs about 11 us of
// stream time around the kernel it brackets -- rocprofv3 trace: 5.9 us before, 5.6 us after -- so the timed region
// of the bench samples instead of bracketing every launch); 4: one in four
struct StageProfiler
{
    int                mode    = 0;
    unsigned           count   = 0;
    bool               sampled = false;
    std::vector<Event> ev_pool;
    std::vector<int>   ev_stage; // stage id of interval [2i, 2i+1]
    size_t             ev_used = 0;

    bool skip(int stage, bool begin)
    {
        if (!mode)
        {
            return true;
        }
        if (mode >= 2 && stage != CSLAM_STAGE_DOWNDATE)
        {
            return true;
        }
        if (mode == 3 || mode == 4)
        {
            if (begin)
            {
                sampled = (count++ % (mode == 3 ? 16u : 4u)) == 0;
            }
            return !sampled;
        }
        return false;
    }
    int begin(int stage, hipStream_t st)
    {
        if (skip(stage, true))
        {
            return CSLAM_OK;
        }
        if (ev_used + 2 > ev_pool.size())
        {
            for (int i = 0; i < 2; i++)
            {
                Event e;
                CSLAM_TRY(e.create(hipEventDefault));
                ev_pool.push_back(std::move(e));
            }
        }
        ev_stage.resize(ev_pool.size() / 2);
        ev_stage[ev_used / 2] = stage;
        CSLAM_HIP_TRY(hipEventRecord(ev_pool[ev_used].get(), st));
        return CSLAM_OK;
    }
    int end(int stage, hipStream_t st)
    {
        if (skip(stage, false))
        {
            return CSLAM_OK;
        }
        CSLAM_HIP_TRY(hipEventRecord(ev_pool[ev_used + 1].get(), st));
        ev_used += 2;
        return CSLAM_OK;
    }
    // (both: the caller has waited for every stream)
    void set_mode(int on) { mode = on; ev_used = 0; count = 0; }
    int  times(double* ms, int* launches) const
    {
        for (int s = 0; s < CSLAM_N_STAGES; s++)
        {
            ms[s]       = 0.0;
            launches[s] = 0;
        }
        for (size_t i = 0; i + 1 < ev_used; i += 2)
        {
            float t = 0.f;
            CSLAM_HIP_TRY(hipEventElapsedTime(&t, ev_pool[i].get(), ev_pool[i + 1].get()));
            int s = ev_stage[i / 2];
            ms[s] += (double)t;
            launches[s] += 1;
        }
        return CSLAM_OK;
    }
};

} // namespace cslam
