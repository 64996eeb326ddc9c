// pf_staging.hpp -- how the small per-call host inputs of the particle handle reach the device (host code): the pinned
// staging ring, and the device staging area with the memo of what it holds.
#pragma once

#include <algorithm>

#include "device_owners.hpp"
#include "pf_host_parts.hpp"

namespace cslam
{

// Pinned staging ring.  The small host inputs of a call (Z, idf, normals, select) are copied into the next slot and
// sent with ONE asynchronous copy, so the call returns without waiting for the stream (the caller's arrays are
// consumed before return all the same).
class PfStageRing
{
  public:
    static constexpr int kSlots = 16;

    // `bytes` to `dst` on `stream` through the next slot; fill(char* slot) writes them into the slot
    template <typename Fill>
    int send(void* dst, size_t bytes, hipStream_t stream, Fill fill)
    {
        char* slot = nullptr;
        CSLAM_TRY(slot_for(bytes, stream, &slot));
        fill(slot);
        CSLAM_HIP_TRY(hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, stream));
        return commit(stream);
    }
    // host-to-device copy commands enqueued for per-step inputs
    long long copies() const { return copies_; }

  private:
    int slot_for(size_t bytes, hipStream_t stream, char** out)
    {
        if (bytes > slot_)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // (the slots' events are all complete after this)
            size_t          newsz = std::max((bytes + 4095) / 4096 * 4096, 2 * slot_);
            PinnedBuf<char> ring;
            CSLAM_TRY(ring.alloc(newsz * kSlots));
            ring_ = std::move(ring);
            slot_ = newsz;
            pos_  = 0;
        }
        // a slot is reused one lap later: wait for the copy that read it last (long done in the steady state) instead of
        // draining the stream once per lap (which cost a ~60 us bubble every 16 calls)
        if (ev_[pos_])
        {
            CSLAM_HIP_TRY(hipEventSynchronize(ev_[pos_].get()));
        }
        last_ = pos_;
        *out  = ring_.get() + (size_t)pos_ * slot_;
        pos_  = (pos_ + 1) % kSlots;
        return CSLAM_OK;
    }
    // the copy out of the slot handed out last has been enqueued: mark it
    int commit(hipStream_t stream)
    {
        if (!ev_[last_])
        {
            CSLAM_TRY(ev_[last_].create(hipEventDisableTiming));
        }
        CSLAM_HIP_TRY(hipEventRecord(ev_[last_].get(), stream));
        copies_++;
        return CSLAM_OK;
    }

    PinnedBuf<char> ring_;
    size_t          slot_ = 0; // bytes per slot
    int             pos_  = 0;
    int             last_ = 0;   // slot handed out by the last slot_for()
    Event           ev_[kSlots]; // created (and recorded) by the first copy out of the slot
    long long       copies_ = 0;
};

// The device staging area (PfObsLayout) and the index list of pack / unpack (max(mcap, np) ints), grown together.
// The memo is cleared here whenever a copy lands in the area or the area is replaced; a caller that lets a KERNEL
// write the area says forget() first and remember() after.
template <typename T>
class PfObsArea
{
  public:
    void set_particles(int np) { lay_.np = np; }
    const PfObsLayout<T>& layout() const { return lay_; }

    T*   z() const { return dObs_.get(); }
    int* dIdf() const { return reinterpret_cast<int*>(base() + lay_.off_idf()); }
    T*   dNormals() const { return reinterpret_cast<T*>(base() + lay_.off_normals()); }
    T*   dSelect() const { return reinterpret_cast<T*>(base() + lay_.off_select()); }
    int* dIdx() const { return dIdx_.get(); }

    int ensure(int m, hipStream_t stream)
    {
        if (m <= lay_.mcap)
        {
            return CSLAM_OK;
        }
        const int newm = PfObsLayout<T>::grown(m, lay_.mcap);
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        DevBuf<T>   obs;
        DevBuf<int> idx;
        CSLAM_TRY(obs.alloc(PfObsLayout<T>::alloc_count(newm, lay_.np)));
        CSLAM_TRY(idx.alloc((size_t)std::max(newm, lay_.np)));
        memo_.clear();
        dObs_     = std::move(obs);
        dIdx_     = std::move(idx);
        lay_.mcap = newm;
        return CSLAM_OK;
    }

    // one staged copy of the first `bytes` of the area; fill(char* slot) lays them out as PfObsLayout says
    template <typename Fill>
    int receive(PfStageRing& ring, size_t bytes, hipStream_t stream, Fill fill)
    {
        memo_.clear();
        return ring.send(dObs_.get(), bytes, stream, fill);
    }

    bool holds(const void* Z, int m, const int* idf) const { return memo_.holds(Z, lay_.bytes_z(m), idf, ib(idf, m)); }
    void remember(const void* Z, int m, const int* idf) { memo_.remember(Z, lay_.bytes_z(m), idf, ib(idf, m)); }
    void forget() { memo_.clear(); }

  private:
    char*         base() const { return reinterpret_cast<char*>(dObs_.get()); }
    static size_t ib(const int* idf, int m) { return idf ? (size_t)m * sizeof(int) : 0; }

    DevBuf<T>      dObs_;
    DevBuf<int>    dIdx_;
    PfObsLayout<T> lay_;
    PfStagedMemo   memo_;
};

} // namespace cslam
