// device_owners.hpp -- move-only owners of the GPU resources a handle holds: device and pinned buffers, events, streams.
// Host code only.  An owner is empty or holds exactly one resource, which its destructor releases (errors ignored).
// The owners do not remember a device: a handle's destructor selects the device and synchronises its streams, then its
// members die in reverse declaration order -- so a handle declares its streams BEFORE its buffers and events.
//
// Growing a workspace is all-or-nothing: allocate the complete new set into local owners, return on the first failure
// (the locals free themselves, the handle is untouched), and only then move-assign into the members and set the capacity
// fields.  Move-assignment releases what the target held, so the old set lives until that point.
#pragma once

#include <cassert>
#include <cstddef>
#include <utility>

#include "cslam_common.hpp"

// returns the error code of a step that reports one (an owner's alloc / create: the text is already set)
#define CSLAM_TRY(expr)         \
    do                          \
    {                           \
        if (int rc__ = (expr))  \
        {                       \
            return rc__;        \
        }                       \
    } while (0)

namespace cslam
{

namespace detail
{
// the one raw handle of an owner; Release is called on a non-empty one exactly once
template <typename H, typename Release>
class Owned
{
  public:
    Owned() = default;
    Owned(const Owned&)            = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H())) {}
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o)
        {
            reset();
            h_ = std::exchange(o.h_, H());
        }
        return *this;
    }
    ~Owned() { reset(); }

    void reset()
    {
        if (h_ != H())
        {
            Release()(h_);
            h_ = H();
        }
    }
    H        get() const { return h_; }
    explicit operator bool() const { return h_ != H(); }

  protected:
    H h_ = H();
};

struct FreeDevice
{
    void operator()(void* p) const { (void)hipFree(p); }
};
struct FreePinned
{
    void operator()(void* p) const { (void)hipHostFree(p); }
};
struct DestroyEvent
{
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
struct DestroyStream
{
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
} // namespace detail

// `count` elements of T from hipMalloc.  alloc() is exactly one hipMalloc, into an EMPTY owner (growth paths allocate
// into a local owner and move it in).
template <typename T>
class DevBuf : public detail::Owned<T*, detail::FreeDevice>
{
  public:
    int alloc(size_t count)
    {
        assert(!*this);
        void* p = nullptr;
        CSLAM_HIP_TRY(hipMalloc(&p, count * sizeof(T)));
        this->h_ = static_cast<T*>(p);
        count_   = count;
        return CSLAM_OK;
    }
    // hipMalloc + hipMemsetAsync on `st`
    int alloc_zeroed(size_t count, hipStream_t st)
    {
        CSLAM_TRY(alloc(count));
        CSLAM_HIP_TRY(hipMemsetAsync(this->h_, 0, count * sizeof(T), st));
        return CSLAM_OK;
    }
    // hipMalloc + the blocking hipMemset
    int alloc_zeroed_blocking(size_t count)
    {
        CSLAM_TRY(alloc(count));
        CSLAM_HIP_TRY(hipMemset(this->h_, 0, count * sizeof(T)));
        return CSLAM_OK;
    }
    size_t count() const { return *this ? count_ : 0; }

  private:
    size_t count_ = 0;
};

// the same for hipHostMalloc(..., hipHostMallocDefault)
template <typename T>
class PinnedBuf : public detail::Owned<T*, detail::FreePinned>
{
  public:
    int alloc(size_t count)
    {
        assert(!*this);
        void* p = nullptr;
        CSLAM_HIP_TRY(hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault));
        this->h_ = static_cast<T*>(p);
        count_   = count;
        return CSLAM_OK;
    }
    size_t count() const { return *this ? count_ : 0; }
    T&     operator[](size_t i) const { return this->h_[i]; } // (host memory)

  private:
    size_t count_ = 0;
};

class Event : public detail::Owned<hipEvent_t, detail::DestroyEvent>
{
  public:
    // flags: hipEventDefault (a timing event) or hipEventDisableTiming
    int create(unsigned flags)
    {
        assert(!*this);
        CSLAM_HIP_TRY(hipEventCreateWithFlags(&h_, flags));
        return CSLAM_OK;
    }
};

class Stream : public detail::Owned<hipStream_t, detail::DestroyStream>
{
  public:
    int create(unsigned flags)
    {
        assert(!*this);
        CSLAM_HIP_TRY(hipStreamCreateWithFlags(&h_, flags));
        return CSLAM_OK;
    }
    int create_with_priority(unsigned flags, int priority)
    {
        assert(!*this);
        CSLAM_HIP_TRY(hipStreamCreateWithPriority(&h_, flags, priority));
        return CSLAM_OK;
    }
};

} // namespace cslam
