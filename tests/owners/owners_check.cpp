// owners_check.cpp -- host-only check of conan_slam_amd/csrc/device_owners.hpp (built and run by tests/test_owners_cpu.py).
// Without a HIP device: empty owners, and an allocation that fails comes back as CSLAM_ERR_HIP with the owner still
// empty.  With one: a few KB of real allocations -- zero fill, moves, reset, and the allocate / move-assign / set-capacity
// sequence every growth path of the handles uses.  No kernel is launched.
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "device_owners.hpp"

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

// is p an allocation the runtime knows (i.e. not freed yet)?
static bool alive(const void* p)
{
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    const bool ok = hipPointerGetAttributes(&a, p) == hipSuccess && a.type != hipMemoryTypeUnregistered;
    (void)hipGetLastError(); // (a failed query leaves its error behind)
    return ok;
}

// a handle in miniature: two buffers and the capacity they were sized for
struct Grower
{
    DevBuf<float> a;
    DevBuf<int>   b;
    size_t        cap = 0;

    // the growth rule: the whole new set into locals, members and capacity only once every allocation has succeeded
    int ensure(size_t n, hipStream_t st, const float** old_a_seen_alive)
    {
        if (n <= cap)
        {
            return CSLAM_OK;
        }
        DevBuf<float> na;
        DevBuf<int>   nb;
        int           rc = na.alloc_zeroed(n, st);
        if (rc || (rc = nb.alloc(n)))
        {
            return rc;
        }
        *old_a_seen_alive = (a && alive(a.get())) ? a.get() : nullptr; // the old set is still there beside the new one
        a   = std::move(na);
        b   = std::move(nb);
        cap = n;
        return CSLAM_OK;
    }
};

static void check_empty()
{
    DevBuf<float>   d;
    PinnedBuf<char> p;
    Event           e;
    Stream          s;
    CHECK(!d && d.get() == nullptr && d.count() == 0);
    CHECK(!p && p.get() == nullptr && p.count() == 0);
    CHECK(!e && e.get() == nullptr);
    CHECK(!s && s.get() == nullptr);
    d.reset(); // (no-ops, as the destructors at the end of this scope are)
    p.reset();
    e.reset();
    s.reset();
    DevBuf<float> d2(std::move(d));
    d = std::move(d2);
    CHECK(!d && !d2);
}

static void check_without_device()
{
    last_error_buf()[0] = 0;
    DevBuf<float> d;
    CHECK(d.alloc(256) == CSLAM_ERR_HIP);
    CHECK(!d && d.count() == 0);
    CHECK(std::strstr(last_error_buf(), "hipMalloc") != nullptr);
    last_error_buf()[0] = 0;
    PinnedBuf<int> p;
    CHECK(p.alloc(4) == CSLAM_ERR_HIP);
    CHECK(!p && std::strstr(last_error_buf(), "hipHostMalloc") != nullptr);
    Event  e;
    Stream s;
    CHECK(e.create(hipEventDisableTiming) == CSLAM_ERR_HIP && !e);
    CHECK(s.create(hipStreamNonBlocking) == CSLAM_ERR_HIP && !s);
}

static void check_with_device()
{
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == CSLAM_OK && s);
    Stream sp;
    int    lo = 0, hi = 0;
    CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess);
    CHECK(sp.create_with_priority(hipStreamNonBlocking, hi) == CSLAM_OK && sp);
    Event e;
    CHECK(e.create(hipEventDisableTiming) == CSLAM_OK && e);

    // zero fill, asynchronous and blocking
    const size_t  n = 1024;
    DevBuf<float> z;
    CHECK(z.alloc_zeroed(n, s.get()) == CSLAM_OK && z && z.count() == n);
    DevBuf<int> zb;
    CHECK(zb.alloc_zeroed_blocking(n) == CSLAM_OK && zb.count() == n);
    std::vector<float> hf(n, 1.f);
    std::vector<int>   hi32(n, 1);
    CHECK(hipMemcpyAsync(hf.data(), z.get(), n * sizeof(float), hipMemcpyDeviceToHost, s.get()) == hipSuccess);
    CHECK(hipEventRecord(e.get(), s.get()) == hipSuccess);
    CHECK(hipEventSynchronize(e.get()) == hipSuccess);
    CHECK(hipMemcpy(hi32.data(), zb.get(), n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess);
    bool zeros = true;
    for (size_t i = 0; i < n; i++)
    {
        zeros = zeros && hf[i] == 0.f && hi32[i] == 0;
    }
    CHECK(zeros);
    PinnedBuf<int> pin;
    CHECK(pin.alloc(4) == CSLAM_OK && pin && pin.count() == 4);
    pin[3] = 7;
    CHECK(pin.get()[3] == 7);

    // move construction: the source is emptied, nothing is freed
    float*        zp = z.get();
    DevBuf<float> m(std::move(z));
    CHECK(!z && z.get() == nullptr && z.count() == 0 && m.get() == zp && m.count() == n && alive(zp));
    // move assignment: the overwritten target's allocation is released (once: the source is emptied, so its destructor
    // has nothing left), the moved one stays
    DevBuf<float> t;
    CHECK(t.alloc(64) == CSLAM_OK);
    float* tp = t.get();
    CHECK(alive(tp));
    t = std::move(m);
    CHECK(!m && t.get() == zp && t.count() == n && alive(zp) && !alive(tp));
    // reset
    t.reset();
    CHECK(!t && t.get() == nullptr && t.count() == 0 && !alive(zp));
    {
        DevBuf<float> scoped;
        CHECK(scoped.alloc(64) == CSLAM_OK);
        zp = scoped.get();
    }
    CHECK(!alive(zp)); // the destructor released it

    // the growth sequence: old pointers valid until the move, capacity follows the buffers
    Grower       g;
    const float* seen = nullptr;
    CHECK(g.ensure(256, s.get(), &seen) == CSLAM_OK && g.cap == 256 && g.a.count() == 256 && g.b.count() == 256);
    const float* first = g.a.get();
    CHECK(g.ensure(128, s.get(), &seen) == CSLAM_OK && g.a.get() == first && g.cap == 256);
    CHECK(hipStreamSynchronize(s.get()) == hipSuccess);
    CHECK(g.ensure(512, s.get(), &seen) == CSLAM_OK && g.cap == 512 && g.a.count() == 512 && g.a.get() != first);
    CHECK(seen == first);   // alive while the new set was being allocated ...
    CHECK(!alive(first));   // ... and gone after the move
    CHECK(hipStreamSynchronize(s.get()) == hipSuccess);
}

int main()
{
    int        count = 0;
    hipError_t err   = hipGetDeviceCount(&count);
    (void)hipGetLastError();
    check_empty();
    if (err != hipSuccess || count == 0)
    {
        check_without_device();
        std::printf("owners_check: no device, %d failed\n", g_failed);
    }
    else
    {
        check_with_device();
        check_empty();
        std::printf("owners_check: device, %d failed\n", g_failed);
    }
    return g_failed ? 1 : 0;
}
