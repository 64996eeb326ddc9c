// pf_host_parts_check.cpp -- host-only check of conan_slam_amd/csrc/pf_host_parts.hpp (built and run by
// tests/test_host_parts_cpu.py, with plain g++ and once more under the address and undefined-behaviour sanitizers).
// The layout of the particle handle's staging area, the memo of what it holds, the validity of the association tables,
// the duplicate scan, the exchange bookkeeping and the strata table -- every case for float and for double.  No HIP.
#include <cstdio>
#include <cstring>
#include <vector>

#include "pf_host_parts.hpp"

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

template <typename T>
static void check_layout()
{
    // newm = round_up_4(max(m, 64, 2 * mcap))
    const int ms[6]      = {0, 1, 64, 65, 66, 129};
    const int from0[6]   = {64, 64, 64, 68, 68, 132};
    const int from64[6]  = {128, 128, 128, 128, 128, 132};
    for (int i = 0; i < 6; i++)
    {
        CHECK(PfObsLayout<T>::grown(ms[i], 0) == from0[i]);
        CHECK(PfObsLayout<T>::grown(ms[i], 64) == from64[i]);
        for (int newm : {from0[i], from64[i]})
        {
            for (int np : {1, 65, 300})
            {
                PfObsLayout<T> lay;
                lay.mcap = newm;
                lay.np   = np;
                CHECK(lay.off_idf() == (size_t)2 * newm * sizeof(T));
                CHECK(lay.off_normals() == lay.off_idf() + (size_t)newm * sizeof(int));
                CHECK(lay.off_normals() % 16 == 0);
                CHECK(lay.off_select() == lay.off_normals() + (size_t)3 * np * sizeof(T));
                // the allocation holds the whole step: Z | idf | normals | select
                CHECK(PfObsLayout<T>::alloc_count(newm, np) * sizeof(T) >= lay.off_select() + (size_t)np * sizeof(T));
                CHECK(PfObsLayout<T>::alloc_count(newm, np) * sizeof(T) >= lay.bytes_step());
            }
        }
    }
    // the bytes of each kind of copy
    PfObsLayout<T> lay;
    lay.mcap = 64;
    lay.np   = 300;
    const size_t s = sizeof(T);
    CHECK(lay.bytes_z(0) == 0 && lay.bytes_z(3) == 6 * s);
    CHECK(lay.bytes_z_idf(0) == 128 * s && lay.bytes_z_idf(3) == 128 * s + 3 * sizeof(int));
    CHECK(lay.bytes_z_idf_normals() == 128 * s + 64 * sizeof(int) + 900 * s); // (whatever m: the normals sit behind mcap)
    CHECK(lay.bytes_step() == 128 * s + 64 * sizeof(int) + 1200 * s);
}

template <typename T>
static void check_staged_memo()
{
    const T      Z[6]   = {(T)1, (T)2, (T)3, (T)4, (T)5, (T)6};
    const int    idf[3] = {4, 2, 9};
    const size_t zb = sizeof(Z), ib = sizeof(idf);
    PfStagedMemo memo;
    CHECK(!memo.holds(Z, zb, idf, ib)); // nothing remembered
    memo.remember(Z, zb, idf, ib);
    T   Zc[6];
    int idc[3];
    std::memcpy(Zc, Z, zb);
    std::memcpy(idc, idf, ib);
    CHECK(memo.holds(Zc, zb, idc, ib)); // identical bytes at another address
    Zc[5] = (T)7;
    CHECK(!memo.holds(Zc, zb, idc, ib)); // one Z scalar
    Zc[5]  = Z[5];
    idc[0] = 5;
    CHECK(!memo.holds(Zc, zb, idc, ib)); // one idf
    CHECK(!memo.holds(Z, zb, nullptr, 0)); // remembered with idf, asked without
    CHECK(!memo.holds(Z, 4 * sizeof(T), idf, 2 * sizeof(int))); // fewer observations
    memo.remember(Z, zb, nullptr, 0);
    CHECK(memo.holds(Z, zb, nullptr, 0));
    CHECK(!memo.holds(Z, zb, idf, ib)); // remembered without idf, asked with
    memo.remember(Z, zb, idf, ib);
    memo.clear();
    CHECK(!memo.holds(Z, zb, idf, ib));
    // m = 0: nothing to remember, so nothing is held
    memo.remember(Z, zb, idf, ib);
    memo.remember(nullptr, 0, nullptr, 0);
    CHECK(!memo.holds(nullptr, 0, nullptr, 0));
    CHECK(!memo.holds(Z, zb, idf, ib));
}

template <typename T>
static void check_assoc_memo()
{
    const T   Z[6]   = {(T)1, (T)2, (T)3, (T)4, (T)5, (T)6};
    const int use[3] = {1, 0, 1};
    int       bad    = -1;
    PfAssocMemo<T> memo;
    CHECK(memo.m() == -1);
    CHECK(memo.check(Z, 3, 5, use, &bad) == PfAssocRefusal::never_associated);
    memo.associated(Z, 3, 5);
    CHECK(memo.m() == 3 && memo.nf() == 5);
    T Zc[6];
    std::memcpy(Zc, Z, sizeof(Z));
    CHECK(memo.check(Zc, 3, 5, use, &bad) == PfAssocRefusal::none);
    CHECK(memo.check(Zc, 2, 5, use, &bad) == PfAssocRefusal::other_scan); // m differs
    CHECK(memo.check(Zc, 0, 5, use, &bad) == PfAssocRefusal::other_scan);
    Zc[2] = (T)3.5;
    CHECK(memo.check(Zc, 3, 5, use, &bad) == PfAssocRefusal::other_scan); // one Z scalar
    CHECK(memo.check(Z, 3, 4, use, &bad) == PfAssocRefusal::map_shrank);
    CHECK(memo.check(Z, 3, 6, use, &bad) == PfAssocRefusal::none); // the map grew
    const int use2[3] = {1, 2, 1}, usem[3] = {1, 0, -1};
    CHECK(memo.check(Z, 3, 5, use2, &bad) == PfAssocRefusal::bad_use && bad == 1);
    CHECK(memo.check(Z, 3, 5, usem, &bad) == PfAssocRefusal::bad_use && bad == 2);
    // the refusals in the order the handle reports them: moved before anything about the inputs
    memo.moved();
    CHECK(memo.check(Z, 3, 5, use, &bad) == PfAssocRefusal::moved);
    CHECK(memo.check(Zc, 2, 4, use2, &bad) == PfAssocRefusal::moved);
    memo.associated(Z, 3, 5); // a new associate makes the table valid again
    CHECK(memo.check(Z, 3, 5, use, &bad) == PfAssocRefusal::none);
    memo.forget(); // the tables were replaced
    CHECK(memo.m() == -1 && memo.check(Z, 3, 5, use, &bad) == PfAssocRefusal::never_associated);
    // m = 0: accepted with null Z and null use
    memo.associated(nullptr, 0, 5);
    CHECK(memo.m() == 0);
    CHECK(memo.check(nullptr, 0, 5, nullptr, &bad) == PfAssocRefusal::none);
    CHECK(memo.check(Z, 3, 5, use, &bad) == PfAssocRefusal::other_scan);
    memo.moved();
    CHECK(memo.check(nullptr, 0, 5, nullptr, &bad) == PfAssocRefusal::moved);
}

static void check_has_duplicate()
{
    CHECK(!pf_has_duplicate(nullptr, 0));
    const int one[1] = {7};
    CHECK(!pf_has_duplicate(one, 1));
    std::vector<int> idf(33);
    for (int i = 0; i < 33; i++)
    {
        idf[(size_t)i] = 100 - i;
    }
    CHECK(!pf_has_duplicate(idf.data(), 33));
    idf[32] = idf[0]; // (0, m - 1)
    CHECK(pf_has_duplicate(idf.data(), 33));
    CHECK(!pf_has_duplicate(idf.data(), 32));
    idf[32] = 1;
    idf[17] = idf[16]; // adjacent
    CHECK(pf_has_duplicate(idf.data(), 33));
    const int two[2] = {3, 3};
    CHECK(pf_has_duplicate(two, 2));
}

static void check_exchange()
{
    size_t soff = 9, roff = 9;
    int    n_send = -1, n_recv = -1;
    // world = 1: everything stays
    const int one[2] = {5, 5};
    pf_exchange_offsets(one, 1, 0, &soff, &roff);
    CHECK(soff == 0 && roff == 0);
    CHECK(pf_exchange_plan_ok(one, 1, 0, 5, &n_send, &n_recv) && n_send == 5 && n_recv == 5);
    CHECK(!pf_exchange_plan_ok(one, 1, 0, 4, &n_send, &n_recv));
    // world = 3, L = 4, rank 1 of a skewed plan: it sends 7, 2, 0 records to ranks 0, 1, 2 and receives 1, 2, 1
    const int hc[6] = {7, 2, 0, 1, 2, 1};
    const size_t want_s[3] = {0, 7, 9}, want_r[3] = {0, 1, 3};
    for (int r = 0; r < 3; r++)
    {
        pf_exchange_offsets(hc, 3, r, &soff, &roff);
        CHECK(soff == want_s[r] && roff == want_r[r]);
    }
    CHECK(pf_exchange_plan_ok(hc, 3, 1, 4, &n_send, &n_recv) && n_send == 9 && n_recv == 4);
    CHECK(!pf_exchange_plan_ok(hc, 3, 1, 5, &n_send, &n_recv) && n_recv == 4); // received total != L
    CHECK(!pf_exchange_plan_ok(hc, 3, 0, 4, &n_send, &n_recv));                // self-send 7 != self-receive 1
    CHECK(!pf_exchange_plan_ok(hc, 3, 2, 4, &n_send, &n_recv));                // self-send 0 != self-receive 1
}

template <typename T>
static void check_strata()
{
    for (long long n : {1LL, 2LL, 3LL, 65LL, 1000LL})
    {
        std::vector<T> out((size_t)n + 1, (T)-1);
        const T        k = pf_fill_strata(out.data(), n, n);
        CHECK(k == (T)1 / (T)n);
        CHECK(out[0] == k / (T)2);
        bool chain = true;
        for (long long i = 1; i < n; i++)
        {
            const volatile T next = out[(size_t)i - 1] + k; // (rounded to T, as the table's entries are)
            chain = chain && out[(size_t)i] == next;
        }
        CHECK(chain);
        CHECK(out[(size_t)n] == (T)-1); // nothing behind the table
    }
    // no table: only k
    CHECK(pf_fill_strata<T>(nullptr, 0, 1LL << 31) == (T)1 / (T)(1LL << 31));
}

static void check_seed_args()
{
    long long ns = -1;
    const int np = 300;
    CHECK(pf_seed_args_ok(0, 300, np, &ns) && ns == 300);
    CHECK(!pf_seed_args_ok(-1, 300, np, &ns));
    CHECK(!pf_seed_args_ok(0, 1LL << 32, np, &ns));
    CHECK(pf_seed_args_ok(0, (1LL << 32) - 1, np, &ns) && ns == 0);
    CHECK(pf_seed_args_ok(0, 1LL << 31, np, &ns) && ns == 0); // above 2^31 - 1: normals only
    CHECK(pf_seed_args_ok(0, (1LL << 31) - 1, np, &ns) && ns == (1LL << 31) - 1);
    const long long ng = 1200;
    CHECK(!pf_seed_args_ok(ng - np + 1, ng, np, &ns));
    CHECK(pf_seed_args_ok(ng - np, ng, np, &ns) && ns == ng);
    CHECK(!pf_seed_args_ok(0, np - 1, np, &ns)); // a set smaller than the shard
}

int main()
{
    check_layout<float>();
    check_layout<double>();
    check_staged_memo<float>();
    check_staged_memo<double>();
    check_assoc_memo<float>();
    check_assoc_memo<double>();
    check_has_duplicate();
    check_exchange();
    check_strata<float>();
    check_strata<double>();
    check_seed_args();
    std::printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
