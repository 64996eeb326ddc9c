// pf_buffers.hpp -- the buffer groups of the particle handle (host code).  A group grows all-or-nothing
// (device_owners.hpp): the complete new set is allocated into a local group, the first failure returns with the handle
// untouched, and ONE move-assignment replaces the old set -- after the stream has been waited for, where queued work
// may still use the old one.
#pragma once

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "device_owners.hpp"
#include "pf_estimate_kernels.hpp"
#include "pf_staging.hpp"

namespace cslam
{

// one set of per-particle arrays (structure of arrays, np columns); the handle holds the store and its twin
template <typename T>
struct PfArrays
{
    DevBuf<T> xv, pv, xf, pf;

    // PF.cpp:319-341: X = 0, P = 0, empty map
    int alloc_zeroed(size_t np, size_t nfcap, hipStream_t stream)
    {
        CSLAM_TRY(xv.alloc_zeroed(3 * np, stream));
        CSLAM_TRY(pv.alloc_zeroed(9 * np, stream));
        CSLAM_TRY(xf.alloc_zeroed(2 * nfcap * np, stream));
        return pf.alloc_zeroed(4 * nfcap * np, stream);
    }
};

// the single-shard resample: strata, plan and the {Neff, flag, calls, resamples} block with its pinned mirror
template <typename T>
struct PfResampleBufs
{
    DevBuf<T>         sel, cum;
    DevBuf<int>       keep, enable;
    DevBuf<double>    info;
    PinnedBuf<double> hInfo;

    int ensure(int np, hipStream_t stream)
    {
        if (sel)
        {
            return CSLAM_OK;
        }
        PfResampleBufs b;
        CSLAM_TRY(b.sel.alloc((size_t)np));
        CSLAM_TRY(b.cum.alloc((size_t)np));
        CSLAM_TRY(b.keep.alloc((size_t)np));
        CSLAM_TRY(b.enable.alloc(1));
        CSLAM_TRY(b.info.alloc_zeroed(4, stream));
        CSLAM_TRY(b.hInfo.alloc(4));
        *this = std::move(b);
        return CSLAM_OK;
    }
};

// The sharded resample: everything that can fail is allocated BEFORE the first collective, so that a rank never leaves
// its peers waiting inside one because a local allocation failed.  Two levels: the plan (sized by world) and the record
// buffers (sized by world and by the map).
template <typename T>
struct PfShardedBufs
{
    struct Plan
    {
        DevBuf<double>    sumsG;
        DevBuf<T>         wall, selG;
        DevBuf<T>         cumG; // running sum of the gathered weights (pf_keep_kernel)
        DevBuf<int>       keepG, sendIdx, counts;
        PinnedBuf<double> hCounts; // the two global sums first, later the record counts (ints from double 4 on)
    };
    struct Records
    {
        DevBuf<T> send, recv;
    };
    Plan             plan;
    Records          rec;
    int              world = 0;
    int              nf    = -1;
    std::vector<int> last_counts; // 2 * world record counts of the last exchange (send per destination, receive per source)
    int              last_n_send = 0;

    double* h_sums() const { return plan.hCounts.get(); }
    int*    h_counts() const { return reinterpret_cast<int*>(plan.hCounts.get()) + 8; }

    int ensure(int new_world, int new_nf, int np, hipStream_t stream)
    {
        const size_t N = (size_t)np * new_world;
        if (world != new_world)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            Plan p;
            CSLAM_TRY(p.sumsG.alloc(2));
            CSLAM_TRY(p.wall.alloc(N));
            CSLAM_TRY(p.selG.alloc(N));
            CSLAM_TRY(p.cumG.alloc(N));
            CSLAM_TRY(p.keepG.alloc(N));
            CSLAM_TRY(p.sendIdx.alloc(N));
            CSLAM_TRY(p.counts.alloc((size_t)2 * new_world));
            CSLAM_TRY(p.hCounts.alloc((size_t)2 * new_world + 4));
            plan  = std::move(p);
            world = new_world;
            nf    = -1; // (the record buffers below are sized by N as well)
        }
        if (nf != new_nf)
        {
            const size_t len = (size_t)(13 + 6 * new_nf);
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            Records r;
            CSLAM_TRY(r.send.alloc(N * len)); // worst case: every slot keeps a particle of this rank
            CSLAM_TRY(r.recv.alloc((size_t)np * len));
            rec = std::move(r);
            nf  = new_nf;
        }
        return CSLAM_OK;
    }
};

// The read path brings ONE block back through hEst (pinned): kEstOutHdr doubles, then the T record [w, Xv, Pv, XF, PF].
template <typename T>
struct PfEstimateBufs
{
    DevBuf<double>  part;            // per-chunk partials of passes 1 and 2
    DevBuf<double>  out, local;      // output block
    DevBuf<double>  sum, sumAll;     // this rank's summary / every rank's (sharded estimate)
    DevBuf<double>  bestHdrAll;      // every rank's pick (sharded best particle)
    DevBuf<T>       bestRecAll, feat; // every rank's picked record; the transposed features
    PinnedBuf<char> hEst;

    template <typename B>
    static int grow(B& buf, size_t count, hipStream_t stream)
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
    static T* rec(double* block) { return reinterpret_cast<T*>(block + kEstOutHdr); }
    const double* h_hdr() const { return reinterpret_cast<const double*>(hEst.get()); }

    // header + the first rec_len scalars of the record of `block` -> hEst, one copy, synchronised
    int fetch(const double* block, size_t rec_len, hipStream_t stream)
    {
        const size_t bytes = (size_t)kEstOutHdr * sizeof(double) + rec_len * sizeof(T);
        CSLAM_HIP_TRY(hipMemcpyAsync(hEst.get(), block, bytes, hipMemcpyDeviceToHost, stream));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        return CSLAM_OK;
    }
    // the fetched record into the caller's arrays (the map only when `map`)
    void scatter(bool map, int nf, void* w, void* Xv, void* Pv, void* XF, void* PF) const
    {
        const T* r   = reinterpret_cast<const T*>(hEst.get() + (size_t)kEstOutHdr * sizeof(double));
        auto     put = [](void* dst, const T* src, size_t n) {
            if (dst)
            {
                std::memcpy(dst, src, n * sizeof(T));
            }
        };
        put(w, r, 1);
        put(Xv, r + 1, 3);
        put(Pv, r + 4, 9);
        put(map ? XF : nullptr, r + 13, (size_t)2 * nf);
        put(map ? PF : nullptr, r + 13 + 2 * nf, (size_t)4 * nf);
    }
};

// The score kept on the device (pf_score_kernels.hpp) and its book.  Two levels, each all-or-nothing: the base (totals,
// the landmark kernel's scratch and the truth rows, sized for max_features once) and the log (series and track, sized by
// the largest series_capacity a reset has asked for).  A handle that never calls a score function allocates neither.
struct PfScoreBufs
{
    struct Base
    {
        DevBuf<double> totals; // [fields]
        DevBuf<double> parts;  // [blocks(max_features)][5]
        DevBuf<double> truth;  // [max_features][2]
    };
    struct Log
    {
        DevBuf<float>  series; // [capacity][4]
        DevBuf<double> track;  // [capacity][5]
    };
    Base        base;
    Log         log;
    PfScoreBook book;

    bool allocated() const { return (bool)base.totals; }

    // the base, with zeroed totals (a handle that has never been reset scores from zero)
    int ensure_base(int fields, int nfcap, hipStream_t stream)
    {
        if (allocated())
        {
            return CSLAM_OK;
        }
        const size_t cf = (size_t)std::max(nfcap, 1);
        Base         b;
        CSLAM_TRY(b.totals.alloc_zeroed((size_t)fields, stream));
        CSLAM_TRY(b.parts.alloc((size_t)PfScoreBook::blocks((int)cf) * 5));
        CSLAM_TRY(b.truth.alloc(2 * cf));
        base = std::move(b);
        return CSLAM_OK;
    }
    // room for series_capacity records (the old log is released after the stream has been waited for)
    int ensure_log(int series_capacity, hipStream_t stream)
    {
        if (PfScoreBook::series_fits(log.series.count() / 4, series_capacity))
        {
            return CSLAM_OK;
        }
        Log l;
        CSLAM_TRY(l.series.alloc((size_t)series_capacity * 4));
        CSLAM_TRY(l.track.alloc((size_t)series_capacity * 5));
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still writes the old log
        log = std::move(l);
        return CSLAM_OK;
    }
};

// The tables of the per-particle association and what they describe (PfAssocMemo: growing the tables forgets it).
template <typename T>
struct PfAssocTables
{
    struct Partials // [chunk][observation][particle]
    {
        DevBuf<T>   nd, nis;
        DevBuf<int> j;
    };
    struct Tables // [observation][particle]; summary: 4 doubles per observation
    {
        DevBuf<T>      rawNd;
        DevBuf<int>    rawIdf, rawKind, idf, kind;
        DevBuf<double> summary;
    };
    Partials       part;
    Tables         tab;
    PfAssocMemo<T> memo;

    int ensure(int m, int nchunks, int np, hipStream_t stream)
    {
        const size_t need_part = (size_t)std::max(nchunks, 1) * m * np;
        if (need_part > part_cap_)
        {
            CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still reads the old partials
            Partials p;
            CSLAM_TRY(p.nd.alloc(need_part));
            CSLAM_TRY(p.nis.alloc(need_part));
            CSLAM_TRY(p.j.alloc(need_part));
            part      = std::move(p);
            part_cap_ = need_part;
        }
        if (m > mcap_)
        {
            const int    newm = std::max(m, std::max(64, 2 * mcap_));
            const size_t cnt  = (size_t)newm * np;
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
            Tables t;
            CSLAM_TRY(t.rawNd.alloc(cnt));
            CSLAM_TRY(t.rawIdf.alloc(cnt));
            CSLAM_TRY(t.rawKind.alloc(cnt));
            CSLAM_TRY(t.idf.alloc(cnt));
            CSLAM_TRY(t.kind.alloc(cnt));
            CSLAM_TRY(t.summary.alloc((size_t)newm * 4));
            tab   = std::move(t);
            mcap_ = newm;
            memo.forget(); // the old tables are gone
        }
        return CSLAM_OK;
    }

  private:
    size_t part_cap_ = 0; // entries of the three partial tables
    int    mcap_     = 0; // observations the (m x np) tables and the summary hold
};

// The vote on new features (pf_vote_kernels.hpp) and what it describes (PfVoteMemo).  count and use share one block,
// [q, m, use[mcap]], so that ONE device-to-host copy brings the count and the mask to the pinned mirror; new_idx and ZN
// hold the compacted new observations; summary_all is the sum over the ranks of the shards' summaries and is allocated
// for the sharded vote only.  The event is recorded behind that copy: waiting for it waits for the vote, not for what
// has been queued since.
template <typename T>
struct PfVote
{
    struct Bufs
    {
        DevBuf<int>    count;   // [2 + mcap]: q, m, use[mcap]
        DevBuf<int>    new_idx; // [mcap]
        DevBuf<T>      ZN;      // [2 * mcap]
        PinnedBuf<int> host;    // [2 + mcap], the mirror of count
    };
    Bufs           b;
    DevBuf<double> summary_all; // [4 * mcap], sharded form
    Event          ev;
    PfVoteMemo     memo;

    int* count() const { return b.count.get(); }
    int* use() const { return b.count.get() + 2; }
    const int* h_count() const { return b.host.get(); }
    const int* h_use() const { return b.host.get() + 2; }
    static size_t copy_ints(int m) { return (size_t)2 + (size_t)m; }

    int ensure(int m, bool sharded, hipStream_t stream)
    {
        if (!ev)
        {
            CSLAM_TRY(ev.create(hipEventDisableTiming));
        }
        if (m > mcap_ || !b.count)
        {
            const int newm = std::max(m, std::max(64, 2 * mcap_));
            Bufs      n;
            CSLAM_TRY(n.count.alloc((size_t)2 + newm));
            CSLAM_TRY(n.new_idx.alloc((size_t)newm));
            CSLAM_TRY(n.ZN.alloc((size_t)2 * newm));
            CSLAM_TRY(n.host.alloc((size_t)2 + newm));
            DevBuf<double> s;
            if (sharded || summary_all)
            {
                CSLAM_TRY(s.alloc((size_t)4 * newm));
            }
            CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still uses the old set
            b           = std::move(n);
            summary_all = std::move(s);
            mcap_       = newm;
            memo.forget(); // the old vote is gone
        }
        if (sharded && !summary_all)
        {
            DevBuf<double> s;
            CSLAM_TRY(s.alloc((size_t)4 * mcap_));
            summary_all = std::move(s);
        }
        return CSLAM_OK;
    }

  private:
    int mcap_ = 0; // observations the set holds
};

// The seed of the device-side draws and the strata table of the resample (pf_draw_kernels.hpp).
template <typename T>
struct PfDraws
{
    bool               seeded  = false;
    unsigned long long seed    = 0;
    long long          first   = 0; // global slot of this handle's particle 0
    long long          nglobal = 0; // particles of the whole set = strata of the resample
    T                  k       = (T)0; // 1 / n_global in T (stratified_random's k)
    DevBuf<T>          di;  // [n_strata] k/2, +k, +k, ... (pf_fill_strata)
    DevBuf<T>          out; // [3 np + n_strata] what cslam_pf_get_draws brings back (never the staging area)

    // (the arguments have passed pf_seed_args_ok, which gave n_strata)
    int reseed(long long new_seed, long long first_global, long long n_global, long long n_strata, int np, hipStream_t stream)
    {
        PfDraws        d;
        std::vector<T> h;
        try
        {
            h.resize((size_t)n_strata);
        }
        catch (const std::bad_alloc&)
        {
            return fail(CSLAM_ERR_ALLOC, "pf_seed_draws: out of host memory for %lld strata", n_global);
        }
        CSLAM_TRY(d.di.alloc((size_t)std::max(n_strata, 1LL)));
        CSLAM_TRY(d.out.alloc((size_t)3 * np + (size_t)n_strata));
        d.k = pf_fill_strata(h.data(), n_strata, n_global);
        CSLAM_HIP_TRY(hipStreamSynchronize(stream)); // nothing queued still reads the old table
        if (n_strata > 0)
        {
            CSLAM_HIP_TRY(hipMemcpyAsync(d.di.get(), h.data(), (size_t)n_strata * sizeof(T), hipMemcpyHostToDevice, stream));
            CSLAM_HIP_TRY(hipStreamSynchronize(stream));
        }
        d.seeded  = true;
        d.seed    = (unsigned long long)new_seed;
        d.first   = first_global;
        d.nglobal = n_global;
        *this     = std::move(d);
        return CSLAM_OK;
    }
};

} // namespace cslam
