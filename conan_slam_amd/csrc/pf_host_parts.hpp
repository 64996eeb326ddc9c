// pf_host_parts.hpp -- the arithmetic and bookkeeping of the particle handle that needs no GPU: the layout of the device
// staging area, the memo of what it holds, the validity of the association tables and of the vote on new features, and
// the small host loops of the fused step, the sharded exchange and the strata table, the chunk split and the refusal
// rule of the control run, the refusal rules of the FastSLAM-1 step, and the book of the device-side score.  No HIP include:
// tests/host/pf_host_parts_check.cpp, pf_control_check.cpp, pf_fs1_check.cpp and pf_score_book_check.cpp build it with
// plain g++ (and under the address and undefined-behaviour sanitizers).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

namespace cslam
{

// The device staging area of one handle: Z (2*mcap T) | idf (mcap int) | normals (3*np T) | select (np T).
template <typename T>
struct PfObsLayout
{
    int mcap = 0; // observations the area has room for
    int np   = 0;

    size_t off_idf() const { return (size_t)2 * mcap * sizeof(T); }
    size_t off_normals() const { return off_idf() + (size_t)mcap * sizeof(int); }
    size_t off_select() const { return off_normals() + (size_t)3 * np * sizeof(T); }

    // capacity after growing to m observations: a multiple of 4 keeps the normals 16-byte aligned
    static int grown(int m, int mcap) { return (std::max(m, std::max(64, 2 * mcap)) + 3) / 4 * 4; }
    // elements of T behind the area (newm is a multiple of 4: its ints are a whole number of T)
    static size_t alloc_count(int newm, int np) { return (size_t)2 * newm + (size_t)4 * np + (size_t)newm * sizeof(int) / sizeof(T); }

    // bytes of the one copy that brings ...
    size_t bytes_z(int m) const { return (size_t)2 * m * sizeof(T); }                  // Z
    size_t bytes_z_idf(int m) const { return off_idf() + (size_t)m * sizeof(int); }    // Z | idf
    size_t bytes_z_idf_normals() const { return off_select(); }                        // Z | idf | normals
    size_t bytes_step() const { return off_select() + (size_t)np * sizeof(T); }        // Z | idf | normals | select
};

// Which Z || idf bytes the staging area holds (nothing remembered = unknown).  A call whose Z / idf are byte-identical
// to them (featureUpdate right after sampleProposal, PF.cpp:150-156) sends nothing.
class PfStagedMemo
{
  public:
    void clear() { bytes_.clear(); }
    void remember(const void* Z, size_t zb, const int* idf, size_t ib)
    {
        bytes_.resize(zb + ib);
        if (zb)
        {
            std::memcpy(bytes_.data(), Z, zb);
        }
        if (ib)
        {
            std::memcpy(bytes_.data() + zb, idf, ib);
        }
    }
    bool holds(const void* Z, size_t zb, const int* idf, size_t ib) const
    {
        return !bytes_.empty() && bytes_.size() == zb + ib && std::memcmp(bytes_.data(), Z, zb) == 0 &&
               (ib == 0 || std::memcmp(bytes_.data() + zb, idf, ib) == 0);
    }

  private:
    std::vector<char> bytes_;
};

// why a consumer of the association tables may not read them now
enum class PfAssocRefusal
{
    none,
    never_associated,
    moved,      // particles changed slots since (the table is per slot)
    other_scan, // Z / m are not those of the last associate
    map_shrank,
    bad_use // use[*index] is neither 0 nor 1
};

// What the association tables describe: the observations of the LAST associate call (kept to recognise them again), the
// map size of that moment, and whether the particles still sit in the slots they had then.
template <typename T>
class PfAssocMemo
{
  public:
    int m() const { return assoc_m; }   // -1: associate has not been called (or its tables are gone)
    int nf() const { return assoc_nf; }
    void forget() { assoc_m = -1; }
    void moved() { assoc_moved = true; } // resample, unpack, set_particle
    void associated(const void* Z, int m, int nf)
    {
        assoc_m     = m;
        assoc_nf    = nf;
        assoc_moved = false;
        assoc_Z.clear();
        if (m > 0)
        {
            assoc_Z.assign(static_cast<const char*>(Z), static_cast<const char*>(Z) + (size_t)2 * m * sizeof(T));
        }
    }
    // the consumers take the observations of the last associate: anything else would pair a table with the wrong scan
    PfAssocRefusal check(const void* Z, int m, int nf, const int* use, int* index) const
    {
        const PfAssocRefusal scan = check_scan(Z, m, nf);
        if (scan != PfAssocRefusal::none)
        {
            return scan;
        }
        for (int i = 0; i < m; i++)
        {
            if (use[i] != 0 && use[i] != 1)
            {
                *index = i;
                return PfAssocRefusal::bad_use;
            }
        }
        return PfAssocRefusal::none;
    }
    // the same without a host mask (the _voted consumers read theirs from the device)
    PfAssocRefusal check_scan(const void* Z, int m, int nf) const
    {
        if (assoc_m < 0)
        {
            return PfAssocRefusal::never_associated;
        }
        if (assoc_moved)
        {
            return PfAssocRefusal::moved;
        }
        if (m != assoc_m || (m > 0 && std::memcmp(assoc_Z.data(), Z, (size_t)2 * m * sizeof(T)) != 0))
        {
            return PfAssocRefusal::other_scan;
        }
        if (nf < assoc_nf)
        {
            return PfAssocRefusal::map_shrank;
        }
        return PfAssocRefusal::none;
    }

  private:
    int               assoc_m     = -1;
    int               assoc_nf    = 0;
    bool              assoc_moved = false;
    std::vector<char> assoc_Z; // the 2 * assoc_m observation scalars
};

// why a call that needs the vote on new features (cslam_pf_associate_vote) may not have it now
enum class PfVoteRefusal
{
    none,
    no_vote,      // no cslam_pf_associate_vote yet, or a later cslam_pf_associate dropped it
    already_added // cslam_pf_add_features_voted has added this vote's features
};

// What the vote buffers describe.  A vote belongs to the LAST associate: a later plain associate drops it, a later
// associate_vote replaces it.  Its features are added at most once.  The _voted consumers read use[] next to the
// association table, so they need what PfAssocMemo::check_scan needs as well (same Z and m, particles not moved, map not
// shrunk); adding the voted features needs none of that: ZN is per observation, not per particle slot.  q becomes known
// to the host when somebody has waited for the vote's event.
class PfVoteMemo
{
  public:
    bool live() const { return live_; }
    int  m() const { return m_; }
    bool waited() const { return waited_; } // (of a live vote)
    int  q() const { return q_; }           // (of a live vote somebody has waited for)
    bool added() const { return added_; }

    void forget() { live_ = false; } // a later associate, or the buffers are gone
    void voted(int m)                // the vote of m observations has been queued behind its associate
    {
        live_   = true;
        m_      = m;
        waited_ = false;
        q_      = 0;
        added_  = false;
    }
    void arrived(int q) // somebody waited for the event: q is on the host
    {
        waited_ = true;
        q_      = q;
    }
    void features_added() { added_ = true; }

    // the consumers (together with PfAssocMemo::check_scan), cslam_pf_vote_wait and cslam_pf_get_vote
    PfVoteRefusal check_read() const { return live_ ? PfVoteRefusal::none : PfVoteRefusal::no_vote; }
    // cslam_pf_add_features_voted (a refusal -- this one or a capacity overflow -- leaves the vote as it was)
    PfVoteRefusal check_add() const
    {
        if (!live_)
        {
            return PfVoteRefusal::no_vote;
        }
        return added_ ? PfVoteRefusal::already_added : PfVoteRefusal::none;
    }

  private:
    bool live_   = false;
    bool waited_ = false;
    bool added_  = false;
    int  m_      = 0;
    int  q_      = 0;
};

// does an observation list name a feature twice?
inline bool pf_has_duplicate(const int* idf, int m)
{
    for (int a = 0; a < m; a++)
    {
        for (int c = a + 1; c < m; c++)
        {
            if (idf[a] == idf[c])
            {
                return true;
            }
        }
    }
    return false;
}

// why a call of the new-feature scan (cslam_pf_sample_pose, cslam_pf_new_feature_step and their _drawn forms) is refused
enum class PfNewFeatureRefusal
{
    none,
    bad_arg, // q < 0, no normals, or q > 0 without Z or R
    capacity // nf + q > max_features
};

// The arguments of the new-feature scan: q new observations (Z 2 x q, R 2 x 2) on a store of nf features with room for
// nfcap.  With q = 0 neither Z nor R is read.  A refused call changes nothing.
inline PfNewFeatureRefusal pf_new_feature_check(int q, bool has_Z, bool has_R, bool has_normals, int nf, int nfcap)
{
    if (q < 0 || !has_normals || (q > 0 && (!has_Z || !has_R)))
    {
        return PfNewFeatureRefusal::bad_arg;
    }
    if (q > nfcap - nf)
    {
        return PfNewFeatureRefusal::capacity;
    }
    return PfNewFeatureRefusal::none;
}

// A run of k control steps (test/main.cpp:279-286) goes out kPfControlChunk steps per launch, the chunks back to back.
constexpr int kPfControlChunk = 16; // = kPfControlMax of pf_control_kernels.hpp

// launches of a run of k steps (k <= 0: none)
inline int pf_control_chunks(int k) { return k > 0 ? (k - 1) / kPfControlChunk + 1 : 0; }
// chunk c of a run of k steps covers steps *first .. *first + *count - 1; false when the run has no chunk c
inline bool pf_control_chunk(int k, int c, int* first, int* count)
{
    if (c < 0 || c >= pf_control_chunks(k))
    {
        *first = *count = 0;
        return false;
    }
    *first = c * kPfControlChunk;
    *count = std::min(kPfControlChunk, k - *first);
    return true;
}

// why a control run (cslam_pf_control_run, and the run in front of cslam_pf_cycle_drawn / _assoc_cycle_drawn) is refused
enum class PfControlRefusal
{
    none,
    bad_k,       // k < 0
    null_control, // k > 0 without v, swa or Q
    null_phi     // k > 0 and the heading observed, without phi
};

// The arguments of a control run of k steps.  With k = 0 nothing is read, so nothing needs to be there; phi is read only
// when the heading is observed.  A refused run changes nothing.
inline PfControlRefusal pf_control_check(int k, bool has_v, bool has_swa, bool has_Q, bool has_phi, bool use_heading)
{
    if (k < 0)
    {
        return PfControlRefusal::bad_k;
    }
    if (k > 0 && (!has_v || !has_swa || !has_Q))
    {
        return PfControlRefusal::null_control;
    }
    if (k > 0 && use_heading && !has_phi)
    {
        return PfControlRefusal::null_phi;
    }
    return PfControlRefusal::none;
}

// why a call of the FastSLAM-1 step (cslam_pf_control_run_sampled, cslam_pf_get_control_draws, cslam_pf_likelihood_update,
// cslam_pf_fs1_cycle_drawn) is refused; every refusal comes before the first launch and changes nothing
enum class PfFs1Refusal
{
    none,
    bad_k,        // k < 0
    null_control, // k > 0 without v, swa or Q
    null_phi,     // k > 0 and the heading observed, without phi
    bad_step,     // ctl_step < 0
    bad_q,        // Q[0,0] or Q[1,1] negative (or NaN): the control noise has no standard deviation
    bad_scan,     // a negative count, or observations without Z, idf or R
    bad_idf,      // idf[*index] outside 1..nf
    capacity      // nf + mn > max_features
};

// The arguments of a sampled control run of k steps from control step ctl_step.  q_diag: {Q[0,0], Q[1,1]} as doubles, or
// nullptr where Q is absent; with k = 0 nothing is read and only k and ctl_step are looked at.
inline PfFs1Refusal pf_fs1_control_check(int k, bool has_v, bool has_swa, const double* q_diag, bool has_phi, bool use_heading,
                                         long long ctl_step)
{
    switch (pf_control_check(k, has_v, has_swa, q_diag != nullptr, has_phi, use_heading))
    {
    case PfControlRefusal::none:
        break;
    case PfControlRefusal::bad_k:
        return PfFs1Refusal::bad_k;
    case PfControlRefusal::null_control:
        return PfFs1Refusal::null_control;
    case PfControlRefusal::null_phi:
        return PfFs1Refusal::null_phi;
    }
    if (ctl_step < 0)
    {
        return PfFs1Refusal::bad_step;
    }
    if (k > 0 && (!(q_diag[0] >= 0.0) || !(q_diag[1] >= 0.0)))
    {
        return PfFs1Refusal::bad_q;
    }
    return PfFs1Refusal::none;
}

// cslam_pf_get_control_draws: k steps from ctl_step into `normals`
inline PfFs1Refusal pf_fs1_draws_check(int k, long long ctl_step, bool has_out)
{
    if (k < 0)
    {
        return PfFs1Refusal::bad_k;
    }
    if (ctl_step < 0)
    {
        return PfFs1Refusal::bad_step;
    }
    return (k > 0 && !has_out) ? PfFs1Refusal::null_control : PfFs1Refusal::none;
}

// The scan of the FastSLAM-1 step: mf observations of known features (Z, idf, 1-based, on a store of nf features) and mn
// of new ones (room for nfcap features), R for either.  cslam_pf_likelihood_update is the case mn = 0.
inline PfFs1Refusal pf_fs1_scan_check(int mf, bool has_ZF, const int* idf, int mn, bool has_ZN, bool has_R, int nf, int nfcap,
                                      int* index)
{
    *index = -1;
    if (mf < 0 || mn < 0 || (mf > 0 && (!has_ZF || idf == nullptr)) || (mn > 0 && !has_ZN) || ((mf > 0 || mn > 0) && !has_R))
    {
        return PfFs1Refusal::bad_scan;
    }
    for (int i = 0; i < mf; i++)
    {
        if (idf[i] < 1 || idf[i] > nf)
        {
            *index = i;
            return PfFs1Refusal::bad_idf;
        }
    }
    if (mn > nfcap - nf)
    {
        return PfFs1Refusal::capacity;
    }
    return PfFs1Refusal::none;
}

// the control step chunk c of a sampled run starts at: the chunks are those of pf_control_chunk
inline long long pf_fs1_chunk_step(long long ctl_step, int c) { return ctl_step + (long long)kPfControlChunk * c; }

// The record counts of a sharded exchange: hc[r] records go to rank r, hc[world + r] come from it; both buffers hold
// them grouped by rank.  Where the records for / from `rank` start:
inline void pf_exchange_offsets(const int* hc, int world, int rank, size_t* soff, size_t* roff)
{
    *soff = *roff = 0;
    for (int r = 0; r < rank; r++)
    {
        *soff += (size_t)hc[r];
        *roff += (size_t)hc[world + r];
    }
}

// the plan fills the L slots of this rank, and what it sends itself is what it receives from itself
inline bool pf_exchange_plan_ok(const int* hc, int world, int rank, int L, int* n_send, int* n_recv)
{
    *n_send = *n_recv = 0;
    for (int r = 0; r < world; r++)
    {
        *n_send += hc[r];
        *n_recv += hc[world + r];
    }
    return *n_recv == L && hc[rank] == hc[world + rank];
}

// k/2, +k, +k, ...: the running sum of stratified_random (PF.cpp:579-596, as pf.py rounds it), in T and in index order;
// returns k = 1 / n_global in T
template <typename T>
inline T pf_fill_strata(T* out, long long n_strata, long long n_global)
{
    const T k   = (T)1 / (T)n_global;
    T       acc = k / (T)2;
    for (long long i = 0; i < n_strata; i++)
    {
        out[i] = acc;
        acc    = acc + k;
    }
    return k;
}

// The arguments of seed_draws: 0 <= first_global, first_global + np <= n_global < 2^32.  One launch draws at most
// 2^31 - 1 strata (and every resample form counts its particles in an int): a larger set gets its normals -- the keys
// reach slot 2^32 - 1 -- and no strata table (*n_strata = 0).
inline bool pf_seed_args_ok(long long first_global, long long n_global, int np, long long* n_strata)
{
    *n_strata = (n_global <= 0x7fffffffLL) ? n_global : 0;
    return !(first_global < 0 || n_global >= (1LL << 32) || first_global > n_global - np);
}

// The bookkeeping of the score kept on the device (cslam_pf_score*): which estimate is scored, the gates, how many
// records the series and the track hold, how many truth rows there are, and the calls since the last reset.  The
// default state is that of reset(0, 0, 0, 0): a score call without a prior reset behaves as after it.
class PfScoreBook
{
  public:
    static constexpr double kGatePose = 7.8147; // the 95 % chi-square points of 3 and 2 degrees of freedom
    static constexpr double kGateLm   = 5.9915;
    static constexpr int    kLanes    = 256; // features per workgroup of the landmark kernel

    static bool reset_args_ok(int estimator, int series_capacity)
    {
        return (estimator == 0 || estimator == 1) && series_capacity >= 0;
    }
    // (the arguments have passed reset_args_ok; a gate <= 0, or NaN, selects its default).  The truth rows are kept.
    void reset(int estimator, int series_capacity, double gate_pose, double gate_lm)
    {
        estimator_ = estimator;
        capacity_  = series_capacity;
        gate_pose_ = gate_pose > 0.0 ? gate_pose : kGatePose;
        gate_lm_   = gate_lm > 0.0 ? gate_lm : kGateLm;
        calls_     = 0;
    }
    static bool truth_args_ok(int count, int max_features) { return count >= 0 && count <= max_features; }
    void        set_truth_count(int count) { truth_ = count; }

    int       estimator() const { return estimator_; }
    int       capacity() const { return capacity_; }
    int       truth_count() const { return truth_; }
    double    gate_pose() const { return gate_pose_; }
    double    gate_lm() const { return gate_lm_; }
    long long calls() const { return calls_; }

    // features one call scores: min(nf, truth rows) with the map, none without
    int scored(int nf, int with_map) const { return with_map ? std::min(nf, truth_) : 0; }
    // workgroups (= scratch slots) of the landmark kernel for c features
    static int blocks(int c) { return (c + kLanes - 1) / kLanes; }
    // the record the NEXT call writes, or -1 when the series is full or absent
    long long next_record() const { return calls_ < (long long)capacity_ ? calls_ : -1; }
    void      called() { calls_++; }
    // records held, and how many of them a read into room for capacity_records copies
    int records() const { return (int)std::min(calls_, (long long)capacity_); }
    int records_to_copy(int capacity_records) const { return std::max(0, std::min(records(), capacity_records)); }
    // does a series allocated for `have` records serve a reset to series_capacity?  (it only ever grows)
    static bool series_fits(size_t have, int series_capacity) { return (size_t)series_capacity <= have; }

  private:
    int       estimator_ = 0;
    int       capacity_  = 0;
    int       truth_     = 0;
    double    gate_pose_ = kGatePose;
    double    gate_lm_   = kGateLm;
    long long calls_     = 0;
};

} // namespace cslam
