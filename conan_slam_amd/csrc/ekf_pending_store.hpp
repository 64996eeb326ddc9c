// ekf_pending_store.hpp -- the bookkeeping of the pending W1 store of a single-filter handle.  Host only, plain integers.
// The store is two regions of wcap columns (the device buffers dW1 / dSign stay with Ekf<T>): region `wcur` collects the
// kp pending columns, the other one may still be read by a P-GEMM in flight on a second stream.  One method per event;
// the invariants they keep are listed in DESIGN.md 6 "Host engine layout".
#pragma once

namespace cslam
{
struct PendingCols
{
    int      wcap = 0;            // columns per region
    int      wcur = 0;            // the region that collects pending columns
    int      kp   = 0;            // pending columns (downdates not applied to P yet)
    int      hd_cols[2] = {0, 0}; // heading columns appended to each region since it became the pending store
    unsigned inflight_mask = 0;   // regions an unfinished P-GEMM on a second stream reads
    int      mirror_cols = 0, mirror_n = 0; // leading columns of region wcur the mirror holds, for a state of mirror_n rows

    // k columns written behind the pending ones (heading: rank-1 columns of heading observations, which carry a sign)
    void appended(int k, bool heading = false)
    {
        kp += k;
        hd_cols[wcur] += heading ? k : 0;
    }
    // the P-GEMM of the pending columns has been launched on a second stream (before applied())
    void pgemm_on_second_stream() { inflight_mask |= 1u << wcur; }
    // the P-GEMM of every pending column has been launched: the other region becomes the pending store.  Returns whether
    // that region's column signs have to be cleared (they belong to heading columns applied a flush ago).
    bool applied()
    {
        wcur ^= 1;
        kp = mirror_cols = 0; // (the mirror described the columns that have just been applied)
        const bool clear_signs = hd_cols[wcur] > 0;
        hd_cols[wcur]          = 0;
        return clear_signs;
    }
    // a new state discards updates that were never applied (every stream has been waited for)
    void discarded() { wcur = kp = mirror_cols = hd_cols[0] = hd_cols[1] = inflight_mask = 0; }
    // the store has moved to new buffers of `cols` columns per region (applied and every stream waited for before)
    void regrown(int cols)
    {
        discarded();
        wcap = cols;
    }
    void mirror_written(int cols, int n)
    {
        mirror_cols = cols;
        mirror_n    = n;
    }
    void mirror_void() { mirror_cols = 0; }
    bool mirror_covers(int cols, int n) const { return mirror_cols > 0 && mirror_cols == cols && mirror_n == n; }
    void waited() { inflight_mask = 0; } // stream A has waited for every P-GEMM launched so far
    bool in_flight() const { return inflight_mask != 0; }
    bool in_flight(int region) const { return (inflight_mask & (1u << region)) != 0; } // wait before stream A writes there
};
} // namespace cslam
