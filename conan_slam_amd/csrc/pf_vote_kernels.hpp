// pf_vote_kernels.hpp -- the vote on new features of the particle association, on the device: which observations of the
// last cslam_pf_associate become new features for EVERY particle (the feature index space is shared by all of them).
// It is pf.new_feature_votes (conan_slam_amd/pf.py) bit for bit, on the very doubles of the summary that
// pf_assoc_summary_kernel (pf_assoc_kernels.hpp) left in HBM -- or, for a sharded set, on their sum over the ranks.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace cslam
{

constexpr int kPfVoteLanes = 256; // one workgroup: 4 waves of 64

// summary[m][4] = (sum w matched, sum w new, sum w ambiguous, count matched).  Observation j is NEW when, in double and
// with total = (s0 + s1) + s2 in this order,  total > 0  &&  s1 > 0  &&  s1 >= new_fraction * total  (a NaN takes part
// in no comparison: never new).
//   use[j]      = new ? 0 : 1                                        j < m
//   new_idx[k]  = j, ZN[2k], ZN[2k+1] = Z[2j], Z[2j+1]               the new observations in observation order, k < q
//   count[0..1] = q, m
// Entries of new_idx / ZN from q on are NOT written.  One workgroup of kPfVoteLanes lanes walks the observations in tiles
// of kPfVoteLanes: inside a tile a lane's rank is the number of new lanes below it in its wave (ballot + population
// count) plus the totals of the waves below (LDS); a running base carries across tiles.  Plain stores, no atomics.
template <typename T>
__global__ void __launch_bounds__(kPfVoteLanes) pf_assoc_vote_kernel(const double* __restrict__ summary,
                                                                     const T* __restrict__ Z, int m, double new_fraction,
                                                                     int* __restrict__ use, int* __restrict__ new_idx,
                                                                     T* __restrict__ ZN, int* __restrict__ count)
{
    __shared__ int s_wave[kPfVoteLanes / 64];
    const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int            base = 0; // new observations of the tiles before this one (the same in every lane)
    for (int t0 = 0; t0 < m; t0 += kPfVoteLanes)
    {
        const int j   = t0 + (int)threadIdx.x;
        bool      isn = false;
        if (j < m)
        {
            const double s0 = summary[4 * j], s1 = summary[4 * j + 1], s2 = summary[4 * j + 2];
            const double total = (s0 + s1) + s2;
            isn                = (total > 0.0) && (s1 > 0.0) && (s1 >= new_fraction * total);
            use[j]             = isn ? 0 : 1;
        }
        const unsigned long long bal     = __ballot(isn);
        const int                in_wave = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0)
        {
            s_wave[wave] = __popcll(bal);
        }
        __syncthreads();
        int below = 0, tile = 0;
#pragma unroll
        for (int w = 0; w < kPfVoteLanes / 64; w++)
        {
            const int c = s_wave[w];
            below += (w < wave) ? c : 0;
            tile += c;
        }
        if (isn)
        {
            const int k   = base + below + in_wave; // k <= j < m
            new_idx[k]    = j;
            ZN[2 * k]     = Z[2 * j];
            ZN[2 * k + 1] = Z[2 * j + 1];
        }
        base += tile;
        __syncthreads(); // s_wave is rewritten by the next tile
    }
    if (threadIdx.x == 0)
    {
        count[0] = base;
        count[1] = m;
    }
}

} // namespace cslam
