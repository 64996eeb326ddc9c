// sim_kernels.hpp -- device bodies of the observation generator, shared by the single-scan handle (cslam_sim.hip) and the
// batched Monte-Carlo generator (cslam_sim_batch.hip): both run the same arithmetic and the same ordered compaction.
//
// One workgroup of kSimThreads threads walks the landmarks / the scan in order and compacts with a block-wide exclusive
// scan, so that the outputs come out in ascending tag order exactly as the reference's sequential loops produce them.
#pragma once

#include <hip/hip_runtime.h>

#include "device_math.hpp"

namespace cslam
{

constexpr int kSimThreads = 1024;

// exclusive prefix sum of one flag per thread over the workgroup; returns the thread's offset, *total = block sum
__device__ inline int block_exclusive_scan(int flag, int* s_wave, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag != 0);
    const int                in_wave = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0)
    {
        s_wave[wave] = __popcll(bal);
    }
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < kSimThreads / 64; w++)
    {
        const int c = s_wave[w];
        base += (w < wave) ? c : 0;
        sum += c;
    }
    __syncthreads();
    *total = sum;
    return base + in_wave;
}

// slam.h:575-683 getVisibleLandmarks + slam.h:339-368 computeRangeBearing.  The visibility test is evaluated in
// double on the float differences, as the reference does (slam.h:627-628 stores float subtractions in doubles).
// Returns the number of visible landmarks (the same value in every thread); only the first `cap` are written.
template <typename T>
__device__ inline int sim_get_observations_body(const T* __restrict__ LM, int nlm, T x, T y, T phi, T rmax,
                                                T* __restrict__ Z, int* __restrict__ tags, int cap, int* s_wave)
{
    const double cphi = cos((double)phi), sphi = sin((double)phi), rm = (double)rmax;
    int          done = 0;
    for (int base = 0; base < nlm; base += kSimThreads)
    {
        const int i   = base + threadIdx.x;
        bool      vis = false;
        T         fx = (T)0, fy = (T)0;
        if (i < nlm)
        {
            fx = LM[2 * i] - x;
            fy = LM[2 * i + 1] - y;
            const double dx = (double)fx, dy = (double)fy;
            vis = (fabs(dx) < rm && fabs(dy) < rm) && ((dx * cphi + dy * sphi) > 0.0) && ((dx * dx + dy * dy) < rm * rm);
        }
        int       total;
        const int off = block_exclusive_scan(vis ? 1 : 0, s_wave, &total);
        if (vis && done + off < cap)
        {
            const int o  = done + off;
            Z[2 * o]     = dsqrt(fx * fx + fy * fy);
            Z[2 * o + 1] = datan2(fy, fx) - phi;
            tags[o]      = i + 1;
        }
        done += total;
    }
    return done;
}

// EKF.cpp:146-233.  The scan of m observations is split by the table as it stands before this scan (EKF.cpp:169-182);
// then the new tags receive the state positions nf+1, nf+2, ... in scan order (EKF.cpp:213-226).  route (may be NULL):
// where scan position i went -- o >= 0: column o of ZF, ~o < 0: column o of ZN.
template <typename T>
__device__ inline void sim_associate_table_body(const T* __restrict__ Z, const int* __restrict__ tags, int m,
                                                int* __restrict__ table, int nf, T* __restrict__ ZF, int* __restrict__ idf,
                                                T* __restrict__ ZN, int* __restrict__ route, int* s_wave, int* n_known,
                                                int* n_new)
{
    int nknown = 0, nnew = 0;
    for (int base = 0; base < m; base += kSimThreads)
    {
        const int i  = base + threadIdx.x;
        const int id = (i < m) ? tags[i] : 0;
        const int pos = (i < m) ? table[id - 1] : 0;
        const bool known = (i < m) && pos != 0, fresh = (i < m) && pos == 0;
        int        tk, tn;
        const int  ok = block_exclusive_scan(known ? 1 : 0, s_wave, &tk);
        const int  on = block_exclusive_scan(fresh ? 1 : 0, s_wave, &tn);
        if (known)
        {
            const int o = nknown + ok;
            ZF[2 * o]     = Z[2 * i];
            ZF[2 * o + 1] = Z[2 * i + 1];
            idf[o]        = pos;
            if (route)
            {
                route[i] = o;
            }
        }
        if (fresh)
        {
            const int o = nnew + on;
            ZN[2 * o]     = Z[2 * i];
            ZN[2 * o + 1] = Z[2 * i + 1];
            table[id - 1] = nf + o + 1; // (read above by the same thread only: tags within a scan are distinct)
            if (route)
            {
                route[i] = ~o;
            }
        }
        nknown += tk;
        nnew += tn;
    }
    *n_known = nknown;
    *n_new   = nnew;
}

} // namespace cslam
