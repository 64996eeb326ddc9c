// pf_estimate_kernels.hpp -- gfx950 kernels that READ a FastSLAM-2 particle set: the best particle
// (extractStatesFromParticles, slam.h:493-511), the weighted mixture moments of pose and map, and the transposing
// gather of every particle's features (extractFeaturesFromParticles, slam.h:513-539).  None of them writes the store
// (layout: pf_kernels.hpp).
//
// Everything is accumulated in double whatever T is, with no floating-point atomics: a workgroup owns one CHUNK of
// kEstChunk consecutive particles, reduces it in a fixed order (butterfly inside a wave, waves in wave order) and writes
// one partial; the finishing kernels add the partials in chunk order.  Two calls on the same store return the same bits.
//
//   pass 1  (grid: chunks)                 W, sum w^2, sum w (x - x0), sum w (y - y0), sum w sin phi, sum w cos phi about
//                                          particle 0's position, and the chunk's first maximum / minimum weight
//   pass 2  (grid: chunks x (1 + nf/4))    row 0: the pose second moments sum w (Pv + d d^T) about the TRUE mean (known
//                                          from pass 1; the heading residual is wrapped, so it needs the circular mean);
//                                          rows 1..: one wave per feature, first and second moments about the PIVOT
//                                          particle 0's value of that feature -- a point inside the cloud, so that
//                                          S2 - S1 S1^T / W loses digits relative to the cloud's spread, not to its
//                                          distance from the origin.  The chunk's weights sit in LDS for all features.
//   finish  (grid: 1 + nf/256)             partials -> a SUMMARY per moment group (W, mean, second moment about that
//                                          mean) -> the outputs; or the summary itself, for the sharded form
//   combine (grid: 1 + nf/256)             the summaries of all ranks, merged pairwise in rank order
#pragma once

#include <hip/hip_runtime.h>

#include "pf_kernels.hpp"

#pragma clang fp contract(off)

namespace cslam
{

constexpr int kEstChunk      = 1024; // particles per workgroup (4 per thread)
constexpr int kEstP1         = 12;   // doubles per pass-1 partial: 6 sums, 2 x (best weight, index), 2 scaled sums of squares (f64)
constexpr int kEstP2Pose     = 12;   // doubles per pass-2 pose partial: S1 (3), S2 (9, column-major)
constexpr int kEstP2Feat     = 6;    // doubles per (chunk, feature): S1 (2), S2 (4, column-major)
constexpr int kEstFeatPerWg  = 4;    // one wave per feature
constexpr int kEstSumHdr     = 24;   // doubles of a rank summary before its features: W, W2, Ssin, Scos, r(3), S1(3), S2(9), W2 up, W2 down
constexpr int kEstSumFeat    = 6;    // per feature: mean (2), centred second moment (4)
constexpr int kEstOutHdr     = 8;    // doubles in front of the T record of an output block: w_sum, neff, index, found
constexpr int kEstPickMax    = 0;
constexpr int kEstPickMin    = 1;

__device__ inline double est_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        v += __shfl_xor(v, o, 64);
    }
    return v;
}

// v[k] summed over the 256 threads; thread k < N stores the k-th sum to out[k].  s_red: 4 * N doubles of LDS.
template <int N>
__device__ inline void est_block_sum(double* v, double* s_red, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++)
    {
        const double s = est_wave_sum(v[k]);
        if (lane == 0)
        {
            s_red[wave * N + k] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < N)
    {
        const int k = threadIdx.x;
        out[k]      = ((s_red[k] + s_red[N + k]) + s_red[2 * N + k]) + s_red[3 * N + k];
    }
}

// is candidate b a better pick than a?  index < 0: no candidate (a NaN weight is never one).  Ties: the lower index,
// the "first" rule of std::minmax_element (slam.h:505-506).
__device__ inline bool est_better(int pick, double wa, long long ia, double wb, long long ib)
{
    if (ib < 0)
    {
        return false;
    }
    if (ia < 0)
    {
        return true;
    }
    const bool strictly = (pick == kEstPickMin) ? (wb < wa) : (wb > wa);
    return strictly || (wb == wa && ib < ia);
}

struct EstTotals
{
    double W, W2, Sx, Sy, Ss, Sc;
};

// the pass-1 partials added in chunk order (every thread computes the same)
__device__ inline EstTotals est_totals(const double* __restrict__ part1, int nchunks)
{
    EstTotals t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunks; c++)
    {
        const double* p = part1 + (size_t)c * kEstP1;
        t.W += p[0];
        t.W2 += p[1];
        t.Sx += p[2];
        t.Sy += p[3];
        t.Ss += p[4];
        t.Sc += p[5];
    }
    return t;
}

// x = x0 + sum w (x - x0) / W, y likewise, phi = atan2(sum w sin, sum w cos)
__device__ inline void est_pose_mean(const EstTotals& t, double x0, double y0, double* m)
{
    m[0] = x0 + t.Sx / t.W;
    m[1] = y0 + t.Sy / t.W;
    m[2] = atan2(t.Ss, t.Sc);
}

// Neff = W^2 / sum w^2.  f64 weights beyond 2^-511 .. 2^512 take their squares out of the range of double although W and
// every moment are fine, so an f64 set also carries the sums of the squares of 2^512 w and of 2^-512 w (fixed scales:
// partials and rank summaries add as they are).  Whenever W^2 and sum w^2 are normal numbers Neff is formed from them as
// ever -- and since a power of two scales every term, every partial sum and W^2 exactly, the other two forms would give
// the same bits there.  f32 weights never leave that range (their squares span 2^-298 .. 2^256).
constexpr double kEstUp = 0x1p+512, kEstDown = 0x1p-512;

__device__ inline double est_neff(double W, double W2, double W2u, double W2d, bool wide)
{
    if (!wide || (W2 >= 2.2250738585072014e-308 && W2 <= 1.7976931348623157e+308 && W * W <= 1.7976931348623157e+308))
    {
        return (W * W) / W2;
    }
    if (W2 < 2.2250738585072014e-308)
    {
        const double Wu = W * kEstUp;
        return (Wu * Wu) / W2u;
    }
    const double Wd = W * kEstDown;
    return (Wd * Wd) / W2d;
}

// the scaled sums of squares of the pass-1 partials added in chunk order
__device__ inline void est_wide_squares(const double* __restrict__ part1, int nchunks, double* up, double* down)
{
    double u = 0.0, d = 0.0;
    for (int c = 0; c < nchunks; c++)
    {
        u += part1[(size_t)c * kEstP1 + 10];
        d += part1[(size_t)c * kEstP1 + 11];
    }
    *up   = u;
    *down = d;
}

__device__ inline bool est_degenerate(double W)
{
    return !(W > 0.0) || !isfinite(W);
}

// ------------------------------------------------------------------------------------------------ pass 1
template <typename T>
__global__ void __launch_bounds__(256) pf_est_pass1_kernel(PfStore<T> s, double* __restrict__ part1)
{
    __shared__ double s_red[4 * 6];
    __shared__ double s_bw[2][4];
    __shared__ int    s_bi[2][4];
    const int    np = s.np;
    const int    base = blockIdx.x * kEstChunk, end = min(base + kEstChunk, np);
    const double x0 = (double)s.xv[0], y0 = (double)s.xv[np];
    double       acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double       sq[2]  = {0.0, 0.0}; // (f64) sums of the squares of 2^512 w and 2^-512 w: est_neff
    double       bw[2]  = {0.0, 0.0};
    int          bi[2]  = {-1, -1};
    for (int p = base + (int)threadIdx.x; p < end; p += 256)
    {
        const double w = (double)s.w[p];
        const double x = (double)s.xv[p], y = (double)s.xv[(size_t)np + p], phi = (double)s.xv[(size_t)2 * np + p];
        acc[0] += w;
        acc[1] += w * w;
        acc[2] += w * (x - x0);
        acc[3] += w * (y - y0);
        acc[4] += w * sin(phi);
        acc[5] += w * cos(phi);
        if (sizeof(T) == 8)
        {
            const double wu = w * kEstUp, wd = w * kEstDown;
            sq[0] += wu * wu;
            sq[1] += wd * wd;
        }
        if (w == w)
        {
#pragma unroll
            for (int k = 0; k < 2; k++)
            {
                if (est_better(k, bw[k], bi[k], w, p))
                {
                    bw[k] = w;
                    bi[k] = p;
                }
            }
        }
    }
    double* out = part1 + (size_t)blockIdx.x * kEstP1;
    est_block_sum<6>(acc, s_red, out);
    if (sizeof(T) == 8)
    {
        __shared__ double s_sq[4 * 2];
        est_block_sum<2>(sq, s_sq, out + 10);
    }
    else if (threadIdx.x < 2)
    {
        out[10 + threadIdx.x] = 0.0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 2; k++)
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
        {
            const double ow = __shfl_xor(bw[k], o, 64);
            const int    oi = __shfl_xor(bi[k], o, 64);
            if (est_better(k, bw[k], bi[k], ow, oi))
            {
                bw[k] = ow;
                bi[k] = oi;
            }
        }
        if (lane == 0)
        {
            s_bw[k][wave] = bw[k];
            s_bi[k][wave] = bi[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2)
    {
        const int k = threadIdx.x;
        double    w = s_bw[k][0];
        int       i = s_bi[k][0];
        for (int v = 1; v < 4; v++)
        {
            if (est_better(k, w, i, s_bw[k][v], s_bi[k][v]))
            {
                w = s_bw[k][v];
                i = s_bi[k][v];
            }
        }
        out[6 + 2 * k] = w;
        out[7 + 2 * k] = (double)i;
    }
}

// ------------------------------------------------------------------------------------------------ pass 2
template <typename T>
__global__ void __launch_bounds__(256) pf_est_pass2_kernel(PfStore<T> s, const double* __restrict__ part1, int nchunks,
                                                            double* __restrict__ part2_pose,
                                                            double* __restrict__ part2_feat)
{
    __shared__ double s_w[kEstChunk];
    __shared__ double s_red[4 * kEstP2Pose];
    const int np   = s.np;
    const int base = blockIdx.x * kEstChunk, end = min(base + kEstChunk, np);
    if (blockIdx.y == 0)
    {
        // pose: sum w d and sum w (Pv + d d^T), d = (x - xbar, y - ybar, pi2pi(phi - phibar))
        const EstTotals t = est_totals(part1, nchunks);
        double          m[3];
        est_pose_mean(t, (double)s.xv[0], (double)s.xv[np], m);
        double acc[kEstP2Pose];
#pragma unroll
        for (int k = 0; k < kEstP2Pose; k++)
        {
            acc[k] = 0.0;
        }
        for (int p = base + (int)threadIdx.x; p < end; p += 256)
        {
            const double w = (double)s.w[p];
            double       d[3];
            d[0] = (double)s.xv[p] - m[0];
            d[1] = (double)s.xv[(size_t)np + p] - m[1];
            d[2] = pi2pi<double>((double)s.xv[(size_t)2 * np + p] - m[2]);
#pragma unroll
            for (int i = 0; i < 3; i++)
            {
                acc[i] += w * d[i];
            }
#pragma unroll
            for (int e = 0; e < 9; e++)
            {
                acc[3 + e] += w * ((double)s.pv[(size_t)e * np + p] + d[e % 3] * d[e / 3]);
            }
        }
        est_block_sum<kEstP2Pose>(acc, s_red, part2_pose + (size_t)blockIdx.x * kEstP2Pose);
        return;
    }
    // map: the chunk's weights once into LDS, then one wave per feature
    for (int i = threadIdx.x; i < end - base; i += 256)
    {
        s_w[i] = (double)s.w[base + i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f    = ((int)blockIdx.y - 1) * kEstFeatPerWg + wave;
    if (f >= s.nf)
    {
        return;
    }
    const T*     xf0 = s.xf + (size_t)(2 * f) * np;
    const T*     xf1 = xf0 + np;
    const T*     pf0 = s.pf + (size_t)(4 * f) * np;
    const double px = (double)xf0[0], py = (double)xf1[0];
    double       a[kEstP2Feat] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < end - base; i += 64)
    {
        const int    p  = base + i;
        const double w  = s_w[i];
        const double dx = (double)xf0[p] - px, dy = (double)xf1[p] - py;
        a[0] += w * dx;
        a[1] += w * dy;
        a[2] += w * ((double)pf0[p] + dx * dx);
        a[3] += w * ((double)pf0[(size_t)np + p] + dy * dx);
        a[4] += w * ((double)pf0[(size_t)2 * np + p] + dx * dy);
        a[5] += w * ((double)pf0[(size_t)3 * np + p] + dy * dy);
    }
    double* out = part2_feat + ((size_t)blockIdx.x * s.nf + f) * kEstP2Feat;
#pragma unroll
    for (int k = 0; k < kEstP2Feat; k++)
    {
        const double v = est_wave_sum(a[k]);
        if (lane == 0)
        {
            out[k] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ summaries -> outputs
// record layout of an output block's T part: pf_pack_kernel's [w, xv(3), pv(9), xf(2 nf), pf(4 nf)]
template <typename T>
__device__ inline void est_write_pose(const double* __restrict__ h, bool bad, double* __restrict__ out_hdr, T* __restrict__ rec)
{
    const double nan = __builtin_nan("");
    out_hdr[0]       = h[0];
    out_hdr[1]       = bad ? nan : est_neff(h[0], h[1], h[19], h[20], sizeof(T) == 8);
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        rec[1 + i] = (T)(bad ? nan : h[4 + i]);
    }
#pragma unroll
    for (int e = 0; e < 9; e++)
    {
        rec[4 + e] = (T)(bad ? nan : h[10 + e] / h[0]);
    }
}

template <typename T>
__device__ inline void est_write_feature(const double* __restrict__ g, double W, bool bad, int f, int nf, T* __restrict__ rec)
{
    const double nan = __builtin_nan("");
    rec[13 + 2 * f]     = (T)(bad ? nan : g[0]);
    rec[13 + 2 * f + 1] = (T)(bad ? nan : g[1]);
#pragma unroll
    for (int e = 0; e < 4; e++)
    {
        rec[13 + 2 * nf + 4 * f + e] = (T)(bad ? nan : g[2 + e] / W);
    }
}

// One handle's partials -> its summary.  summary != nullptr: store it (kEstSumHdr + kEstSumFeat * nf doubles; the
// sharded form gathers these); else write the outputs.  Block 0 does the pose, blocks 1.. the features (when part2_feat).
template <typename T>
__global__ void __launch_bounds__(256) pf_est_finish_kernel(PfStore<T> s, const double* __restrict__ part1,
                                                             const double* __restrict__ part2_pose,
                                                             const double* __restrict__ part2_feat, int nchunks,
                                                             double* __restrict__ summary, double* __restrict__ out_hdr,
                                                             T* __restrict__ rec)
{
    const EstTotals t = est_totals(part1, nchunks);
    if (blockIdx.x == 0)
    {
        __shared__ double s_pose[kEstP2Pose];
        if ((int)threadIdx.x < kEstP2Pose)
        {
            double v = 0.0;
            for (int c = 0; c < nchunks; c++)
            {
                v += part2_pose[(size_t)c * kEstP2Pose + threadIdx.x];
            }
            s_pose[threadIdx.x] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0)
        {
            double h[kEstSumHdr];
            h[0] = t.W;
            h[1] = t.W2;
            h[2] = t.Ss;
            h[3] = t.Sc;
            est_pose_mean(t, (double)s.xv[0], (double)s.xv[s.np], h + 4);
            for (int k = 0; k < kEstP2Pose; k++)
            {
                h[7 + k] = s_pose[k];
            }
            est_wide_squares(part1, nchunks, &h[19], &h[20]);
            for (int k = 21; k < kEstSumHdr; k++)
            {
                h[k] = 0.0;
            }
            if (summary)
            {
                for (int k = 0; k < kEstSumHdr; k++)
                {
                    summary[k] = h[k];
                }
            }
            else
            {
                est_write_pose<T>(h, est_degenerate(t.W), out_hdr, rec);
            }
        }
        return;
    }
    const int f = ((int)blockIdx.x - 1) * 256 + (int)threadIdx.x;
    if (f >= s.nf)
    {
        return;
    }
    double a[kEstP2Feat] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunks; c++)
    {
        const double* p = part2_feat + ((size_t)c * s.nf + f) * kEstP2Feat;
#pragma unroll
        for (int k = 0; k < kEstP2Feat; k++)
        {
            a[k] += p[k];
        }
    }
    // about the pivot -> about the mean: m1 = S1 / W, mean = pivot + m1, M2 = S2 - S1 m1^T
    const double m1x = (t.W != 0.0) ? a[0] / t.W : 0.0, m1y = (t.W != 0.0) ? a[1] / t.W : 0.0;
    double       g[kEstSumFeat];
    g[0] = (double)s.xf[(size_t)(2 * f) * s.np] + m1x;
    g[1] = (double)s.xf[(size_t)(2 * f + 1) * s.np] + m1y;
    g[2] = a[2] - a[0] * m1x;
    g[3] = a[3] - a[1] * m1x;
    g[4] = a[4] - a[0] * m1y;
    g[5] = a[5] - a[1] * m1y;
    if (summary)
    {
        for (int k = 0; k < kEstSumFeat; k++)
        {
            summary[kEstSumHdr + (size_t)f * kEstSumFeat + k] = g[k];
        }
    }
    else
    {
        est_write_feature<T>(g, t.W, est_degenerate(t.W), f, s.nf, rec);
    }
}

// The summaries of `world` ranks ([rank][stride] doubles) merged pairwise in rank order; every rank runs this on the same
// gathered bytes and gets the same bits.  A group's state is (W, reference point r, S1 = sum w (x - r),
// S2 = sum w (P + (x - r)(x - r)^T)); merging a and b moves both to the merged mean r' (heading: the circular mean of
// the merged sin / cos sums) by s = r' - r:  S1' = S1 - W s,  S2' = S2 - s S1^T - S1 s^T + W s s^T, then adds.  With
// S1 = 0 that is Chan's update M2a + M2b + delta delta^T Wa Wb / (Wa + Wb), which the features use directly.
template <typename T>
__global__ void __launch_bounds__(256) pf_est_combine_kernel(const double* __restrict__ all, int world, int stride, int nf,
                                                              int with_map, double* __restrict__ out_hdr, T* __restrict__ rec)
{
    if (blockIdx.x == 0)
    {
        if (threadIdx.x != 0)
        {
            return;
        }
        double h[kEstSumHdr];
        for (int k = 0; k < kEstSumHdr; k++)
        {
            h[k] = all[k];
        }
        for (int r = 1; r < world; r++)
        {
            const double* b   = all + (size_t)r * stride;
            const double  Wa = h[0], Wb = b[0], Wab = Wa + Wb;
            const double  frac = (Wab != 0.0) ? Wb / Wab : 0.0;
            const double  Ss = h[2] + b[2], Sc = h[3] + b[3];
            double        rn[3], sa[3], sb[3];
            rn[0] = h[4] + (b[4] - h[4]) * frac;
            rn[1] = h[5] + (b[5] - h[5]) * frac;
            rn[2] = atan2(Ss, Sc);
            for (int i = 0; i < 2; i++)
            {
                sa[i] = rn[i] - h[4 + i];
                sb[i] = rn[i] - b[4 + i];
            }
            sa[2] = pi2pi<double>(rn[2] - h[6]);
            sb[2] = pi2pi<double>(rn[2] - b[6]);
            double S2[9];
            for (int e = 0; e < 9; e++)
            {
                const int i = e % 3, j = e / 3;
                const double ma = ((h[10 + e] - sa[i] * h[7 + j]) - h[7 + i] * sa[j]) + Wa * (sa[i] * sa[j]);
                const double mb = ((b[10 + e] - sb[i] * b[7 + j]) - b[7 + i] * sb[j]) + Wb * (sb[i] * sb[j]);
                S2[e]           = ma + mb;
            }
            for (int i = 0; i < 3; i++)
            {
                h[7 + i] = (h[7 + i] - Wa * sa[i]) + (b[7 + i] - Wb * sb[i]);
                h[4 + i] = rn[i];
            }
            for (int e = 0; e < 9; e++)
            {
                h[10 + e] = S2[e];
            }
            h[0] = Wab;
            h[1] += b[1];
            h[19] += b[19];
            h[20] += b[20];
            h[2] = Ss;
            h[3] = Sc;
        }
        est_write_pose<T>(h, est_degenerate(h[0]), out_hdr, rec);
        return;
    }
    const int f = ((int)blockIdx.x - 1) * 256 + (int)threadIdx.x;
    if (!with_map || f >= nf)
    {
        return;
    }
    double g[kEstSumFeat];
    double W = all[0];
    for (int k = 0; k < kEstSumFeat; k++)
    {
        g[k] = all[kEstSumHdr + (size_t)f * kEstSumFeat + k];
    }
    for (int r = 1; r < world; r++)
    {
        const double* b   = all + (size_t)r * stride;
        const double* gb  = b + kEstSumHdr + (size_t)f * kEstSumFeat;
        const double  Wb = b[0], Wab = W + Wb;
        const double  frac = (Wab != 0.0) ? Wb / Wab : 0.0;
        const double  dx = gb[0] - g[0], dy = gb[1] - g[1];
        const double  c  = W * frac; // Wa Wb / (Wa + Wb)
        g[2] = (g[2] + gb[2]) + (dx * dx) * c;
        g[3] = (g[3] + gb[3]) + (dy * dx) * c;
        g[4] = (g[4] + gb[4]) + (dx * dy) * c;
        g[5] = (g[5] + gb[5]) + (dy * dy) * c;
        g[0] += dx * frac;
        g[1] += dy * frac;
        W = Wab;
    }
    est_write_feature<T>(g, W, est_degenerate(W), f, nf, rec);
}

// ------------------------------------------------------------------------------------------------ the best particle
// The chunks' candidates in chunk order -> the pick; its record gathered into rec (pf_pack_kernel's layout).
// out_hdr[2] = index + index_offset (the global index of a sharded set), out_hdr[3] = 1 if any weight was not NaN
// (else index 0), out_hdr[4] = the weight as a double.  One workgroup.
template <typename T>
__global__ void __launch_bounds__(256) pf_best_finish_kernel(PfStore<T> s, const double* __restrict__ part1, int nchunks,
                                                              int pick, long long index_offset, double* __restrict__ out_hdr,
                                                              T* __restrict__ rec)
{
    double    bw = 0.0;
    long long bi = -1;
    for (int c = 0; c < nchunks; c++)
    {
        const double*   p  = part1 + (size_t)c * kEstP1 + 6 + 2 * pick;
        const long long ci = (long long)p[1];
        if (est_better(pick, bw, bi, p[0], ci))
        {
            bw = p[0];
            bi = ci;
        }
    }
    const int idx = (bi < 0) ? 0 : (int)bi;
    if (threadIdx.x == 0)
    {
        out_hdr[2] = (double)((long long)idx + index_offset);
        out_hdr[3] = (bi < 0) ? 0.0 : 1.0;
        out_hdr[4] = (double)s.w[idx];
    }
    const int len = 13 + 6 * s.nf;
    for (int e = threadIdx.x; e < len; e += 256)
    {
        T v;
        if (e == 0)
        {
            v = s.w[idx];
        }
        else if (e < 4)
        {
            v = s.xv[(size_t)(e - 1) * s.np + idx];
        }
        else if (e < 13)
        {
            v = s.pv[(size_t)(e - 4) * s.np + idx];
        }
        else if (e < 13 + 2 * s.nf)
        {
            v = s.xf[(size_t)(e - 13) * s.np + idx];
        }
        else
        {
            v = s.pf[(size_t)(e - 13 - 2 * s.nf) * s.np + idx];
        }
        rec[e] = v;
    }
}

// Every rank's local pick ([rank][kEstOutHdr] doubles, [rank][len] records), in rank order: the better weight wins, the
// lower global index wins ties.  One workgroup.
template <typename T>
__global__ void __launch_bounds__(256) pf_best_combine_kernel(const double* __restrict__ hdrs, const T* __restrict__ recs,
                                                               int world, int len, int pick, double* __restrict__ out_hdr,
                                                               T* __restrict__ rec)
{
    double    bw = 0.0;
    long long bi = -1;
    int       br = 0;
    for (int r = 0; r < world; r++)
    {
        const double*   h  = hdrs + (size_t)r * kEstOutHdr;
        const long long gi = (h[3] != 0.0) ? (long long)h[2] : -1;
        if (est_better(pick, bw, bi, h[4], gi))
        {
            bw = h[4];
            bi = gi;
            br = r;
        }
    }
    if (threadIdx.x == 0)
    {
        out_hdr[2] = (bi < 0) ? 0.0 : (double)bi; // (no candidate anywhere: rank 0's particle 0)
        out_hdr[3] = (bi < 0) ? 0.0 : 1.0;
        out_hdr[4] = hdrs[(size_t)br * kEstOutHdr + 4];
    }
    for (int e = threadIdx.x; e < len; e += 256)
    {
        rec[e] = recs[(size_t)br * len + e];
    }
}

// ------------------------------------------------------------------------------------------------ all features
// slam.h:531-536: out is 2 x (np nf) column-major with particle p's 2 x nf block at column p nf, i.e.
// out[p][r] = xf[r][p] for the 2 nf rows r = 2 f + c of the store: a transpose, 64 x 64 tiles through LDS so that both
// the loads (p fastest) and the stores (r fastest) are coalesced.  grid: (np / 64, 2 nf / 64), 256 threads.
template <typename T>
__global__ void __launch_bounds__(256) pf_all_features_kernel(PfStore<T> s, T* __restrict__ out)
{
    __shared__ T tile[64][65];
    const int    np = s.np, nr = 2 * s.nf;
    const int    p0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int    tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int k = ty; k < 64; k += 4)
    {
        const int r = r0 + k, p = p0 + tx;
        if (r < nr && p < np)
        {
            tile[k][tx] = s.xf[(size_t)r * np + p];
        }
    }
    __syncthreads();
    for (int k = ty; k < 64; k += 4)
    {
        const int p = p0 + k, r = r0 + tx;
        if (r < nr && p < np)
        {
            out[(size_t)p * nr + r] = tile[tx][k];
        }
    }
}

} // namespace cslam
