// pf_score_kernels.hpp -- the score and the trajectory log of the particle filter (cslam_pf_score / _score_sharded): the
// estimate a caller would have read at this point -- the mixture moments of cslam_pf_estimate or the maximum-weight
// particle of cslam_pf_best_particle, the line test/main.cpp:330 prints from slam.h:493-511 -- scored against the true
// pose and a true position per state feature, accumulated in totals that stay on the device until the study ends.
//
// The estimate kernels (pf_estimate_kernels.hpp) run unchanged and leave the block [hdr | rec] in HBM: kEstOutHdr
// doubles, then pf_pack_kernel's record [w, Xv(3), Pv(9), XF(2 nf), PF(4 nf)] in the handle's dtype T.  Two launches
// follow them on the handle's stream and read that block, i.e. the values AFTER their rounding to T:
//   pf_score_landmarks_kernel  grid ceil(c / 256), one lane per scored feature: e = XF_f - truth_f and the closed-form
//                              NEES of the 2 x 2 block PF_f in f64; the workgroup adds its five partials (valid, bad,
//                              inside the gate, sum err^2, sum NEES) in a fixed order -- a shuffle tree inside each wave,
//                              then waves 0..3 through LDS -- into its slot of the scratch [blocks][5].  Not launched
//                              when no feature is scored.
//   pf_score_finish_kernel     one workgroup, one lane: adds the slots in block order, scores the pose (3 x 3 Cholesky
//                              of the lower triangle of Pv in f64), updates the eleven totals with plain loads and
//                              stores (the stream orders the calls), writes the call's series record (4 f32) and track
//                              record (5 f64) while there is room.
// The arithmetic, the rules and the total indices are those of ekf_score_kernels.hpp with one instance.  No atomics: two
// identical runs give identical bits.  Neither kernel writes the particle store.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/cslam.h"
#include "pf_estimate_kernels.hpp"

#pragma clang fp contract(off)

namespace cslam
{

constexpr int kPfScoreParts = 5; // valid, bad, inside the gate, sum err^2, sum NEES
constexpr int kPfScoreTrack = 5; // doubles per track record

__device__ inline bool pf_score_finite(double v) { return v == v && v - v == 0.0; }

// (-pi, pi]
__device__ inline double pf_score_wrap(double d)
{
    const double two_pi = 6.283185307179586476925286766559;
    return d - two_pi * ceil((d - 3.141592653589793238462643383279) / two_pi);
}

// rec: the record of the estimate block (nf features); truth [count][2] doubles: the true position of state feature
// j + 1, count <= nf; a non-finite row (or estimate) counts as a bad block.  parts [gridDim.x][kPfScoreParts].
template <typename T>
__global__ void __launch_bounds__(256) pf_score_landmarks_kernel(const T* __restrict__ rec, int nf, int count,
                                                                 const double* __restrict__ truth, double gate,
                                                                 double* __restrict__ parts)
{
    __shared__ double s_part[4][kPfScoreParts];
    const int         f = blockIdx.x * 256 + threadIdx.x;
    double            v[kPfScoreParts] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (f < count)
    {
        const T*     xf  = rec + 13 + 2 * (size_t)f;
        const T*     pf  = rec + 13 + 2 * (size_t)nf + 4 * (size_t)f;
        const double e0 = (double)xf[0] - truth[2 * (size_t)f], e1 = (double)xf[1] - truth[2 * (size_t)f + 1];
        const double p00 = (double)pf[0], p10 = (double)pf[1], p11 = (double)pf[3];
        const double det  = p00 * p11 - p10 * p10;
        const double nees = (p11 * e0 * e0 - 2.0 * p10 * e0 * e1 + p00 * e1 * e1) / det;
        const double err2 = e0 * e0 + e1 * e1;
        const bool   ok   = pf_score_finite(e0) && pf_score_finite(e1) && pf_score_finite(p00) && pf_score_finite(p10) &&
                        pf_score_finite(p11) && p00 > 0.0 && det > 0.0 && pf_score_finite(nees);
        if (ok)
        {
            v[0] = 1.0;
            v[2] = nees <= gate ? 1.0 : 0.0;
            v[3] = err2;
            v[4] = nees;
        }
        else
        {
            v[1] = 1.0;
        }
    }
    // fixed order: the shuffle tree of a wave, then waves 0..3 (every lane takes part; lanes past count hold zeros)
    for (int q = 0; q < kPfScoreParts; q++)
    {
        for (int off = 32; off > 0; off >>= 1)
        {
            v[q] += __shfl_down(v[q], off, 64);
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
    {
        for (int q = 0; q < kPfScoreParts; q++)
        {
            s_part[wave][q] = v[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < kPfScoreParts)
    {
        const int q = threadIdx.x;
        parts[(size_t)blockIdx.x * kPfScoreParts + q] = ((s_part[0][q] + s_part[1][q]) + s_part[2][q]) + s_part[3][q];
    }
}

// hdr | rec: the estimate block.  blocks: the slots pf_score_landmarks_kernel has just written (0: no feature scored).
// estimator CSLAM_PF_SCORE_MEAN: the track record is (Xv, W = hdr[0], Neff = hdr[1]); CSLAM_PF_SCORE_BEST: (Xv, the
// weight hdr[4], the index hdr[2]).  record: the index of this call's series / track record, < 0 when they are full or
// absent (an exact integer in a double, as the true pose travels).  totals [CSLAM_SCORE_FIELDS], series [capacity][4],
// track [capacity][kPfScoreTrack].
template <typename T>
__global__ void __launch_bounds__(64) pf_score_finish_kernel(const double* __restrict__ hdr, const T* __restrict__ rec,
                                                             const double* __restrict__ parts, int blocks, double xt,
                                                             double yt, double pt, double gate, int estimator,
                                                             double* __restrict__ totals, float* __restrict__ series,
                                                             double* __restrict__ track, double record)
{
    if (threadIdx.x != 0)
    {
        return;
    }
    double lm[kPfScoreParts] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < blocks; b++)
    {
        const double* p = parts + (size_t)b * kPfScoreParts;
        for (int q = 0; q < kPfScoreParts; q++)
        {
            lm[q] += p[q];
        }
    }
    // the pose: e = (x - xt, y - yt, wrap(phi - phit)); the lower triangle of Pv (column-major: P[r, c] = pv[3 c + r])
    const T*     x  = rec + 1;
    const T*     pv = rec + 4;
    const double e0 = (double)x[0] - xt, e1 = (double)x[1] - yt;
    const double e2 = pf_score_wrap((double)x[2] - pt);
    const double a00 = (double)pv[0], a10 = (double)pv[1], a20 = (double)pv[2], a11 = (double)pv[4], a21 = (double)pv[5],
                 a22 = (double)pv[8];
    bool ok = pf_score_finite(e0) && pf_score_finite(e1) && pf_score_finite(e2) && pf_score_finite(a00) &&
              pf_score_finite(a10) && pf_score_finite(a20) && pf_score_finite(a11) && pf_score_finite(a21) &&
              pf_score_finite(a22);
    double nees = 0.0;
    if (ok)
    {
        // A = L L^T, L y = e, NEES = y^T y
        const double d0 = a00;
        ok              = d0 > 0.0;
        if (ok)
        {
            const double l00 = sqrt(d0), l10 = a10 / l00, l20 = a20 / l00;
            const double d1 = a11 - l10 * l10;
            ok              = d1 > 0.0 && pf_score_finite(d1);
            if (ok)
            {
                const double l11 = sqrt(d1), l21 = (a21 - l20 * l10) / l11;
                const double d2 = a22 - l20 * l20 - l21 * l21;
                ok              = d2 > 0.0 && pf_score_finite(d2);
                if (ok)
                {
                    const double l22 = sqrt(d2);
                    const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / l11, y2 = (e2 - l20 * y0 - l21 * y1) / l22;
                    nees = y0 * y0 + y1 * y1 + y2 * y2;
                    ok   = pf_score_finite(nees);
                }
            }
        }
    }
    const double err2 = e0 * e0 + e1 * e1;
    if (ok)
    {
        totals[CSLAM_SCORE_POSE_N] += 1.0;
        totals[CSLAM_SCORE_POSE_IN] += nees <= gate ? 1.0 : 0.0;
        totals[CSLAM_SCORE_POSE_ERR2] += err2;
        totals[CSLAM_SCORE_POSE_EPHI2] += e2 * e2;
        totals[CSLAM_SCORE_POSE_NEES] += nees;
    }
    else
    {
        totals[CSLAM_SCORE_POSE_BAD] += 1.0;
    }
    totals[CSLAM_SCORE_LM_N] += lm[0];
    totals[CSLAM_SCORE_LM_BAD] += lm[1];
    totals[CSLAM_SCORE_LM_IN] += lm[2];
    totals[CSLAM_SCORE_LM_ERR2] += lm[3];
    totals[CSLAM_SCORE_LM_NEES] += lm[4];
    if (record >= 0.0)
    {
        const size_t r   = (size_t)record;
        const float  nan = __builtin_nanf("");
        float*       s   = series + r * 4;
        s[0]             = ok ? (float)err2 : nan;
        s[1]             = ok ? (float)nees : nan;
        s[2]             = lm[0] > 0.0 ? (float)(lm[3] / lm[0]) : nan;
        s[3]             = lm[0] > 0.0 ? (float)(lm[4] / lm[0]) : nan;
        double* t        = track + r * kPfScoreTrack;
        t[0]             = (double)x[0];
        t[1]             = (double)x[1];
        t[2]             = (double)x[2];
        t[3]             = estimator == CSLAM_PF_SCORE_BEST ? hdr[4] : hdr[0];
        t[4]             = estimator == CSLAM_PF_SCORE_BEST ? hdr[2] : hdr[1];
    }
}

} // namespace cslam
