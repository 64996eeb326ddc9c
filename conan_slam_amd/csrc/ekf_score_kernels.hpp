// ekf_score_kernels.hpp -- the score of a Monte-Carlo study (cslam_ekf_batch_score / _score_scan): per instance the pose
// error and NEES against the true pose (the pose test/main.cpp:136 prints), the map error and every landmark's NEES
// e^T P_jj^-1 e against a true position per state feature (the blocks EKF.cpp:131-144 reads), accumulated in totals
// that stay on the device until the study ends.  Nothing here writes the filter's state: X, the pose stripe, Ps and
// the pending panels are read as they stand (landmark_read_body: P_jj = Ps_jj - sum over the pending columns), so the
// values are those cslam_ekf_batch_get_landmarks would return at that point and the run continues bit for bit.
//
// Two launches on the main stream:
//   ekf_score_landmarks_batch  grid (ceil(count / 256), I), the landmark read's mapping: one lane per (instance,
//                              feature), the lanes of a wave read consecutive scalars of each pending column.  Each lane
//                              forms e and the closed-form NEES in f64; the workgroup adds its five partials (valid,
//                              bad, inside the gate, sum err^2, sum NEES) in a fixed order -- a shuffle tree inside
//                              each wave, then the four waves in wave order through LDS -- and stores them in its slot
//                              of the scratch [I][blocks][5].
//   ekf_score_finish_batch     one workgroup per instance: lane 0 adds the slots in block order, scores the pose (3 x 3
//                              Cholesky of the stripe block in f64), updates the instance's totals with plain loads and
//                              stores (the stream orders the calls) and writes the call's series record.
// No atomics: the totals of a run are reproducible bit for bit.
//
// The single handle (cslam_ekf_score, f32 and f64) has the same two launches as templates at the end of this file:
// ekf_score_landmarks<T> and ekf_score_finish<T>, which also log the pose, trace(P) and n of every call.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/cslam.h"
#include "ekf_landmark_kernels.hpp"

namespace cslam
{

constexpr int kScoreParts = 5; // valid, bad, inside the gate, sum err^2, sum NEES

__device__ inline bool score_finite(double v) { return v == v && v - v == 0.0; }

// (-pi, pi]
__device__ inline double score_wrap(double d)
{
    const double two_pi = 6.283185307179586476925286766559;
    return d - two_pi * ceil((d - 3.141592653589793238462643383279) / two_pi);
}

// (The batch kernels are plain functions, so exactly one translation unit may hold them: cslam_ekf_batch.hip.  The single
// handle's translation unit defines CSLAM_SCORE_SINGLE_ONLY and gets the helpers above and the templates below.)
#ifndef CSLAM_SCORE_SINGLE_ONLY

// truth [count][2]: the true position of state feature j + 1; a non-finite row counts as a bad block
__global__ void __launch_bounds__(256) ekf_score_landmarks_batch(const float* __restrict__ X, const float* __restrict__ Pv,
                                                                 const float* __restrict__ P, int ldp,
                                                                 const float* __restrict__ W, long sW, int kp, int count,
                                                                 const float* __restrict__ truth, double gate,
                                                                 double* __restrict__ parts)
{
    __shared__ double s_part[4][kScoreParts];
    const int         j = blockIdx.x * 256 + threadIdx.x;
    const size_t      i = blockIdx.y;
    const size_t      L = (size_t)ldp;
    double            v[kScoreParts] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < count)
    {
        float x[2], pll[4];
        landmark_read_body<float>(X + i * L, Pv + i * 3 * L, P + i * L * L, ldp, 1, W + i * (size_t)sW, ldp, kp, nullptr,
                                  1 + j, 0, x, pll, nullptr);
        const double e0 = (double)x[0] - (double)truth[2 * j], e1 = (double)x[1] - (double)truth[2 * j + 1];
        const double p00 = pll[0], p10 = pll[1], p11 = pll[3];
        const double det  = p00 * p11 - p10 * p10;
        const double nees = (p11 * e0 * e0 - 2.0 * p10 * e0 * e1 + p00 * e1 * e1) / det;
        const double err2 = e0 * e0 + e1 * e1;
        const bool   ok   = score_finite(e0) && score_finite(e1) && score_finite(p00) && score_finite(p10) &&
                        score_finite(p11) && p00 > 0.0 && det > 0.0 && score_finite(nees);
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
    for (int q = 0; q < kScoreParts; q++)
    {
        for (int off = 32; off > 0; off >>= 1)
        {
            v[q] += __shfl_down(v[q], off, 64);
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
    {
        for (int q = 0; q < kScoreParts; q++)
        {
            s_part[wave][q] = v[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < kScoreParts)
    {
        const int q = threadIdx.x;
        double*   o = parts + (i * gridDim.x + blockIdx.x) * kScoreParts;
        o[q]        = ((s_part[0][q] + s_part[1][q]) + s_part[2][q]) + s_part[3][q];
    }
}

// blocks: the slots ekf_score_landmarks_batch has just written per instance (0: no feature to score); record < 0: the
// series is full or absent.  totals [I][CSLAM_SCORE_FIELDS], series [capacity][I][4].
__global__ void __launch_bounds__(64) ekf_score_finish_batch(const float* __restrict__ X, const float* __restrict__ Pv, int ldp,
                                                             const double* __restrict__ parts, int blocks, float xt, float yt,
                                                             float pt, double gate, double* __restrict__ totals,
                                                             float* __restrict__ series, int record, int instances)
{
    if (threadIdx.x != 0)
    {
        return;
    }
    const size_t i = blockIdx.x;
    const size_t L = (size_t)ldp;
    double       lm[kScoreParts] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < blocks; b++)
    {
        const double* p = parts + (i * blocks + b) * kScoreParts;
        for (int q = 0; q < kScoreParts; q++)
        {
            lm[q] += p[q];
        }
    }
    // the pose: e = (x - xt, y - yt, wrap(phi - phit)); the lower triangle of the stripe block, P[r, c] = Pv[c ldp + r]
    const float*  x  = X + i * L;
    const float*  pv = Pv + i * 3 * L;
    const double  e0 = (double)x[0] - (double)xt, e1 = (double)x[1] - (double)yt;
    const double  e2 = score_wrap((double)x[2] - (double)pt);
    const double  a00 = pv[0], a10 = pv[1], a20 = pv[2], a11 = pv[L + 1], a21 = pv[L + 2], a22 = pv[2 * L + 2];
    bool          ok = score_finite(e0) && score_finite(e1) && score_finite(e2) && score_finite(a00) && score_finite(a10) &&
              score_finite(a20) && score_finite(a11) && score_finite(a21) && score_finite(a22);
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
            ok              = d1 > 0.0 && score_finite(d1);
            if (ok)
            {
                const double l11 = sqrt(d1), l21 = (a21 - l20 * l10) / l11;
                const double d2 = a22 - l20 * l20 - l21 * l21;
                ok              = d2 > 0.0 && score_finite(d2);
                if (ok)
                {
                    const double l22 = sqrt(d2);
                    const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / l11, y2 = (e2 - l20 * y0 - l21 * y1) / l22;
                    nees = y0 * y0 + y1 * y1 + y2 * y2;
                    ok   = score_finite(nees);
                }
            }
        }
    }
    const double err2 = e0 * e0 + e1 * e1;
    double*      t    = totals + i * CSLAM_SCORE_FIELDS;
    if (ok)
    {
        t[CSLAM_SCORE_POSE_N] += 1.0;
        t[CSLAM_SCORE_POSE_IN] += nees <= gate ? 1.0 : 0.0;
        t[CSLAM_SCORE_POSE_ERR2] += err2;
        t[CSLAM_SCORE_POSE_EPHI2] += e2 * e2;
        t[CSLAM_SCORE_POSE_NEES] += nees;
    }
    else
    {
        t[CSLAM_SCORE_POSE_BAD] += 1.0;
    }
    t[CSLAM_SCORE_LM_N] += lm[0];
    t[CSLAM_SCORE_LM_BAD] += lm[1];
    t[CSLAM_SCORE_LM_IN] += lm[2];
    t[CSLAM_SCORE_LM_ERR2] += lm[3];
    t[CSLAM_SCORE_LM_NEES] += lm[4];
    if (record >= 0)
    {
        const float nan = __builtin_nanf("");
        float*      s   = series + ((size_t)record * instances + i) * 4;
        s[0]            = ok ? (float)err2 : nan;
        s[1]            = ok ? (float)nees : nan;
        s[2]            = lm[0] > 0.0 ? (float)(lm[3] / lm[0]) : nan;
        s[3]            = lm[0] > 0.0 ? (float)(lm[4] / lm[0]) : nan;
    }
}

// cslam_ekf_batch_score_scan: the generator's map LM [nlm][2] and association table (tag t -> state feature table[t - 1],
// 0: not seen yet) into the truth rows lo < p <= hi.  A position is assigned once and never changes, so rows at or
// below lo (filled by an earlier call) are left alone.  One lane per tag; each row has at most one writer.
__global__ void __launch_bounds__(256) ekf_score_gather_truth(const float* __restrict__ LM, const int* __restrict__ table,
                                                              int nlm, int lo, int hi, float* __restrict__ truth)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nlm)
    {
        return;
    }
    const int p = table[t];
    if (p > lo && p <= hi)
    {
        truth[2 * (p - 1)]     = LM[2 * t];
        truth[2 * (p - 1) + 1] = LM[2 * t + 1];
    }
}

#endif // CSLAM_SCORE_SINGLE_ONLY

// ------------------------------------------------------------------------------------------------
// The single filter (cslam_ekf_score, both dtypes): the same two launches with one instance, the single handle's
// storage switch and sign words, truth rows in f64, and two additions -- a sixth partial, p00 + p11 of EVERY landmark of
// the state (the map's share of trace(P), read from the deferred form), and a track record per call.
//   ekf_score_landmarks<T>  grid ceil(nl / 256), nl = (n - 3) / 2: one lane per landmark of the state.  Lanes below
//                           count = min(nl, truth rows) score their landmark by the batch kernel's rules and arithmetic;
//                           every lane below nl adds its two diagonal entries.  Slots [blocks][6].
//   ekf_score_finish<T>     one workgroup, lane 0: adds the slots in block order, scores the pose, updates the totals,
//                           writes the series record (4 f32) and the track record (5 f64: X[0], X[1], X[2], trace(P), n).
// ------------------------------------------------------------------------------------------------
constexpr int kScorePartsSingle = 6; // the five of kScoreParts, then sum p00 + p11 over every landmark of the state
constexpr int kScoreTrack       = 5; // doubles per track record

// truth [count][2] doubles: the true position of state feature j + 1, count <= nl; sgn: the sign words of the pending
// region (null: no heading column with S < 0 is pending)
template <typename T>
__global__ void __launch_bounds__(256) ekf_score_landmarks(const T* __restrict__ X, const T* __restrict__ Pv,
                                                           const T* __restrict__ P, int ldp, int lower,
                                                           const T* __restrict__ W, int kp, const int* __restrict__ sgn,
                                                           int nl, int count, const double* __restrict__ truth, double gate,
                                                           double* __restrict__ parts)
{
    __shared__ double s_part[4][kScorePartsSingle];
    const int         j = blockIdx.x * 256 + threadIdx.x;
    double            v[kScorePartsSingle] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < nl)
    {
        T x[2], pll[4];
        landmark_read_body<T>(X, Pv, P, ldp, lower, W, ldp, kp, sgn, 1 + j, 0, x, pll, nullptr);
        const double p00 = pll[0], p10 = pll[1], p11 = pll[3];
        v[5]             = p00 + p11;
        if (j < count)
        {
            const double e0 = (double)x[0] - truth[2 * (size_t)j], e1 = (double)x[1] - truth[2 * (size_t)j + 1];
            const double det  = p00 * p11 - p10 * p10;
            const double nees = (p11 * e0 * e0 - 2.0 * p10 * e0 * e1 + p00 * e1 * e1) / det;
            const double err2 = e0 * e0 + e1 * e1;
            const bool   ok   = score_finite(e0) && score_finite(e1) && score_finite(p00) && score_finite(p10) &&
                            score_finite(p11) && p00 > 0.0 && det > 0.0 && score_finite(nees);
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
    }
    // fixed order: the shuffle tree of a wave, then waves 0..3 (every lane takes part; lanes past nl hold zeros)
    for (int q = 0; q < kScorePartsSingle; q++)
    {
        for (int off = 32; off > 0; off >>= 1)
        {
            v[q] += __shfl_down(v[q], off, 64);
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
    {
        for (int q = 0; q < kScorePartsSingle; q++)
        {
            s_part[wave][q] = v[q];
        }
    }
    __syncthreads();
    if (threadIdx.x < kScorePartsSingle)
    {
        const int q = threadIdx.x;
        parts[(size_t)blockIdx.x * kScorePartsSingle + q] = ((s_part[0][q] + s_part[1][q]) + s_part[2][q]) + s_part[3][q];
    }
}

// blocks: the slots ekf_score_landmarks has just written (0: the state holds no landmark, or with_map == 0).  with_map
// == 0: the landmark totals are left alone and the track's trace is NaN.  record: the index of this call's series / track
// record, < 0 when they are full or absent.  totals [CSLAM_SCORE_FIELDS], series [capacity][4], track
// [capacity][kScoreTrack].
template <typename T>
__global__ void __launch_bounds__(64) ekf_score_finish(const T* __restrict__ X, const T* __restrict__ Pv, int ldp, int n,
                                                       const double* __restrict__ parts, int blocks, int with_map, double xt,
                                                       double yt, double pt, double gate, double* __restrict__ totals,
                                                       float* __restrict__ series, double* __restrict__ track,
                                                       long long record)
{
    if (threadIdx.x != 0)
    {
        return;
    }
    const size_t L = (size_t)ldp;
    double       lm[kScorePartsSingle] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < blocks; b++)
    {
        const double* p = parts + (size_t)b * kScorePartsSingle;
        for (int q = 0; q < kScorePartsSingle; q++)
        {
            lm[q] += p[q];
        }
    }
    // the pose: e = (x - xt, y - yt, wrap(phi - phit)); the lower triangle of the stripe block, P[r, c] = Pv[c ldp + r]
    const double e0 = (double)X[0] - xt, e1 = (double)X[1] - yt;
    const double e2 = score_wrap((double)X[2] - pt);
    const double a00 = Pv[0], a10 = Pv[1], a20 = Pv[2], a11 = Pv[L + 1], a21 = Pv[L + 2], a22 = Pv[2 * L + 2];
    bool         ok = score_finite(e0) && score_finite(e1) && score_finite(e2) && score_finite(a00) && score_finite(a10) &&
              score_finite(a20) && score_finite(a11) && score_finite(a21) && score_finite(a22);
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
            ok              = d1 > 0.0 && score_finite(d1);
            if (ok)
            {
                const double l11 = sqrt(d1), l21 = (a21 - l20 * l10) / l11;
                const double d2 = a22 - l20 * l20 - l21 * l21;
                ok              = d2 > 0.0 && score_finite(d2);
                if (ok)
                {
                    const double l22 = sqrt(d2);
                    const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / l11, y2 = (e2 - l20 * y0 - l21 * y1) / l22;
                    nees = y0 * y0 + y1 * y1 + y2 * y2;
                    ok   = score_finite(nees);
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
    if (with_map)
    {
        totals[CSLAM_SCORE_LM_N] += lm[0];
        totals[CSLAM_SCORE_LM_BAD] += lm[1];
        totals[CSLAM_SCORE_LM_IN] += lm[2];
        totals[CSLAM_SCORE_LM_ERR2] += lm[3];
        totals[CSLAM_SCORE_LM_NEES] += lm[4];
    }
    if (record >= 0)
    {
        const size_t r   = (size_t)record;
        const float  nan = __builtin_nanf("");
        float*       s   = series + r * 4;
        s[0]             = ok ? (float)err2 : nan;
        s[1]             = ok ? (float)nees : nan;
        s[2]             = lm[0] > 0.0 ? (float)(lm[3] / lm[0]) : nan;
        s[3]             = lm[0] > 0.0 ? (float)(lm[4] / lm[0]) : nan;
        double* t        = track + r * kScoreTrack;
        t[0]             = (double)X[0];
        t[1]             = (double)X[1];
        t[2]             = (double)X[2];
        t[3]             = with_map ? ((a00 + a11) + a22) + lm[5] : __builtin_nan("");
        t[4]             = (double)n;
    }
}

} // namespace cslam
