// ekf_assoc_deferred_kernels.hpp -- gated nearest-neighbour data association of the single-filter handle
// (cslam_ekf_associate_deferred; EKF.cpp:131-144 computeAssociation, EKF.cpp:235-326 dataAssociate) read from the
// deferred form of the covariance WITHOUT applying it:
//     P = Ps - Wp diag(s) Wp^T   over the kp pending columns of the current region (see ekf_landmark_kernels.hpp).
// Of the 5 x 5 block of P that H_j touches, the pose rows and the pose-landmark entries live in the stripe Pv, which is
// always current; only the landmark's 2 x 2 block needs the rank-kp correction, and landmark_read_body computes it.
//
// Two launches.
//   ekf_assoc_pair_kernel    : one lane per feature, 256 per workgroup.  The lane keeps its feature (inv(S), log det S,
//                              the predicted observation) in registers -- in the operation order of
//                              ekf_assoc_feature_kernel -- and loops over the observations, staged in LDS kAdObsChunk at
//                              a time.  Per observation the workgroup reduces (a) the smallest gated non-NaN nd with the
//                              lowest feature index that holds it and (b) the smallest nis over all its features, and
//                              writes ONE partial per (observation, workgroup).  No per-feature scratch in HBM, no
//                              serial walk over the features.
//   ekf_assoc_resolve_kernel : one workgroup.  Per observation it combines the partials in workgroup order (a strict `<`
//                              keeps the lower index on equal nd), decides kind, and compacts ZF / idf_f / ZN with a
//                              block-wide exclusive scan in observation order (as sim_associate_table_body does).
//
// Why the parallel form gives the sequential loop's answer.  The reference walks the features j = 1, 2, ... with
//     if (nis_j < gate1 && nd_j < nbest) { nbest = nd_j; jbest = j; } else if (nis_j < outer) outer = nis_j;
// from nbest = outer = +inf, jbest = 0.
//   * nbest only ever decreases and takes exactly the values of gated features; a NaN nd never passes `nd < nbest`, an
//     nd of +inf never passes it either (nbest <= +inf).  So at the end nbest is the minimum of nd over the gated
//     features with a comparable nd, and jbest is the FIRST feature that reached that minimum (a later equal one fails
//     the strict test), or 0 when that minimum is not below +inf.  A minimum with the lowest index is associative: the
//     per-wave, per-workgroup and cross-workgroup steps below each keep (smaller nd, then lower index).
//   * `outer` decides the answer only when jbest == 0, that is when NO feature set a record.  Then every feature went
//     through the else branch, none was excluded, and outer is the plain minimum of nis over all features, with a NaN
//     never the smaller one.  (When some feature did set a record, the reference's outer misses those features -- and
//     is not looked at.)
// tests/test_assoc_deferred_cpu.py proves the decomposed rule against the sequential one, with negative controls.
#pragma once

#include <hip/hip_runtime.h>

#include "ekf_kernels.hpp"
#include "ekf_landmark_kernels.hpp"
#include "sim_kernels.hpp"

namespace cslam
{

constexpr int kAdObsChunk = 128; // observations staged in LDS per pass of the pair kernel (2 * 128 = one scalar per lane)

// What the pair loop needs of feature j (0-based): ekf_assoc_feature_kernel's eight scalars, kept in registers.  A sibling
// of that kernel's body (which stays as it is): the same operation order, with the landmark's own 2 x 2 block taken from
// the deferred form.
template <typename T>
struct AdFeature
{
    T i00, i10, i01, i11, logdet, zr, zb;
};

template <typename T>
__device__ inline AdFeature<T> ad_feature(const T* __restrict__ X, const T* __restrict__ P, const T* __restrict__ Pv, int ldp,
                                          int n, T r00, T r10, T r01, T r11, int lower, const T* __restrict__ W, int ldw,
                                          int kp, const int* __restrict__ sgn, int j)
{
    T   coef[10], v[2];
    int fx;
    observe_model<T>(X, n, j + 1, (T)0, (T)0, coef, v, &fx);
    const T dx = X[fx] - X[0], dy = X[fx + 1] - X[1];
    const T zr = dsqrt(dx * dx + dy * dy);
    const T zb = datan2(dy, dx) - X[2];
    const int idx[5] = {0, 1, 2, fx, fx + 1};
    // the landmark's block under the pending columns: {p00, p10, p10, p11}
    T blk[4];
    landmark_read_body<T>(X, Pv, P, ldp, lower, W, ldw, kp, sgn, j + 1, 0, (T*)nullptr, blk, (T*)nullptr);
    T HP[2][5];
#pragma unroll
    for (int c = 0; c < 5; c++)
    {
        T p[5];
#pragma unroll
        for (int l = 0; l < 5; l++)
        {
            // (l < 3 or c < 3: the stripe)
            p[l] = (l >= 3 && c >= 3) ? blk[2 * (c - 3) + (l - 3)] : p_get<T>(P, Pv, ldp, idx[l], idx[c], lower);
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
        {
            T sm = coef[5 * r + 0] * p[0];
            sm += coef[5 * r + 1] * p[1];
            sm += coef[5 * r + 2] * p[2];
            sm += coef[5 * r + 3] * p[3];
            sm += coef[5 * r + 4] * p[4];
            HP[r][c] = sm;
        }
    }
    T       S[2][2];
    const T R[2][2] = {{r00, r01}, {r10, r11}};
#pragma unroll
    for (int c = 0; c < 2; c++)
    {
#pragma unroll
        for (int r = 0; r < 2; r++)
        {
            T sm = HP[r][0] * coef[5 * c + 0];
            sm += HP[r][1] * coef[5 * c + 1];
            sm += HP[r][2] * coef[5 * c + 2];
            sm += HP[r][3] * coef[5 * c + 3];
            sm += HP[r][4] * coef[5 * c + 4];
            S[r][c] = sm + R[r][c];
        }
    }
    // partially pivoted LU of [[a b],[c d]]
    const T    a = S[0][0], b = S[0][1], c2 = S[1][0], d = S[1][1];
    const bool sw  = dabs(c2) > dabs(a);
    const T    u00 = sw ? c2 : a, u01 = sw ? d : b;
    const T    l10 = (sw ? a : c2) / u00;
    const T    u11 = (sw ? b : d) - l10 * u01;
    const T    det = sw ? -(u00 * u11) : (u00 * u11);
    T          inv[2][2];
#pragma unroll
    for (int c = 0; c < 2; c++)
    {
        T x0 = ((sw ? 1 : 0) == c) ? (T)1 : (T)0;
        T x1 = ((sw ? 0 : 1) == c) ? (T)1 : (T)0;
        x1 -= l10 * x0;
        x1        = x1 / u11;
        x0        = (x0 - u01 * x1) / u00;
        inv[0][c] = x0;
        inv[1][c] = x1;
    }
    return AdFeature<T>{inv[0][0], inv[1][0], inv[0][1], inv[1][1], dlog(det), zr, zb};
}

// grid.x = G = ceil(nf / 256) (nf >= 1).  Partials, observation-major: pnd / pj / pnis [m][G].
//   pnd[i][g]  smallest gated non-NaN nd of observation i among the features of workgroup g (+inf: none)
//   pj[i][g]   the lowest 1-based feature that holds it (0: none)
//   pnis[i][g] smallest nis of observation i among the features of workgroup g (a NaN is never the smaller; +inf: none)
template <typename T>
__global__ void __launch_bounds__(256) ekf_assoc_pair_kernel(const T* __restrict__ X, const T* __restrict__ P,
                                                              const T* __restrict__ Pv, int ldp, int n, T r00, T r10, T r01,
                                                              T r11, int lower, const T* __restrict__ W, int ldw, int kp,
                                                              const int* __restrict__ sgn, const T* __restrict__ Z, int m,
                                                              T gate1, T* __restrict__ pnd, int* __restrict__ pj,
                                                              T* __restrict__ pnis)
{
    __shared__ T   s_z[2 * kAdObsChunk];
    __shared__ T   s_nd[4][kAdObsChunk];
    __shared__ T   s_nis[4][kAdObsChunk];
    __shared__ int s_j[4][kAdObsChunk];
    const int  nf    = (n - 3) / 2;
    const int  tid   = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int  j     = blockIdx.x * 256 + tid; // 0-based feature
    const bool valid = j < nf;
    const T    inf   = (T)INFINITY;
    AdFeature<T> f{(T)0, (T)0, (T)0, (T)0, (T)0, (T)0, (T)0};
    if (valid)
    {
        f = ad_feature<T>(X, P, Pv, ldp, n, r00, r10, r01, r11, lower, W, ldw, kp, sgn, j);
    }
    for (int base = 0; base < m; base += kAdObsChunk)
    {
        const int cnt = (m - base < kAdObsChunk) ? (m - base) : kAdObsChunk;
        __syncthreads(); // (the previous pass has been read)
        if (tid < 2 * cnt)
        {
            s_z[tid] = Z[2 * (size_t)base + tid];
        }
        __syncthreads();
        for (int i = 0; i < cnt; i++)
        {
            const T    v0    = s_z[2 * i] - f.zr;
            const T    v1    = pi2pi<T>(s_z[2 * i + 1] - f.zb);
            const T    t0    = v0 * f.i00 + v1 * f.i10; // (V^T Sinv)[0]
            const T    t1    = v0 * f.i01 + v1 * f.i11;
            const T    nis   = t0 * v0 + t1 * v1;
            const T    nd    = nis + f.logdet;
            const bool gated = valid && (nis < gate1);
            const T    cand  = (gated && nd == nd) ? nd : inf;
            T          cmin  = cand;
            T          nmin  = (valid && nis == nis) ? nis : inf;
#pragma unroll
            for (int dlt = 32; dlt >= 1; dlt >>= 1)
            {
                const T oc = __shfl_xor(cmin, dlt);
                const T on = __shfl_xor(nmin, dlt);
                cmin       = (oc < cmin) ? oc : cmin;
                nmin       = (on < nmin) ? on : nmin;
            }
            const unsigned long long hits = __ballot(cand == cmin);
            if (lane == 0)
            {
                s_nd[wave][i]  = cmin;
                s_j[wave][i]   = (cmin < inf) ? (blockIdx.x * 256 + wave * 64 + __builtin_ctzll(hits) + 1) : 0;
                s_nis[wave][i] = nmin;
            }
        }
        __syncthreads();
        if (tid < cnt)
        {
            T   nb = inf, ob = inf;
            int jb = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) // in wave order: the strict `<` keeps the lower index on equal nd
            {
                const T c = s_nd[w][tid], o = s_nis[w][tid];
                if (c < nb)
                {
                    nb = c;
                    jb = s_j[w][tid];
                }
                ob = (o < ob) ? o : ob;
            }
            const size_t at = (size_t)(base + tid) * gridDim.x + blockIdx.x;
            pnd[at]         = nb;
            pj[at]          = jb;
            pnis[at]        = ob;
        }
    }
}

// One workgroup of kSimThreads.  G = 0 (an empty map): no partials are read, every observation is of kind 2.
// Outputs: idf_out[m] (1-based feature or 0), kind_out[m] (1 / 2 / 0), and the split in observation order -- ZF (2 x mf),
// idf_f (mf), ZN (2 x mn) -- with counts[3] = {mf, mn, dropped}.
template <typename T>
__global__ void __launch_bounds__(kSimThreads) ekf_assoc_resolve_kernel(const T* __restrict__ pnd, const int* __restrict__ pj,
                                                                        const T* __restrict__ pnis, int G,
                                                                        const T* __restrict__ Z, int m, T gate2,
                                                                        int* __restrict__ idf_out, int* __restrict__ kind_out,
                                                                        T* __restrict__ ZF, int* __restrict__ idf_f,
                                                                        T* __restrict__ ZN, int* __restrict__ counts)
{
    __shared__ int s_wave[kSimThreads / 64];
    const T        inf = (T)INFINITY;
    int            nknown = 0, nnew = 0;
    for (int base = 0; base < m; base += kSimThreads)
    {
        const int  i  = base + threadIdx.x;
        const bool in = i < m;
        T          nbest = inf, outer = inf;
        int        jbest = 0;
        if (in)
        {
            for (int g = 0; g < G; g++) // in workgroup order: the strict `<` keeps the lower index on equal nd
            {
                const size_t at = (size_t)i * G + g;
                const T      c = pnd[at], o = pnis[at];
                if (c < nbest)
                {
                    nbest = c;
                    jbest = pj[at];
                }
                outer = (o < outer) ? o : outer;
            }
        }
        const int  kind  = (jbest != 0) ? 1 : ((outer > gate2) ? 2 : 0);
        const bool known = in && kind == 1, fresh = in && kind == 2;
        int        tk, tn;
        const int  ok = block_exclusive_scan(known ? 1 : 0, s_wave, &tk);
        const int  on = block_exclusive_scan(fresh ? 1 : 0, s_wave, &tn);
        if (in)
        {
            idf_out[i]  = jbest;
            kind_out[i] = kind;
        }
        if (known)
        {
            const int o   = nknown + ok;
            ZF[2 * o]     = Z[2 * i];
            ZF[2 * o + 1] = Z[2 * i + 1];
            idf_f[o]      = jbest;
        }
        if (fresh)
        {
            const int o   = nnew + on;
            ZN[2 * o]     = Z[2 * i];
            ZN[2 * o + 1] = Z[2 * i + 1];
        }
        nknown += tk;
        nnew += tn;
    }
    if (threadIdx.x == 0)
    {
        counts[0] = nknown;
        counts[1] = nnew;
        counts[2] = m - nknown - nnew;
    }
}

} // namespace cslam
