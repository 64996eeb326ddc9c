// pf_assoc_kernels.hpp -- per-particle gated nearest-neighbour data association of the FastSLAM-2 store, and the
// consumers that read a per-particle correspondence table.
//
// The measure is the reference's computeAssociation (EKF.cpp:131-144) and the rule its dataAssociate (EKF.cpp:235-326),
// applied to ONE particle's own state.  A particle holds no pose-feature cross-covariance, so its P is
// blockdiag(Pv, PF_f) and
//     S = HV Pv HV^T + HF PF_f HF^T + R,   v = (z_r - ZP_r, pi2pi(z_b - ZP_b)),   nis = v^T S^-1 v,   nd = nis + log det S.
// S, its inverse and log det S depend on (particle, feature) only: they are formed once per feature and serve all the
// observations of the chunk.
//
//   pf_assoc_scan_kernel     one lane per particle (index fastest in the store: the six words of a feature coalesce over
//                            64 particles); blockIdx.y = a chunk of kPfAssocFeatChunk features, blockIdx.z = a chunk of
//                            kPfAssocObsChunk observations.  The running (nbest, jbest, outer) of the observation chunk
//                            live in registers; one partial per (feature chunk, observation, particle) goes to memory.
//   pf_assoc_merge_kernel    one lane per (particle, observation): partials in chunk order -> smallest gated nd with the
//                            lowest index on ties, smallest nis, kind.
//   pf_assoc_resolve_kernel  one lane per (particle, observation): among the observations of the particle that claim the
//                            same feature the smallest nd keeps it (lower observation index on equal nd); the others
//                            become idf = 0, kind = 0.
//   pf_assoc_summary_kernel  one workgroup per observation: weight mass by kind in double, fixed order.
//
// Tables: idf[m][np], kind[m][np] (particle index fastest), summary[m][4] = (sum w kind 1, kind 2, kind 0, count kind 1).
#pragma once

#include <hip/hip_runtime.h>

#include "pf_kernels.hpp"

#pragma clang fp contract(off)

namespace cslam
{

constexpr int kPfAssocFeatChunk = 32; // features per blockIdx.y of the scan
// Observations per blockIdx.z of the scan.  8: the chunk's state is 2 x 8 observation words, 8 nbest, 8 jbest, 8 outer
// next to the pose (3), Pv (9), R (4) and the live values of one feature's S / S^-1: the scan compiles to 90 VGPRs in
// f32 and 181 in f64, no scratch in either.  16 would halve the feature re-reads of m > 8 but takes f64 past 256 VGPRs.
constexpr int kPfAssocObsChunk = 8;

template <typename T>
__global__ void __launch_bounds__(64) pf_assoc_scan_kernel(PfStore<T> s, const T* __restrict__ Z, int m, T r00, T r10, T r01,
                                                            T r11, T gate1, T* __restrict__ part_nd,
                                                            int* __restrict__ part_j, T* __restrict__ part_nis)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= s.np)
    {
        return;
    }
    const int c  = blockIdx.y;
    const int f0 = c * kPfAssocFeatChunk;
    const int f1 = min(s.nf, f0 + kPfAssocFeatChunk);
    const int j0 = blockIdx.z * kPfAssocObsChunk;
    const T   R[4] = {r00, r10, r01, r11};
    const T   inf  = (T)INFINITY;
    T         X[3], Pv[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        X[i] = s.xv[(size_t)i * s.np + p];
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        Pv[i] = s.pv[(size_t)i * s.np + p];
    }
    T   z0[kPfAssocObsChunk], z1[kPfAssocObsChunk], nbest[kPfAssocObsChunk], outer[kPfAssocObsChunk];
    int jbest[kPfAssocObsChunk];
#pragma unroll
    for (int u = 0; u < kPfAssocObsChunk; u++)
    {
        const int j = min(j0 + u, m - 1); // (a slot beyond m repeats the last observation; it is not stored)
        z0[u]       = Z[2 * j];
        z1[u]       = Z[2 * j + 1];
        nbest[u]    = inf;
        outer[u]    = inf;
        jbest[u]    = 0;
    }
    for (int f = f0; f < f1; f++)
    {
        T xf[2], pf[4], ZP[2], HV[6], HF[4], SF[4];
        load_feature<T>(s, p, f, xf, pf);
        compute_jacobians<T>(X, xf, pf, R, ZP, HV, HF, SF); // SF = HF PF HF^T + R
        T HVP[6], HVt[6], SV[4], S[4], SI[4];
        mm<T, 2, 3, 3>(HV, Pv, HVP);
        tr<T, 2, 3>(HV, HVt);
        mm<T, 2, 3, 2>(HVP, HVt, SV);
#pragma unroll
        for (int e = 0; e < 4; e++)
        {
            S[e] = SV[e] + SF[e];
        }
        inverse_lu<T, 2>(S, SI);
        // det S with the sign of the partially pivoted LU (what Eigen's dynamic determinant() returns): S is column-major
        const bool sw  = dfabs(S[1]) > dfabs(S[0]);
        const T    u00 = sw ? S[1] : S[0], u01 = sw ? S[3] : S[2];
        const T    l10 = (sw ? S[0] : S[1]) / u00;
        const T    u11 = (sw ? S[2] : S[3]) - l10 * u01;
        const T    ld  = dlog(sw ? -(u00 * u11) : (u00 * u11));
#pragma unroll
        for (int u = 0; u < kPfAssocObsChunk; u++)
        {
            const T v0  = z0[u] - ZP[0];
            const T v1  = pi2pi<T>(z1[u] - ZP[1]);
            const T t0  = v0 * SI[0] + v1 * SI[1];
            const T t1  = v0 * SI[2] + v1 * SI[3];
            const T nis = t0 * v0 + t1 * v1;
            const T nd  = nis + ld;
            if (nis < gate1 && nd < nbest[u]) // (a NaN fails both)
            {
                nbest[u] = nd;
                jbest[u] = f + 1;
            }
            if (nis < outer[u])
            {
                outer[u] = nis;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kPfAssocObsChunk; u++)
    {
        const int j = j0 + u;
        if (j < m)
        {
            const size_t o = ((size_t)c * m + j) * s.np + p;
            part_nd[o]     = nbest[u];
            part_j[o]      = jbest[u];
            part_nis[o]    = outer[u];
        }
    }
}

// grid = (ceil(np/64), m).  nchunks = 0 (an empty map): nothing is inside a gate and outer = inf > gate2: kind 2.
template <typename T>
__global__ void __launch_bounds__(64) pf_assoc_merge_kernel(int np, int m, int nchunks, const T* __restrict__ part_nd,
                                                             const int* __restrict__ part_j,
                                                             const T* __restrict__ part_nis, T gate2,
                                                             int* __restrict__ raw_idf, int* __restrict__ raw_kind,
                                                             T* __restrict__ raw_nd)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y;
    if (p >= np || j >= m)
    {
        return;
    }
    const T inf   = (T)INFINITY;
    T       nbest = inf, outer = inf;
    int     jbest = 0;
    for (int c = 0; c < nchunks; c++) // ascending feature index: `<` keeps the lowest index among equal nd
    {
        const size_t o  = ((size_t)c * m + j) * np + p;
        const int    jj = part_j[o];
        const T      nd = part_nd[o], ns = part_nis[o];
        if (jj != 0 && nd < nbest)
        {
            nbest = nd;
            jbest = jj;
        }
        if (ns < outer)
        {
            outer = ns;
        }
    }
    const size_t o = (size_t)j * np + p;
    raw_idf[o]     = jbest;
    raw_kind[o]    = (jbest != 0) ? 1 : ((outer > gate2) ? 2 : 0);
    raw_nd[o]      = nbest;
}

// grid = (ceil(np/64), m)
template <typename T>
__global__ void __launch_bounds__(64) pf_assoc_resolve_kernel(int np, int m, const int* __restrict__ raw_idf,
                                                               const int* __restrict__ raw_kind,
                                                               const T* __restrict__ raw_nd, int* __restrict__ idf,
                                                               int* __restrict__ kind)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y;
    if (p >= np || j >= m)
    {
        return;
    }
    const size_t o    = (size_t)j * np + p;
    const int    mine = raw_idf[o];
    bool         lost = false;
    if (mine != 0)
    {
        const T nd = raw_nd[o];
        for (int k = 0; k < m; k++)
        {
            const size_t q = (size_t)k * np + p;
            if (k != j && raw_idf[q] == mine)
            {
                const T other = raw_nd[q];
                lost          = lost || other < nd || (other == nd && k < j);
            }
        }
    }
    idf[o]  = lost ? 0 : mine;
    kind[o] = lost ? 0 : raw_kind[o];
}

// summary[j] = (sum w kind 1, sum w kind 2, sum w kind 0, particles of kind 1), in double and in the fixed order of
// pf_weight_sums_kernel.  grid = m, one workgroup per observation.
template <typename T>
__global__ void __launch_bounds__(256) pf_assoc_summary_kernel(const T* __restrict__ w, int np, const int* __restrict__ kind,
                                                                double* __restrict__ summary)
{
    __shared__ double sm[4][256];
    const int         j = blockIdx.x;
    double            a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < np; i += 256)
    {
        const int    k = kind[(size_t)j * np + i];
        const double x = (double)w[i];
        a[0] += (k == 1) ? x : 0.0;
        a[1] += (k == 2) ? x : 0.0;
        a[2] += (k == 0) ? x : 0.0;
        a[3] += (k == 1) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
    {
        sm[e][threadIdx.x] = a[e];
    }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1)
    {
        if ((int)threadIdx.x < st)
        {
#pragma unroll
            for (int e = 0; e < 4; e++)
            {
                sm[e][threadIdx.x] += sm[e][threadIdx.x + st];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 4)
    {
        summary[(size_t)j * 4 + threadIdx.x] = sm[threadIdx.x][0];
    }
}

// ---------------------------------------------------------------- consumers with a per-particle table
// PF::sampleProposal (PF.cpp:502-544) with PF::featureUpdate (PF.cpp:222-277) riding along, as
// pf_sample_proposal_kernel with fu_mode != 0 and no predict, but every particle reads ITS OWN correspondence
// tab[j * np + p] (1-based, 0 = none) and the observation mask use[j]:
//   use[j] = 0             the observation does not exist for any particle;
//   use[j] = 1, tab != 0   the arithmetic of pf_sample_proposal_kernel in its order;
//   use[j] = 1, tab == 0   no pose or feature update; the likelihood product takes the factor `miss` at j's place.
// fu_mode: 1 the reference's gain, 2 the textbook one (never 0: a particle's matched features are distinct after
// pf_assoc_resolve_kernel, so the fused feature update has no write conflict).
template <typename T>
__global__ void __launch_bounds__(64) pf_sample_proposal_assoc_kernel(PfStore<T> s, const T* __restrict__ Z,
                                                                       const int* __restrict__ tab,
                                                                       const int* __restrict__ use, int m, T r00, T r10,
                                                                       T r01, T r11, const T* __restrict__ normals,
                                                                       T miss, int fu_mode)
{
    const int gl  = blockIdx.x * 64 + threadIdx.x;
    const int p   = gl / kPfSubLanes;
    const int sub = threadIdx.x & (kPfSubLanes - 1);
    if (p >= s.np)
    {
        return;
    }
    const T R[4] = {r00, r10, r01, r11};
    T       X[3], P[9], X0[3], P0[9], PX[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        X[i] = s.xv[(size_t)i * s.np + p];
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        P[i] = s.pv[(size_t)i * s.np + p];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        X0[i] = X[i];
        PX[i] = X[i];
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        P0[i] = P[i];
    }
    constexpr int kObsChunk = kPfSubLanes;
    T             xfc[kObsChunk][2], pfc[kObsChunk][4];
    int           fc[kObsChunk]; // 0-based feature of the chunk's observations for this particle, -1 = not matched / unused
    for (int base = 0; base < m; base += kObsChunk)
    {
#pragma unroll
        for (int j = 0; j < kObsChunk; j++)
        {
            const int i = min(base + j, m - 1);
            const int f = (base + j < m && use[i] != 0) ? tab[(size_t)i * s.np + p] - 1 : -1;
            fc[j]       = f;
            load_feature<T>(s, p, max(f, 0), xfc[j], pfc[j]); // (unconditional, as in pf_sample_proposal_kernel)
        }
#pragma unroll
        for (int j = 0; j < kObsChunk; j++)
        {
            const int i = base + j;
            if (fc[j] < 0)
            {
                continue;
            }
            T xf[2] = {xfc[j][0], xfc[j][1]}, pf[4] = {pfc[j][0], pfc[j][1], pfc[j][2], pfc[j][3]};
            T ZP[2], HV[6], HF[4], SF[4], SFI[4], VI[2];
            compute_jacobians<T>(PX, xf, pf, R, ZP, HV, HF, SF);
            inverse_lu<T, 2>(SF, SFI);
            VI[0] = Z[2 * i] - ZP[0];
            VI[1] = pi2pi<T>(Z[2 * i + 1] - ZP[1]);
            T HVt[6], t32[6], t33[9], Pinv[9], PT[9];
            tr<T, 2, 3>(HV, HVt);
            mm<T, 3, 2, 2>(HVt, SFI, t32);
            mm<T, 3, 2, 3>(t32, HV, t33);
            inverse_lu<T, 3>(P, Pinv);
#pragma unroll
            for (int e = 0; e < 9; e++)
            {
                PT[e] = t33[e] + Pinv[e];
            }
            inverse_lu<T, 3>(PT, P);
            T a32[6], b32[6], dx[3];
            mm<T, 3, 3, 2>(P, HVt, a32);
            mm<T, 3, 2, 2>(a32, SFI, b32);
            mm<T, 3, 2, 1>(b32, VI, dx);
#pragma unroll
            for (int e = 0; e < 3; e++)
            {
                X[e]  = X[e] + dx[e];
                PX[e] = X[e];
            }
        }
    }
    T L[9], XS[3], z[3];
#pragma unroll
    for (int e = 0; e < 3; e++)
    {
        z[e] = normals[(size_t)e * s.np + p];
    }
    chol_decomp<T, 3>(P, L);
    mm<T, 3, 3, 1>(L, z, XS);
#pragma unroll
    for (int e = 0; e < 3; e++)
    {
        XS[e] = XS[e] + X[e];
    }
    // likelihood at the sampled pose (PF.cpp:343-359): sub-lane j evaluates observation base + j
    T like = (T)1;
    for (int base = 0; base < m; base += kObsChunk)
    {
        const int i = min(base + sub, m - 1);
        const int f = (base + sub < m && use[i] != 0) ? tab[(size_t)i * s.np + p] - 1 : -1;
        T         lf = miss;
        if (f >= 0)
        {
            T xf[2], pf[4], ZP[2], HV[6], HF[4], SF[4], V[2];
            load_feature<T>(s, p, f, xf, pf);
            compute_jacobians<T>(XS, xf, pf, R, ZP, HV, HF, SF);
            V[0] = Z[2 * i] - ZP[0];
            V[1] = pi2pi<T>(Z[2 * i + 1] - ZP[1]);
            lf   = gauss_evaluate<T, 2>(V, SF);
            T xn[2], pn[4];
            pf_feature_kf<T>(xf, pf, HF, V, R, fu_mode == 2 ? 1 : 0, xn, pn);
            s.xf[((size_t)f * 2 + 0) * s.np + p] = xn[0];
            s.xf[((size_t)f * 2 + 1) * s.np + p] = xn[1];
#pragma unroll
            for (int e = 0; e < 4; e++)
            {
                s.pf[((size_t)f * 4 + e) * s.np + p] = pn[e];
            }
        }
        const int lane0 = (int)(threadIdx.x & ~(kPfSubLanes - 1));
#pragma unroll
        for (int j = 0; j < kObsChunk; j++)
        {
            const T lj = __shfl(lf, lane0 + j);
            if (base + j < m && use[base + j] != 0)
            {
                like = like * lj; // the reference's order: ((1 * l0) * l1) * ...; an unmatched observation's factor is `miss`
            }
        }
    }
    T d1[3] = {X0[0] - XS[0], X0[1] - XS[1], pi2pi<T>(X0[2] - XS[2])};
    T d2[3] = {X[0] - XS[0], X[1] - XS[1], pi2pi<T>(X[2] - XS[2])};
    T prior = gauss_evaluate<T, 3>(d1, P0);
    T prop  = gauss_evaluate<T, 3>(d2, P);
    if (sub != 0)
    {
        return;
    }
    T w    = s.w[p];
    s.w[p] = w * like * prior / prop;
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        s.xv[(size_t)i * s.np + p] = XS[i];
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        s.pv[(size_t)i * s.np + p] = (T)0; // PF.cpp:537
    }
}

// PF::featureUpdate (PF.cpp:222-277) alone, as pf_feature_update_kernel, from the per-particle table and the mask
template <typename T>
__global__ void __launch_bounds__(64) pf_feature_update_assoc_kernel(PfStore<T> s, const T* __restrict__ Z,
                                                                      const int* __restrict__ tab,
                                                                      const int* __restrict__ use, int m, T r00, T r10,
                                                                      T r01, T r11, int textbook)
{
    int p = blockIdx.x * 64 + threadIdx.x;
    int i = blockIdx.y;
    if (p >= s.np || i >= m || use[i] == 0)
    {
        return;
    }
    const int f = tab[(size_t)i * s.np + p] - 1;
    if (f < 0)
    {
        return;
    }
    const T R[4] = {r00, r10, r01, r11};
    T       X[3], xf[2], pf[4], ZP[2], HV[6], HF[4], SF[4], V[2];
#pragma unroll
    for (int e = 0; e < 3; e++)
    {
        X[e] = s.xv[(size_t)e * s.np + p];
    }
    load_feature<T>(s, p, f, xf, pf);
    compute_jacobians<T>(X, xf, pf, R, ZP, HV, HF, SF);
    V[0] = Z[2 * i] - ZP[0];
    V[1] = pi2pi<T>(Z[2 * i + 1] - ZP[1]);
    T xn[2], pn[4];
    pf_feature_kf<T>(xf, pf, HF, V, R, textbook, xn, pn);
    s.xf[((size_t)f * 2 + 0) * s.np + p] = xn[0];
    s.xf[((size_t)f * 2 + 1) * s.np + p] = xn[1];
#pragma unroll
    for (int e = 0; e < 4; e++)
    {
        s.pf[((size_t)f * 4 + e) * s.np + p] = pn[e];
    }
}

} // namespace cslam
