// pf_new_feature_kernels.hpp -- gfx950 kernels of the FastSLAM-2 scan that observes ONLY new features
// (test/main.cpp:314-328): every particle's pose is drawn from its own Gaussian, X <- X + chol(P) z
// (multivariateNormalGaussianDistribution, slam.h:753-764, with choleskyDecomposition, slam.h:413-436), P <- 0, and the
// new features are initialised at the SAMPLED pose (PF::addOneNewFeature, PF.cpp:9-60).  The weights are not touched:
// the reference does not reweight in this branch.
//
// One lane owns one particle, 64-lane workgroups (wave64), the layout and helpers of pf_kernels.hpp.  The fused kernel
// loops over the q new features inside the lane that sampled the pose: the grid of pf_add_features_kernel (particle x
// observation) cannot serve here, because the lanes of its other rows would read xv / pv while row 0 overwrites them.
// In both kernels a lane reads and writes only its own particle's columns, and every load of the pose comes before the
// first store: no lane of a launch reads pose memory that another lane of the same launch writes.
#pragma once

#include <hip/hip_runtime.h>

#include "pf_kernels.hpp"

namespace cslam
{

// XS = chol(P) z + X for one particle, in registers: the tail of pf_sample_proposal_kernel (chol_decomp, then
// mm<T, 3, 3, 1>(L, z), then + X, in that order).  Contraction is off here whatever the including file says, so that every
// kernel that inlines it rounds alike: the fused and the unfused form give the same bits.
template <typename T>
__device__ inline void pf_sample_pose_state(const T* X, const T* P, const T* z, T* XS)
{
#pragma clang fp contract(off)
    T L[9];
    chol_decomp<T, 3>(P, L);
    mm<T, 3, 3, 1>(L, z, XS);
#pragma unroll
    for (int e = 0; e < 3; e++)
    {
        XS[e] = XS[e] + X[e];
    }
}

// xv[3], pv[9] of particle p and its normals z[3] (component-major: normals[e * np + p], as the proposal reads them)
template <typename T>
__device__ inline void pf_load_pose_and_normals(const PfStore<T>& s, int p, const T* __restrict__ normals, T* X, T* P, T* z)
{
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
    for (int e = 0; e < 3; e++)
    {
        z[e] = normals[(size_t)e * s.np + p];
    }
}

// xv <- XS, pv <- nine exact zeros
template <typename T>
__device__ inline void pf_store_sampled_pose(const PfStore<T>& s, int p, const T* XS)
{
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        s.pv[(size_t)i * s.np + p] = (T)0;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        s.xv[(size_t)i * s.np + p] = XS[i];
    }
}

// ---------------------------------------------------------------- test/main.cpp:321-324; one lane per particle
template <typename T>
__global__ void __launch_bounds__(64) pf_sample_pose_kernel(PfStore<T> s, const T* __restrict__ normals)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= s.np)
    {
        return;
    }
    T X[3], P[9], z[3], XS[3];
    pf_load_pose_and_normals<T>(s, p, normals, X, P, z);
    pf_sample_pose_state<T>(X, P, z, XS);
    pf_store_sampled_pose<T>(s, p, XS);
}

// ---------------------------------------------------------------- test/main.cpp:314-328 in one launch
// [pred.on (kernel-uniform): PF::predict, PF.cpp:419-471, applied to the loaded pose exactly as
// pf_sample_proposal_kernel applies it; the predicted values never go to memory] -> sample the pose, zero Pv, store xv
// -> features s.nf .. s.nf + q - 1 from the sampled pose, with the expressions of pf_add_features_kernel (PF.cpp:9-60).
// The caller has checked s.nf + q <= the store's feature capacity.  Z: 2 x q, column-major, in device memory.
template <typename T>
__global__ void __launch_bounds__(64) pf_new_feature_step_kernel(PfStore<T> s, const T* __restrict__ Z, int q, T r00,
                                                                  T r10, T r01, T r11, const T* __restrict__ normals,
                                                                  PfPredict<T> pred)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= s.np)
    {
        return;
    }
    const T R[4] = {r00, r10, r01, r11};
    T       X[3], P[9], z[3], XS[3];
    pf_load_pose_and_normals<T>(s, p, normals, X, P, z);
    if (pred.on) // (kernel-uniform)
    {
        const T Q[4] = {pred.q00, pred.q10, pred.q01, pred.q11};
        pf_predict_state<T>(X, P, pred.v, pred.swa, Q, pred.wb, pred.dt);
    }
    pf_sample_pose_state<T>(X, P, z, XS);
    pf_store_sampled_pose<T>(s, p, XS);
    const T x = XS[0], y = XS[1], phi = XS[2];
    for (int i = 0; i < q; i++)
    {
        T         r = Z[2 * i], b = Z[2 * i + 1];
        T         sn = dsin(phi + b), cs = dcos(phi + b);
        const int f = s.nf + i;
        s.xf[((size_t)f * 2 + 0) * s.np + p] = x + (r * cs);
        s.xf[((size_t)f * 2 + 1) * s.np + p] = y + (r * sn);
        T Gz[4] = {cs, sn, -r * sn, r * cs};
        T GzR[4], Gzt[4], out[4];
        mm<T, 2, 2, 2>(Gz, R, GzR);
        tr<T, 2, 2>(Gz, Gzt);
        mm<T, 2, 2, 2>(GzR, Gzt, out);
#pragma unroll
        for (int e = 0; e < 4; e++)
        {
            s.pf[((size_t)f * 4 + e) * s.np + p] = out[e];
        }
    }
}

} // namespace cslam
