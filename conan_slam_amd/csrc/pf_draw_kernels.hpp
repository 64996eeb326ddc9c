// pf_draw_kernels.hpp -- the particle filter's random inputs drawn on the device: the three proposal normals of every
// particle (slam.h:753-764, multivariateGauss) and the strata positions of the resample (PF.cpp:557, 579-596,
// stratifiedRandom), from the counter-based generator of conan_slam_amd/synth.py (counter_rng.hpp).
//
// Every draw is a pure function of (seed, step, stream, GLOBAL particle slot) -- synth.pf_draw_key:
//     key(step, e, g) = ((step * 4 + e) << 32) | g        e = 0, 1, 2: the proposal normals, e = 3: the strata uniform
// so a set sharded over ranks sees the noise of the unsharded set, and nobody distributes select[].
//
// ONE producer kernel writes the draws into the handle's staging area in the layout the consumers already read
// (Z | idf | normals | select); pf_sample_proposal_kernel, pf_sample_proposal_assoc_kernel, pf_feature_update_kernel,
// pf_resample_plan_kernel and pf_keep_kernel are launched behind it with the arguments they always get.
#pragma once

#include <hip/hip_runtime.h>

#include "counter_rng.hpp"

namespace cslam
{

constexpr int kPfDrawObsMax = 32; // observations that travel as kernel arguments (more: the staged copy carries them)

// Z (2 x m, column-major) and idf (or the use[] mask of the _assoc consumer) of one call, by value
template <typename T>
struct PfDrawObs
{
    T   z[2 * kPfDrawObsMax];
    int idf[kPfDrawObsMax];
};

__host__ __device__ inline unsigned long long pf_draw_key(unsigned long long step, unsigned long long e, unsigned long long g)
{
    return ((step * 4ull + e) << 32) | g;
}

// grid = ceil(max(np, n_sel, 2 m) / 256) x 256 lanes.
//   lane p < np      normals[e * np + p] = T(normal(seed, key(step, e, first + p))), e = 0..2     (np = 0: no normals)
//   lane i < n_sel   select[i] = di[i] + (T(u) * k - k / 2), u = uniform01(seed, 2 key(step, 3, i)) (n_sel = 0: none)
//                    di = k/2, +k, +k, ...: the running sum of stratified_random (pf.py), computed once on the host
//   lane j < 2 m     Z[j] = obs.z[j]; lane j < m: idf[j] = obs.idf[j]                               (m = 0: none)
// np, n_sel and m are kernel-uniform.  The strata arithmetic is numpy's: the product, the difference and the sum are
// rounded one by one in T.
template <typename T>
__global__ void __launch_bounds__(256) pf_stage_draw_kernel(unsigned long long seed, unsigned long long step,
                                                             unsigned long long first, T* __restrict__ normals, int np,
                                                             T* __restrict__ select, const T* __restrict__ di, int n_sel,
                                                             T k, T* __restrict__ Z, int* __restrict__ idf, int m,
                                                             PfDrawObs<T> obs)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * m)
    {
        Z[i] = obs.z[i];
        if (i < m)
        {
            idf[i] = obs.idf[i];
        }
    }
    if (i < np)
    {
        const unsigned long long g = first + (unsigned long long)i;
#pragma unroll
        for (int e = 0; e < 3; e++)
        {
            normals[(size_t)e * np + i] = (T)counter_normal(seed, pf_draw_key(step, (unsigned long long)e, g));
        }
    }
    if (i < n_sel)
    {
        const T u = (T)uniform01(seed, 2ull * pf_draw_key(step, 3ull, (unsigned long long)i));
        const T a = u * k;
        const T b = a - k / (T)2;
        select[i] = di[i] + b;
    }
}

} // namespace cslam
