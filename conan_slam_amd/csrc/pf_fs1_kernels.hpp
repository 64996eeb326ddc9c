// pf_fs1_kernels.hpp -- gfx950 kernels of the FastSLAM-1.0 step of the particle handle (the sibling of the FastSLAM-2
// loop that the reference declares a switch for, mSwitchSampleProposal, slam.h:102, and never reads):
//   sample the motion per particle   addControlNoise (slam.h:149-159) per particle, then PF::predict (PF.cpp:419-471)
//   weight by the observation likelihood   PF::likelihood (PF.cpp:343-359) at the particle's own pose
//   update the features              PF::featureUpdate (PF.cpp:222-277)
// The resample (PF.cpp:473-500) and the new features (PF.cpp:9-60) are those of the FastSLAM-2 path.  Nothing here
// inverts Pv.
//
// The control draws are a second stream, independent of the proposal / strata stream of pf_draw_kernels.hpp: the same
// keys (pf_draw_key) under another seed, pf_control_seed(seed) = splitmix64(seed, 0x4354524C):
//     normal(control step t, component c, global slot g) = T(counter_normal(pf_control_seed(seed), key(t, c, g)))
// c = 0: velocity, c = 1: steering.  synth.pf_control_normals / pf_control_noise restate them.
#pragma once

#include <hip/hip_runtime.h>

#include "counter_rng.hpp"
#include "pf_control_kernels.hpp"
#include "pf_draw_kernels.hpp"
#include "pf_kernels.hpp"

#pragma clang fp contract(off)

namespace cslam
{

constexpr unsigned long long kPfControlStream = 0x4354524Cull; // "CTRL"

__host__ __device__ inline unsigned long long pf_control_seed(unsigned long long seed)
{
    return splitmix64(seed, kPfControlStream);
}

// what the sampled run needs beside the controls: the control stream's seed, the control step of the launch's step 0,
// the global slot of particle 0, and the standard deviations sqrt(Q00), sqrt(Q11) in T
template <typename T>
struct PfControlNoise
{
    unsigned long long cseed, step0, first;
    T                  s0, s1;
};

template <typename T>
__device__ inline T pf_control_normal(unsigned long long cseed, unsigned long long step, unsigned long long c,
                                      unsigned long long g)
{
    return (T)counter_normal(cseed, pf_draw_key(step, c, g));
}

// out[c * np + p] = the normal of (step, c, first + p), c = 0, 1: what cslam_pf_get_control_draws brings back
template <typename T>
__global__ void __launch_bounds__(256) pf_control_draws_kernel(unsigned long long cseed, unsigned long long step,
                                                                unsigned long long first, T* __restrict__ out, int np)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= np)
    {
        return;
    }
    const unsigned long long g = first + (unsigned long long)p;
    out[p]                     = pf_control_normal<T>(cseed, step, 0ull, g);
    out[(size_t)np + p]        = pf_control_normal<T>(cseed, step, 1ull, g);
}

// pf_control_run_kernel with the controls of every particle drawn: step j of the launch uses
//     vn = v[j] + n0 * s0,  swan = swa[j] + n1 * s1       (slam.h:149-159 with a diagonal Q; product, then sum, in T)
// Same grid, one lane per particle; pose and Pv loaded once, stored once.
template <typename T>
__global__ void __launch_bounds__(64) pf_control_run_sampled_kernel(PfStore<T> s, int k, PfControls<T> c,
                                                                    PfControlNoise<T> nz, T q00, T q10, T q01, T q11,
                                                                    T wb, T dt, int use_heading, T Rphi)
{
    int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= s.np)
    {
        return;
    }
    const unsigned long long g = nz.first + (unsigned long long)p;
    T X[3], P[9], Q[4] = {q00, q10, q01, q11};
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
#pragma unroll 1
    for (int j = 0; j < k; j++)
    {
        const unsigned long long t  = nz.step0 + (unsigned long long)j;
        const T                  n0 = pf_control_normal<T>(nz.cseed, t, 0ull, g);
        const T                  n1 = pf_control_normal<T>(nz.cseed, t, 1ull, g);
        const T                  a0 = n0 * nz.s0;
        const T                  a1 = n1 * nz.s1;
        const T                  vn = c.v[j] + a0;
        const T                  sn = c.swa[j] + a1;
        pf_predict_state<T>(X, P, vn, sn, Q, wb, dt);
        if (use_heading)
        {
            pf_heading_state<T>(X, P, c.phi[j], Rphi);
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        s.pv[(size_t)i * s.np + p] = P[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        s.xv[(size_t)i * s.np + p] = X[i];
    }
}

constexpr int kPfFs1Obs = 8; // observations of one chunk of pf_likelihood_update_kernel (= waves of its workgroup)

// The scan's per-particle work of the FastSLAM-1 step.  Workgroup (64, kPfFs1Obs): threadIdx.x is the particle, so every
// feature load and store is 64 consecutive particles of the SoA store (whole lines); threadIdx.y is the observation
// within a chunk of kPfFs1Obs, one wave each.  Wave y evaluates the factor of observation base + y at the particle's
// pose (compute_jacobians, V = Z - ZP with the bearing wrapped, gauss_evaluate) and leaves it in LDS; wave 0 forms the
// product in the reference's order, ((1 * l0) * l1) ..., carrying it across chunks, and multiplies the weight by it.
//   fu_mode != 0: the lane that holds observation i's Jacobians and innovation finishes the feature's Kalman update
//                 (pf_feature_kf; 1: the reference's gain, 2: the textbook one) and stores it.  The host asks for this
//                 only when no feature is named twice, so no lane reads what another one writes.
//   zero_pv:      Pv = 0 after the scan (the state sampleProposal leaves, PF.cpp:537).
// xv is never written; Pv is never read.
template <typename T>
__global__ void __launch_bounds__(64 * kPfFs1Obs) pf_likelihood_update_kernel(PfStore<T> s, const T* __restrict__ Z,
                                                                               const int* __restrict__ idf, int m, T r00,
                                                                               T r10, T r01, T r11, int fu_mode,
                                                                               int zero_pv)
{
    __shared__ T s_l[kPfFs1Obs][64];
    const int  lane = threadIdx.x, y = threadIdx.y;
    const int  p    = blockIdx.x * 64 + lane;
    const bool live = p < s.np;
    const int  pc   = live ? p : s.np - 1; // (a lane beyond the store repeats the last particle and stores nothing)
    const T    R[4] = {r00, r10, r01, r11};
    T          X[3];
#pragma unroll
    for (int e = 0; e < 3; e++)
    {
        X[e] = s.xv[(size_t)e * s.np + pc];
    }
    T like = (T)1;
    for (int base = 0; base < m; base += kPfFs1Obs)
    {
        const int i = base + y;
        if (i < m) // (wave-uniform)
        {
            const int f = idf[i] - 1;
            T         xf[2], pf[4], ZP[2], HV[6], HF[4], SF[4], V[2];
            load_feature<T>(s, pc, f, xf, pf);
            compute_jacobians<T>(X, xf, pf, R, ZP, HV, HF, SF);
            V[0]         = Z[2 * i] - ZP[0];
            V[1]         = pi2pi<T>(Z[2 * i + 1] - ZP[1]);
            s_l[y][lane] = gauss_evaluate<T, 2>(V, SF);
            if (fu_mode != 0 && live)
            {
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
        }
        __syncthreads();
        if (y == 0)
        {
#pragma unroll
            for (int j = 0; j < kPfFs1Obs; j++)
            {
                if (base + j < m)
                {
                    like = like * s_l[j][lane]; // the reference's order: ((1 * l0) * l1) * ...
                }
            }
        }
        __syncthreads(); // the factors have been read before the next chunk overwrites them
    }
    if (y != 0 || !live)
    {
        return;
    }
    s.w[p] = s.w[p] * like;
    if (zero_pv)
    {
#pragma unroll
        for (int e = 0; e < 9; e++)
        {
            s.pv[(size_t)e * s.np + p] = (T)0;
        }
    }
}

} // namespace cslam
