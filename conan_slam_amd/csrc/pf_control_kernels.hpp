// pf_control_kernels.hpp -- a run of control steps of the FastSLAM-2 particle loop in ONE launch.
//
// Between two scans the reference's particle loop runs about six control steps (mDtObserve = 5.058 mDtControls,
// slam.h:69-77), each of them PF::predict followed by PF::observeHeading for every particle (test/main.cpp:279-286;
// mSwitchHeadingKnown is true by default, slam.h:99).  pf_predict_kernel and pf_heading_kernel (pf_kernels.hpp) do one
// of the two per launch and move the 12 scalars of pose state through HBM each time.  pf_control_run_kernel loads the
// pose once, applies up to kPfControlMax steps in registers and stores once.
//
// The arithmetic is that of the two kernels it replaces, operation by operation: pf_predict_state is shared, and
// pf_heading_state below is a sibling of pf_heading_kernel's body (the existing kernel keeps its own copy, so its code
// object does not change).
#pragma once

#include <hip/hip_runtime.h>

#include "pf_kernels.hpp"

#pragma clang fp contract(off)

namespace cslam
{

constexpr int kPfControlMax = 16; // control steps of one launch

// the controls of one launch, by value: the loop index is kernel-uniform, so step j's values are scalar loads from the
// kernel-argument segment
template <typename T>
struct PfControls
{
    T v[kPfControlMax], swa[kPfControlMax], phi[kPfControlMax];
};

// PF::observeHeading (PF.cpp:382-417) -> the KF update of slam.h:700-725 with n = 3, k = 1, H = (0 0 1), for one
// particle in registers: X and P (column-major 3 x 3) in, updated values out.  The operation order is that of
// pf_heading_kernel: the dense P H^T, S = H P H^T + R, SI = 1/S symmetrised as (SI + SI) * 0.5, W = P H^T SI, the Joseph
// form (I - W H) P (I - W H)^T + W R W^T, and + delta_ij FLT_MIN on the diagonal.
template <typename T>
__device__ inline void pf_heading_state(T* X, T* P, T phi, T R)
{
    const T H[3] = {(T)0, (T)0, (T)1};
    T       V    = pi2pi<T>(phi - X[2]);
    T       PHT[3], W[3];
#pragma unroll
    for (int i = 0; i < 3; i++) // P*H^T, dense order
    {
        T a = (T)0;
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            a += P[i + 3 * j] * H[j];
        }
        PHT[i] = a;
    }
    T S = (T)0;
#pragma unroll
    for (int j = 0; j < 3; j++)
    {
        S += H[j] * PHT[j];
    }
    S    = S + R;
    T SI = (T)1 / S;
    SI   = (SI + SI) * (T)0.5;
#pragma unroll
    for (int i = 0; i < 3; i++)
    {
        W[i] = PHT[i] * SI;
        X[i] = X[i] + W[i] * V;
    }
    T Cm[9], CP[9], out[9];
#pragma unroll
    for (int j = 0; j < 3; j++)
    {
#pragma unroll
        for (int i = 0; i < 3; i++)
        {
            Cm[i + 3 * j] = ((i == j) ? (T)1 : (T)0) - W[i] * H[j];
        }
    }
    mm<T, 3, 3, 3>(Cm, P, CP);
#pragma unroll
    for (int j = 0; j < 3; j++)
    {
#pragma unroll
        for (int i = 0; i < 3; i++)
        {
            T a = (T)0;
#pragma unroll
            for (int l = 0; l < 3; l++)
            {
                a += CP[i + 3 * l] * Cm[j + 3 * l];
            }
            T b  = (W[i] * R) * W[j];
            T o  = a + b;
            o    = o + ((i == j) ? (T)1 : (T)0) * (T)1.17549435e-38f;
            out[i + 3 * j] = o;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
    {
        P[i] = out[i];
    }
}

// k <= kPfControlMax iterations of test/main.cpp:279-286 for every particle of the store: one lane per particle, grid
// ceil(np / 64) x 64 lanes.  k, use_heading and the controls are kernel-uniform; the loop is a runtime loop.
template <typename T>
__global__ void __launch_bounds__(64) pf_control_run_kernel(PfStore<T> s, int k, PfControls<T> c, T q00, T q10, T q01,
                                                            T q11, T wb, T dt, int use_heading, T Rphi)
{
    int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= s.np)
    {
        return;
    }
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
        pf_predict_state<T>(X, P, c.v[j], c.swa[j], Q, wb, dt);
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

} // namespace cslam
