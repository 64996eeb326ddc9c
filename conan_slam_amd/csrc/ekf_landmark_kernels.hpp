// ekf_landmark_kernels.hpp -- the landmark read (cslam_ekf_get_landmarks / cslam_ekf_batch_get_landmarks): every
// landmark's mean X[fx:fx+2], its 2 x 2 block P[fx:fx+2, fx:fx+2] and its pose block P[0:3, fx:fx+2], read from the
// deferred form of the covariance WITHOUT applying it (no P-GEMM, no mirror, no copy of P):
//     P = Ps - Wp diag(s) Wp^T   over the kp pending columns of the current region,
// with s_c = -1 for the single filter's heading columns stored with S < 0 (sgn[c] != 0, ekf_pose_step_kernel) and +1
// otherwise.  The pose block lives in the stripe Pv, which is always current (the pending panels carry zero pose rows:
// see p_get in ekf_kernels.hpp), so only the 2 x 2 block needs the rank-kp correction: three Ps entries and three dot
// products of length kp over the panel rows fx and fx+1.
//
// One lane per landmark.  Lane j reads rows fx = 2 (first + j) + 1 and fx + 1 of every pending column: the lanes of a
// wave read 128 consecutive scalars of each column (coalesced); nothing is staged in LDS.
//
// Outputs (compact, landmark-major; any pointer may be null): x [count][2], pll [count][4] (2 x 2 column-major, both
// off-diagonal entries written from the one value P[fx+1, fx] -- exactly symmetric), pvl [count][6] (P[0:3, fx:fx+2]
// column-major).
#pragma once

#include <hip/hip_runtime.h>

#include "ekf_kernels.hpp"

namespace cslam
{

template <typename T>
__device__ inline void landmark_read_body(const T* __restrict__ X, const T* __restrict__ Pv, const T* __restrict__ P, int ldp,
                                          int lower, const T* __restrict__ W, int ldw, int kp, const int* __restrict__ sgn,
                                          int first, int j, T* __restrict__ x, T* __restrict__ pll, T* __restrict__ pvl)
{
    const int fx = 2 * (first + j) + 1; // 0-based row of landmark first + j (1-based): 3 + 2 (f - 1)
    if (x)
    {
        x[2 * j]     = X[fx];
        x[2 * j + 1] = X[fx + 1];
    }
    if (pvl)
    {
        for (int c = 0; c < 2; c++)
        {
            for (int r = 0; r < 3; r++)
            {
                pvl[6 * j + 3 * c + r] = p_get<T>(P, Pv, ldp, r, fx + c, lower);
            }
        }
    }
    if (pll)
    {
        T s00 = (T)0, s10 = (T)0, s11 = (T)0;
        for (int c = 0; c < kp; c++)
        {
            const T* w  = W + (size_t)c * ldw;
            const T  a  = w[fx];
            const T  b  = w[fx + 1];
            const T  sa = (sgn != nullptr && sgn[c] != 0) ? -a : a;
            const T  sb = (sgn != nullptr && sgn[c] != 0) ? -b : b;
            s00 += sa * a;
            s10 += sb * a;
            s11 += sb * b;
        }
        // (fx >= 3: p_sym, not the stripe.  A landmark with fx = 127 mod 128 straddles two row tiles: p_sym reads its
        // (fx+1, fx) entry from the lower tile, where block-lower storage keeps it.)
        const T p00 = p_sym<T>(P, ldp, fx, fx, lower) - s00;
        const T p10 = p_sym<T>(P, ldp, fx + 1, fx, lower) - s10;
        const T p11 = p_sym<T>(P, ldp, fx + 1, fx + 1, lower) - s11;
        pll[4 * j]     = p00;
        pll[4 * j + 1] = p10;
        pll[4 * j + 2] = p10;
        pll[4 * j + 3] = p11;
    }
}

// single filter: grid.x = ceil(count / 256)
template <typename T>
__global__ void __launch_bounds__(256) ekf_landmark_read_kernel(const T* __restrict__ X, const T* __restrict__ Pv,
                                                                const T* __restrict__ P, int ldp, int lower,
                                                                const T* __restrict__ W, int ldw, int kp,
                                                                const int* __restrict__ sgn, int first, int count,
                                                                T* __restrict__ x, T* __restrict__ pll, T* __restrict__ pvl)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= count)
    {
        return;
    }
    landmark_read_body<T>(X, Pv, P, ldp, lower, W, ldw, kp, sgn, first, j, x, pll, pvl);
}

// (the batched engine's kernel, ekf_landmark_read_batch, lives in cslam_ekf_batch.hip)

} // namespace cslam
