// conan-slam-amd: Slam::augment for the single handle with the new features read from device memory, q features per
// launch (cslam_ekf_augment_device).
//
//   ekf_augment_many_kernel   EKF::addOneNewFeature (EKF.cpp:28-91) applied q <= kAugChunk times by ONE launch.
//
// ekf_augment_kernel (ekf_pose_kernels.hpp) adds one feature per launch and takes (r, b) as launch arguments; feature f
// reads back, through the pose stripe, what the launches of the features before it wrote.  Here every input is pre-call
// data -- X[0:3], the stripe Pv[:, 0:len0] with its 3 x 3 pose block, R and Z -- so that no thread reads what another
// writes and one launch can hold every feature:
//
//   * With len_f = len0 + 2 f, the rows feature f adds are Gv_f * P[0:3, 0:len_f] (EKF.cpp:77-84).  For an existing
//     column j < len0 the three stripe values are read once and serve all q features.
//   * A column j >= len0 is a row that an earlier feature g of the same call added: the launch of g would have written its
//     stripe entries as Gv_g[rr, :] * Pvv[:, c], c = 0..2, with the statements of the column loop; they are recomputed
//     here from Gv_g and the 3 x 3 block instead of being read back, and carry the same bits.
//   * q tail threads, one per feature, write the 2 x 2 diagonal blocks (EKF.cpp:74) and the new entries of X.
//
// One thread per column j < len0 + 2 q, then the q tail threads.  Thread j stores the 2 (q - f0) new entries of column j
// contiguously, from P[j ldp + len0 + 2 f0] on (f0 = 0 for an existing column, g + 1 for a column that feature g added), where the per-feature
// kernel makes q scattered two-scalar stores at a stride of ldp; the mirror stores run along the columns' rows and are
// coalesced across the threads.  Mirrors follow the rule of ekf_augment_body: always under full storage, inside the same
// 128-tile under block-lower storage.
//
// The same bits as q launches of ekf_augment_kernel.  That kernel leaves the choice between a fused multiply-add and a
// rounded product to the compiler (-ffp-contract=fast), and the choice depends on the code around an expression: the
// same statements compiled here came out contracted differently (one ulp in the diagonal block).  So this kernel fixes
// the arithmetic instead: contraction is switched off inside its functions and every fused multiply-add is written out,
// following what ekf_augment_kernel<float> and <double> do in their gfx950 code (the two agree):
//   * every accumulation `acc += a * b` of ekf_augment_body is fused, and a first term `0 + a * b` is fma(a, b, 0);
//   * the constant entries 1 and 0 of Gv are folded as 1 * a = a, while 0 * a stays a term (it is exact);
//   * -r s and r c are rounded products; X[len] = X[0] + (r c) adds the rounded product, X[len + 1] = fma(r, s, X[1]).
// Every workgroup computes sin and cos of the q bearings once, into LDS.
#pragma once

#include "ekf_kernels.hpp"

namespace cslam
{

constexpr int kAugChunk = 64; // features per launch (cslam_ekf_augment_device splits a longer list into chunks)

__device__ __forceinline__ float  aug_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double aug_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// Gv (rows (1, 0, g4) and (0, 1, g5)) applied to one column (a0, a1, a2) of P[0:3, :]: the column loop of
// ekf_augment_body, `acc = 0; acc += Gv[rr] * a0; acc += Gv[rr + 2] * a1; acc += Gv[rr + 4] * a2`
template <typename T>
__device__ __forceinline__ T aug_row0(T g4, T a0, T a1, T a2)
{
#pragma clang fp contract(off)
    return aug_fma(g4, a2, aug_fma((T)0, a1, a0 + (T)0));
}
template <typename T>
__device__ __forceinline__ T aug_row1(T g5, T a0, T a1, T a2)
{
#pragma clang fp contract(off)
    return aug_fma(g5, a2, a1 + aug_fma(a0, (T)0, (T)0));
}

// grid = ceil((len0 + 3 q) / 256) x 256, 1 <= q <= kAugChunk; Z: 2 x q (r, b) pairs in device memory
template <typename T>
__global__ void __launch_bounds__(256) ekf_augment_many_kernel(T* __restrict__ X, T* __restrict__ P, T* __restrict__ Pv,
                                                                int ldp, int len0, const T* __restrict__ Z, int q, T r00,
                                                                T r10, T r01, T r11, int lower)
{
#pragma clang fp contract(off)
    __shared__ T s_r[kAugChunk], s_s[kAugChunk], s_c[kAugChunk], s_g4[kAugChunk], s_g5[kAugChunk];
    if ((int)threadIdx.x < q)
    {
        const T r = Z[2 * threadIdx.x], b = Z[2 * threadIdx.x + 1];
        const T s = dsin(X[2] + b), c = dcos(X[2] + b);
        s_r[threadIdx.x]  = r;
        s_s[threadIdx.x]  = s;
        s_c[threadIdx.x]  = c;
        s_g4[threadIdx.x] = -r * s;
        s_g5[threadIdx.x] = r * c;
    }
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= len0 + 3 * q)
    {
        return;
    }
    if (j >= len0 + 2 * q)
    {
        // tail thread of feature f: X and the 2 x 2 diagonal block (thread 0 of ekf_augment_body)
        const int f   = j - (len0 + 2 * q);
        const int len = len0 + 2 * f;
        const T   r = s_r[f], s = s_s[f], c = s_c[f], g4 = s_g4[f], g5 = s_g5[f];
        X[len]     = X[0] + g5;
        X[len + 1] = aug_fma(r, s, X[1]);
        const T Gz[4] = {c, s, g4, g5};
        const T R[4]  = {r00, r10, r01, r11};
        T       GvP[6]; // Gv * Pvv, 2x3 column-major
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
        {
            const T p0 = Pv[(size_t)cc * ldp + 0], p1 = Pv[(size_t)cc * ldp + 1], p2 = Pv[(size_t)cc * ldp + 2];
            GvP[0 + 2 * cc] = aug_row0<T>(g4, p0, p1, p2);
            GvP[1 + 2 * cc] = aug_row1<T>(g5, p0, p1, p2);
        }
        T GzR[4];
#pragma unroll
        for (int cc = 0; cc < 2; cc++)
        {
#pragma unroll
            for (int rr = 0; rr < 2; rr++)
            {
                GzR[rr + 2 * cc] = aug_fma(Gz[rr + 2], R[1 + 2 * cc], aug_fma(Gz[rr], R[2 * cc], (T)0));
            }
        }
#pragma unroll
        for (int rr = 0; rr < 2; rr++)
        {
            // Gv Pvv Gv^T: `b1 = 0; b1 += GvP[rr + 2 l] * Gv[cc + 2 l]` with Gv[cc + 2 l] = (1, 0, g4) and (0, 1, g5)
            const T b1c0 = aug_fma(g4, GvP[rr + 4], aug_fma((T)0, GvP[rr + 2], GvP[rr]));
            const T b1c1 = aug_fma(g5, GvP[rr + 4], aug_fma(GvP[rr], (T)0, (T)0) + GvP[rr + 2]);
            // Gz R Gz^T
            const T b2c0 = aug_fma(GzR[rr + 2], Gz[0 + 2], aug_fma(GzR[rr], Gz[0], (T)0));
            const T b2c1 = aug_fma(GzR[rr + 2], Gz[1 + 2], aug_fma(GzR[rr], Gz[1], (T)0));
            P[(size_t)(len + 0) * ldp + len + rr] = b1c0 + b2c0; // EKF.cpp:74
            P[(size_t)(len + 1) * ldp + len + rr] = b1c1 + b2c1;
        }
        return;
    }
    T   a0, a1, a2; // column j of P[0:3, :]
    int f0;         // the first feature whose rows reach column j
    if (j < len0)
    {
        a0 = Pv[(size_t)0 * ldp + j];
        a1 = Pv[(size_t)1 * ldp + j];
        a2 = Pv[(size_t)2 * ldp + j];
        f0 = 0;
    }
    else
    {
        const int g = (j - len0) >> 1, grr = (j - len0) & 1;
        const T   g4 = s_g4[g], g5 = s_g5[g];
        // the stripe entries of row j, as the threads 0..2 of the launch of feature g form them
        T st[3];
#pragma unroll
        for (int cc = 0; cc < 3; cc++)
        {
            const T p0 = Pv[(size_t)0 * ldp + cc], p1 = Pv[(size_t)1 * ldp + cc], p2 = Pv[(size_t)2 * ldp + cc];
            const T v0 = aug_row0<T>(g4, p0, p1, p2), v1 = aug_row1<T>(g5, p0, p1, p2);
            st[cc]     = grr ? v1 : v0;
        }
        a0 = st[0];
        a1 = st[1];
        a2 = st[2];
        f0 = g + 1;
    }
    // EKF.cpp:77-78, 83-84 for every feature f >= f0: rows len0 + 2 f, + 1 of column j, mirrored into the new columns
    T* const col = (j < 3 ? Pv : P) + (size_t)j * ldp; // pose columns of the new rows: the stripe
    for (int f = f0; f < q; f++)
    {
        const T   v0 = aug_row0<T>(s_g4[f], a0, a1, a2), v1 = aug_row1<T>(s_g5[f], a0, a1, a2);
        const int row = len0 + 2 * f;
        col[row]     = v0;
        col[row + 1] = v1;
        if (j >= 3)
        {
            if (!lower || ((j >> 7) == (row >> 7)))
            {
                P[(size_t)row * ldp + j] = v0; // the mirror exists under full storage / inside a diagonal tile
            }
            if (!lower || ((j >> 7) == ((row + 1) >> 7)))
            {
                P[(size_t)(row + 1) * ldp + j] = v1;
            }
        }
    }
}

} // namespace cslam
