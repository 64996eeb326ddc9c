// ekf_counted_kernels.hpp -- the classic update chain (gather -> [correction] -> factor -> gain) with the number of
// observations read on the device (cslam_ekf_update_counted; slam.h:235-266 via EKF.cpp:93-129, where the count is the
// row count of the ZF that dataAssociate has just split off, slam.h:938-943).
//
// Every kernel of the chain takes m (or k, kq, nc, ldb = 2m) as a launch argument.  A counted entry takes a pointer to
// the count and the capacity m_cap the host sized the launch for instead:
//     c = clamp(*d_count, 0, m_cap),   loaded once, made wave-uniform with readfirstlane (k = 2c stays in scalar
//                                      registers: index arithmetic and loop bounds built from it need no waterfall loops)
// and then runs the statements of the kernel it mirrors (the *_body.inc files, or the __device__ body where the kernel has
// one) with m = c, so every layout that depends on k -- the stride of the
// compact `sub` block, the leading dimensions of Gt / S / Y, the row stride of M -- is the one an update of c
// observations has, consistently from one kernel to the next.  The kernel CLASS (small / MFMA 32 / 64 / 128) is chosen
// on the host from m_cap, so a body built for 32 < k <= 64 also sees k = 2, 4, ...: the identity padding of the factor
// bodies (rows and columns [k, K) of S) is what makes that legal.
//   c = 0: gather and factor workgroups leave without a store (the factor kernel may raise the clamp flag); the gain
//   kernel only zero-fills.
//   Grids are sized from m_cap: gather workgroups whose observations are all >= c leave, and so do the column tiles of
//   the correction launch beyond 2c.  The gain kernel's column tiles write columns [2c, 2 m_cap) of the W1 slot as exact
//   zeros on all n_pad rows: the host books 2 m_cap pending columns, and every reader of the pending store (the P-GEMM,
//   the gather corrections, the landmark read, the score, the association pair kernel) sees inert columns there.
// Entries c .. m_cap-1 of Z / idf are never read.
#pragma once

#include <hip/hip_runtime.h>

#include "ekf_kernels.hpp"
#include "ekf_kernels_fast.hpp"

namespace cslam
{

constexpr int kFlagCountClamped = 64; // *d_count was outside 0..m_cap (cslam_ekf_update_counted)

// the count of a counted launch: one load, clamped, in a scalar register
__device__ __forceinline__ int counted_m(const int* __restrict__ d_count, int m_cap, bool* clamped)
{
    const int raw = __builtin_amdgcn_readfirstlane(*d_count);
    const int c   = min(max(raw, 0), m_cap);
    *clamped      = (raw != c);
    return c;
}

// ---------------------------------------------------------------------------------------------- gather
// grid = (ceil(n/256), ceil(m_cap/OBS)), as ekf_gather_kernel<T, KC, OBS> with m = m_cap.  No held predict rides along
// (cslam_ekf_update_counted resolves it first): pp.valid = 0 and pred_out = nullptr.  They stay launch arguments, as in
// the kernel this one mirrors, on purpose: with pp a compile-time constant the compiler contracts the f32 observation
// model differently (d2 = dx*dx + dy*dy as a packed multiply and an add instead of a fused multiply-add), and a count
// equal to m_cap would no longer give update_device's result bit for bit.
template <typename T, int KC = kGatherCorr, int OBS = kGatherObs>
__global__ void __launch_bounds__(256) ekf_gather_counted_kernel(const T* __restrict__ X, const T* __restrict__ P,
                                                                  const T* __restrict__ Pv, int ldp, int n,
                                                                  const T* __restrict__ Z, const int* __restrict__ idf,
                                                                  const int* __restrict__ d_count, int m_cap,
                                                                  T* __restrict__ PHT, int ldw, int lower,
                                                                  T* __restrict__ sub, PredictArgs<T> pp,
                                                                  T* __restrict__ pred_out, const T* __restrict__ Wc,
                                                                  int ldwc, int kc, const int* __restrict__ sgn,
                                                                  int* __restrict__ flags, T* __restrict__ Yout)
{
    bool      clamped;
    const int m = counted_m(d_count, m_cap, &clamped);
    if ((int)(blockIdx.y * OBS) >= m) // (workgroup-uniform) every observation of this workgroup lies in the unused tail
    {
        return;
    }
#include "ekf_gather_kernel_body.inc"
}

// ---------------------------------------------------------------------------------------------- factor
// one workgroup each, launched exactly as the kernel it mirrors (block 256, the same dynamic LDS)
__device__ __forceinline__ int counted_factor_m(const int* __restrict__ d_count, int m_cap, int* __restrict__ flags)
{
    bool      clamped;
    const int m = counted_m(d_count, m_cap, &clamped);
    if (clamped && threadIdx.x == 0)
    {
        atomicOr(&flags[0], kFlagCountClamped);
    }
    return m;
}

template <typename T, int K>
__global__ void __launch_bounds__(256) ekf_factor_small_counted_kernel(FactorArgs<T> a, T* __restrict__ du,
                                                                        const int* __restrict__ d_count, int m_cap)
{
    a.m = counted_factor_m(d_count, m_cap, a.flags);
    if (a.m == 0)
    {
        return;
    }
#include "ekf_factor_small_kernel_body.inc"
}

template <int K>
__global__ void __launch_bounds__(256) ekf_factor_mfma_f32_counted(FactorArgs<float> a, float* __restrict__ du,
                                                                    const int* __restrict__ d_count, int m_cap)
{
    a.m = counted_factor_m(d_count, m_cap, a.flags);
    if (a.m == 0)
    {
        return;
    }
    ekf_factor_mfma_f32_body<K>(a, du);
}

template <int K>
__global__ void __launch_bounds__(256) ekf_factor_mfma_f64_counted(FactorArgs<double> a, double* __restrict__ du,
                                                                    const int* __restrict__ d_count, int m_cap)
{
    a.m = counted_factor_m(d_count, m_cap, a.flags);
    if (a.m == 0)
    {
        return;
    }
    ekf_factor_mfma_f64_body<K>(a, du);
}

template <int K>
__global__ void __launch_bounds__(256) ekf_factor_mfma_big_f32_counted(FactorArgs<float> a, float* __restrict__ du,
                                                                        const int* __restrict__ d_count, int m_cap)
{
    a.m = counted_factor_m(d_count, m_cap, a.flags);
    if (a.m == 0)
    {
        return;
    }
#include "ekf_factor_mfma_big_f32_body.inc"
}

// ---------------------------------------------------------------------------------------------- correction and gain
// The two launches of ekf_panel_mfma_f32 / _f64 that depend on k:
//   correction <true, false>: OUT = PHT -= Wp * Y^T, kq = kp (from the host), nc = ldb = k
//   gain       <false, true>: OUT = W1 slot = PHT * G, kq = nc = ldb = k, X += PHT * u, pose-stripe downdate from Mv
// grid = (n_pad/TR, ceil(2 m_cap/TC)) single-wave workgroups, TR x TC = 32 x 32 (f32) or 16 x 16 (f64).

// columns [c_lo, c_hi) of the rows [row0, row0 + TR) of OUT <- 0; one wave, TR rows across the low lanes
template <typename T, int TR>
__device__ __forceinline__ void counted_zero_cols(T* __restrict__ OUT, int ldo, int row0, int c_lo, int c_hi)
{
    const int lj = threadIdx.x % TR, lc = threadIdx.x / TR;
    for (int col = c_lo + lc; col < c_hi; col += 64 / TR)
    {
        OUT[(size_t)col * ldo + row0 + lj] = (T)0;
    }
}

__global__ void __launch_bounds__(64) ekf_corr_mfma_f32_counted(const float* __restrict__ Wp, int lda, int n, int kp,
                                                                 const int* __restrict__ d_count, int m_cap,
                                                                 const float* __restrict__ Y, float* __restrict__ PHT,
                                                                 int ldo)
{
    bool      clamped;
    const int k = 2 * counted_m(d_count, m_cap, &clamped);
    if ((int)(blockIdx.y * 32) >= k)
    {
        return;
    }
    constexpr bool     SUB = true, XUPD = false;
    const float* const A = Wp, *const Bt = Y, *const u = nullptr, *const pred = nullptr, *const Mv = nullptr;
    float* const       OUT = PHT, *const X = nullptr, *const P = nullptr, *const wv_out = nullptr;
    const int          kq = kp, nc = k, ldb = k, pred_w = 0, ldp = 0;
#include "ekf_panel_mfma_f32_body.inc"
}

__global__ void __launch_bounds__(64) ekf_corr_mfma_f64_counted(const double* __restrict__ Wp, int lda, int n, int kp,
                                                                 const int* __restrict__ d_count, int m_cap,
                                                                 const double* __restrict__ Y, double* __restrict__ PHT,
                                                                 int ldo)
{
    bool      clamped;
    const int k = 2 * counted_m(d_count, m_cap, &clamped);
    if ((int)(blockIdx.y * 16) >= k)
    {
        return;
    }
    constexpr bool      SUB = true, XUPD = false;
    const double* const A = Wp, *const Bt = Y, *const u = nullptr, *const pred = nullptr, *const Mv = nullptr;
    double* const       OUT = PHT, *const X = nullptr, *const Pv = nullptr, *const wv_out = nullptr;
    const int           kq = kp, nc = k, ldb = k, pred_w = 0, ldp = 0;
#include "ekf_panel_mfma_f64_body.inc"
}

__global__ void __launch_bounds__(64) ekf_gain_mfma_f32_counted(const float* __restrict__ PHT, int lda, int n,
                                                                 const int* __restrict__ d_count, int m_cap,
                                                                 const float* __restrict__ Gt, const float* __restrict__ u,
                                                                 float* __restrict__ slot, int ldo, float* __restrict__ X,
                                                                 float* __restrict__ Pv, int ldp,
                                                                 const float* __restrict__ Mv, float* __restrict__ wv_out)
{
    bool      clamped;
    const int k    = 2 * counted_m(d_count, m_cap, &clamped);
    const int c0   = blockIdx.y * 32;
    const int c_hi = min(c0 + 32, 2 * m_cap);
    if (c0 < k) // (workgroup-uniform)
    {
        constexpr bool     SUB = false, XUPD = true;
        const float* const A = PHT, *const Bt = Gt, *const pred = nullptr;
        float* const       OUT = slot, *const P = Pv;
        const int          kq = k, nc = k, ldb = k, pred_w = 0;
#include "ekf_panel_mfma_f32_body.inc"
    }
    counted_zero_cols<float, 32>(slot, ldo, blockIdx.x * 32, max(c0, k), c_hi);
}

__global__ void __launch_bounds__(64) ekf_gain_mfma_f64_counted(const double* __restrict__ PHT, int lda, int n,
                                                                 const int* __restrict__ d_count, int m_cap,
                                                                 const double* __restrict__ Gt,
                                                                 const double* __restrict__ u, double* __restrict__ slot,
                                                                 int ldo, double* __restrict__ X, double* __restrict__ Pv,
                                                                 int ldp, const double* __restrict__ Mv,
                                                                 double* __restrict__ wv_out)
{
    bool      clamped;
    const int k    = 2 * counted_m(d_count, m_cap, &clamped);
    const int c0   = blockIdx.y * 16;
    const int c_hi = min(c0 + 16, 2 * m_cap);
    if (c0 < k) // (workgroup-uniform)
    {
        constexpr bool      SUB = false, XUPD = true;
        const double* const A = PHT, *const Bt = Gt, *const pred = nullptr;
        double* const       OUT = slot;
        const int           kq = k, nc = k, ldb = k, pred_w = 0;
#include "ekf_panel_mfma_f64_body.inc"
    }
    counted_zero_cols<double, 16>(slot, ldo, blockIdx.x * 16, max(c0, k), c_hi);
}

} // namespace cslam
