// ekf_factor_small_kernel_body.inc -- the statements of ekf_factor_small_kernel<T, K> (see there for what they do), kept apart so that the
// counted entry of ekf_counted_kernels.hpp, which reads the observation count from device memory, is built from the
// same text: included inside a function that has the kernel's parameters (and template parameters) in scope.
    constexpr int LD = K + 1;
    __shared__ T   S[K * LD];
    __shared__ T   coef[(K / 2) * 10];
    __shared__ T   V[K];
    __shared__ T   tvec[K];
    __shared__ int fxs[K / 2];
    __shared__ int sflg[2];
    const int      k   = 2 * a.m;
    const int      tid = threadIdx.x;

    auto stamp = [&](int i) {
        if (a.stamps && tid == 0)
        {
            a.stamps[i] = (long long)__builtin_readcyclecounter();
        }
    };
    stamp(0);
    if (tid == 0)
    {
        sflg[0] = 0;
        sflg[1] = 0;
    }
    if (tid < K)
    {
        V[tid] = (T)0;
    }
    __syncthreads();
    for (int o = tid; o < a.m; o += 256)
    {
        observe_model<T>(a.X, a.n, a.idf[o], a.Z[2 * o], a.Z[2 * o + 1], &coef[o * 10], &V[2 * o], &fxs[o]);
        a.dV[2 * o]     = V[2 * o];
        a.dV[2 * o + 1] = V[2 * o + 1];
    }
    __syncthreads();
    // S = H*PHT + RR (slam.h:244): 5-term sums in ascending column order; identity padding.
    // Two passes with compile-time trip counts: first every global load of the thread's elements is issued
    // (they are independent L2 hits), then the sums are formed -- one round trip instead of one per element.
    {
        constexpr int NE = (K * K + 255) / 256;
        const T       r00 = a.R[0], r10 = a.R[1], r01 = a.R[2], r11 = a.R[3]; // no indexed kernarg loads below
        T             ph[NE][5];
#pragma unroll
        for (int it = 0; it < NE; it++)
        {
            const int e  = tid + it * 256;
            const int r  = e & (K - 1);
            const int c  = e / K;
            const bool in = (e < K * K) && (r < k) && (c < k);
            const int rc = in ? r : 0, cc = in ? c : 0; // clamped: loads stay unconditional
            const int fx = fxs[rc >> 1];
            const T*  p  = a.PHT + (size_t)cc * a.ldw;
            ph[it][0]    = p[0];
            ph[it][1]    = p[1];
            ph[it][2]    = p[2];
            ph[it][3]    = p[fx];
            ph[it][4]    = p[fx + 1];
        }
#pragma unroll
        for (int it = 0; it < NE; it++)
        {
            const int e = tid + it * 256;
            if (e < K * K)
            {
                const int r = e & (K - 1);
                const int c = e / K;
                T         v;
                if (r < k && c < k)
                {
                    const int ob = r >> 1, ra = r & 1;
                    const T*  cf = &coef[ob * 10 + ra * 5];
                    T         sm = cf[0] * ph[it][0];
                    sm += cf[1] * ph[it][1];
                    sm += cf[2] * ph[it][2];
                    sm += cf[3] * ph[it][3];
                    sm += cf[4] * ph[it][4];
                    const int ri = ra + 2 * (c & 1);
                    const T   rv = (ri == 0) ? r00 : ((ri == 1) ? r10 : ((ri == 2) ? r01 : r11));
                    v = sm + (((c >> 1) == ob) ? rv : (T)0);
                }
                else
                {
                    v = (r == c) ? (T)1 : (T)0;
                }
                S[r + c * LD] = v;
            }
        }
    }
    __syncthreads();
    // makeSymmetric (slam.h:776-779)
    for (int e = tid; e < K * K; e += 256)
    {
        const int r = e & (K - 1);
        const int c = e / K;
        if (r > c)
        {
            T v           = (S[r + c * LD] + S[c + r * LD]) * (T)0.5;
            S[r + c * LD] = v;
            S[c + r * LD] = v;
        }
        else if (r == c)
        {
            T d           = S[r + c * LD];
            S[r + c * LD] = (d + d) * (T)0.5;
        }
    }
    __syncthreads();
    for (int e = tid; e < K * K; e += 256)
    {
        const int r = e & (K - 1), c = e / K;
        if (r < k && c < k)
        {
            a.dS[r + c * k] = S[r + c * LD];
        }
    }
    __syncthreads();

    stamp(1);
    if (tid < 64) // ---------------- one wave: lane = row of S / column of inv(L)
    {
        const int lane = tid;
        T         row[K];
#pragma unroll
        for (int c = 0; c < K; c++)
        {
            row[c] = (lane < K) ? S[lane + c * LD] : ((c == lane) ? (T)1 : (T)0);
        }
        T          rdiag[K]; // wave-uniform reciprocals of the diagonal of L
        const bool failed = wave_cholesky<T, K>(row, rdiag, lane);
        stamp(2);
        T    x[K];
        bool bad = false;
        if (!failed)
        {
            bad = wave_tri_inverse<T, K>(row, rdiag, lane, k, x);
        }
        stamp(3);
        const bool zero = failed || bad;
        // G back into LDS (over S): REF_EXACT G = inv(L) -> G[r][c] = x[r] of lane c; TEXTBOOK G = inv(L)^T
        if (lane < K)
        {
#pragma unroll
            for (int r = 0; r < K; r++)
            {
                const T g = zero ? (T)0 : x[r];
                if (a.textbook)
                {
                    S[lane + r * LD] = g; // G[c][r] = inv(L)[r][c]
                }
                else
                {
                    S[r + lane * LD] = g;
                }
            }
        }
        if (lane == 0)
        {
            sflg[0] = failed ? 1 : 0;
            sflg[1] = (!failed && bad) ? 1 : 0;
        }
    }
    __syncthreads();
    // outputs: G, G^T (coalesced), t = G^T V, u = G t
    for (int e = tid; e < K * K; e += 256)
    {
        const int r = e & (K - 1), c = e / K;
        if (r < k && c < k)
        {
            a.dG[r + c * k] = S[r + c * LD];
        }
    }
    for (int e = tid; e < K * K; e += 256)
    {
        const int c = e & (K - 1), r = e / K;
        if (r < k && c < k)
        {
            a.dGt[c + r * k] = S[r + c * LD];
        }
    }
    // t = G^T V and u = G t: 4 lanes per output element, partial sums combined in a fixed order
    {
        const int o = tid >> 2, part = tid & 3; // 256 threads = 64 outputs x 4 parts
        T         s = (T)0;
        if (o < K)
        {
#pragma unroll 4
            for (int r = part; r < K; r += 4)
            {
                s += S[r + o * LD] * V[r]; // padding rows of V are zero
            }
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (part == 0 && o < K)
        {
            if (o < k)
            {
                a.dt[o] = s;
            }
            tvec[o] = (o < k) ? s : (T)0;
        }
        __syncthreads();
        T s2 = (T)0;
        if (o < K)
        {
#pragma unroll 4
            for (int c = part; c < K; c += 4)
            {
                s2 += S[o + c * LD] * tvec[c];
            }
        }
        s2 += __shfl_xor(s2, 1);
        s2 += __shfl_xor(s2, 2);
        if (part == 0 && o < k)
        {
            du[o] = s2;
        }
        // M[:, c] = G (G^T PHT[c, :]^T), c = 0..2: lets the gain kernel apply the pose-stripe downdate itself
        // (see ekf_factor_mfma_f32; the sequential update runs this kernel once per observation)
        if (a.dM != nullptr)
        {
            for (int c = 0; c < 3; c++)
            {
                __syncthreads();
                T s3 = (T)0;
                if (o < K)
                {
#pragma unroll 4
                    for (int r = part; r < K; r += 4)
                    {
                        s3 += S[r + o * LD] * ((r < k) ? a.PHT[(size_t)r * a.ldw + c] : (T)0);
                    }
                }
                s3 += __shfl_xor(s3, 1);
                s3 += __shfl_xor(s3, 2);
                if (part == 0 && o < K)
                {
                    tvec[o] = (o < k) ? s3 : (T)0;
                }
                __syncthreads();
                T s4 = (T)0;
                if (o < K)
                {
#pragma unroll 4
                    for (int q = part; q < K; q += 4)
                    {
                        s4 += S[o + q * LD] * tvec[q];
                    }
                }
                s4 += __shfl_xor(s4, 1);
                s4 += __shfl_xor(s4, 2);
                if (part == 0 && o < k)
                {
                    a.dM[c * k + o] = s4;
                }
            }
        }
    }
    stamp(4);
    if (tid == 0)
    {
        const int code = (sflg[0] ? kFlagLltFailed : 0) | (sflg[1] ? kFlagZeroed : 0);
        a.flags[1]     = code;
        if (code)
        {
            atomicOr(&a.flags[0], code);
        }
    }
