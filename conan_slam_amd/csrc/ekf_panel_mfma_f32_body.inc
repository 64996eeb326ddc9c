// ekf_panel_mfma_f32_body.inc -- the statements of ekf_panel_mfma_f32<SUB, XUPD> (see there for what they do), kept apart so that the
// counted entry of ekf_counted_kernels.hpp, which reads the observation count from device memory, is built from the
// same text: included inside a function that has the kernel's parameters (and template parameters) in scope.
    // (P here is the pose stripe Pv, see p_get: the predicted stripe and pose block are committed there)
    // Mv != nullptr (gain, XUPD): the factor kernel supplied M = G G^T PHT[0:3,:]^T (3 x kq): the column-tile-0
    // workgroups also apply the pose-stripe share of slam.h:260, Pv[:, c] -= PHT * M[c, :]^T (= W1 * W1[c, :]^T), and the
    // pose rows of the W1 panel are written as ZERO (saved to wv_out, 3 x nc, for the debug entry point): the pending-
    // panel algebra never touches the stripe.
    // pred != nullptr (gain, XUPD): a predict() was applied on the fly by the gather and factor kernels (PredictArgs);
    // this kernel commits it: the column-tile-0 workgroups write the predicted stripe and Pvv into P and add the state
    // correction to the PREDICTED pose.  pred = {g02, g12, pose (3), Pvv (9)} from the factor kernel.
    // one wave per workgroup, one 32x32 MFMA tile per wave: grid = (n_pad/32 row tiles, ceil(nc/32) column tiles).
    // Small tiles on purpose: the kernel is a latency chain (load -> MFMA -> store), so it wants many waves.
    const int  lane = threadIdx.x;
    const int  lj   = lane & 31;
    const int  lh   = lane >> 5;
    const int  row0 = blockIdx.x * 32;
    const int  c0   = blockIdx.y * 32;
    const bool cok  = (c0 + lj) < nc;
    const int  cc   = cok ? (c0 + lj) : (nc - 1); // clamped: loads are unconditional, the VALUE is selected
    const bool dox  = XUPD && (blockIdx.y == 0);
    f32x16     acc  = {0};
    float      xs   = 0.f, xm0 = 0.f, xm1 = 0.f, xm2 = 0.f;
    const float* pa = A + row0 + lj;
    // SUB: the old values of the output tile are requested first, so that their latency (the tile was written by
    // another kernel on other XCDs a moment ago) hides behind the operand loads and the MFMAs
    float oldv[16];
    if (SUB)
    {
#pragma unroll
        for (int r = 0; r < 16; r++)
        {
            const int col = c0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            oldv[r]       = OUT[(size_t)(col < nc ? col : nc - 1) * ldo + row0 + lj];
        }
    }
    constexpr int NP = 32; // k-pairs per trip: every load of the trip is issued before its first MFMA
    for (int qb = 0; qb < kq; qb += 2 * NP)
    {
        float b[NP], g[NP], uq[NP];
#pragma unroll
        for (int t = 0; t < NP; t++)
        {
            const int q  = qb + 2 * t + lh;
            const int qc = (q < kq) ? q : (kq - 1);
            b[t]         = pa[(size_t)qc * lda];
            g[t]         = Bt[(size_t)qc * ldb + cc];
            uq[t]        = XUPD ? u[qc] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < NP; t++)
        {
            const int   q  = qb + 2 * t + lh;
            const bool  ok = q < kq;
            const float gg = (ok && cok) ? g[t] : 0.f;
            const float bb = ok ? b[t] : 0.f;
            acc            = __builtin_amdgcn_mfma_f32_32x32x2f32(gg, bb, acc, 0, 0, 0);
            xs += bb * uq[t];
        }
        if (XUPD && dox && Mv != nullptr) // (workgroup-uniform)
        {
#pragma unroll
            for (int t = 0; t < NP; t++)
            {
                const int   q  = qb + 2 * t + lh;
                const int   qc = (q < kq) ? q : (kq - 1);
                const float bb = (q < kq) ? b[t] : 0.f;
                xm0 += bb * Mv[qc];
                xm1 += bb * Mv[kq + qc];
                xm2 += bb * Mv[2 * kq + qc];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++)
    {
        const int col = c0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (col < nc)
        {
            float* o = OUT + (size_t)col * ldo + row0 + lj;
            if (!SUB && Mv != nullptr && row0 + lj < 3) // pose rows of the W1 panel: kept aside, stored as zero
            {
                wv_out[(size_t)(row0 + lj) * nc + col] = acc[r];
                *o                                     = 0.f;
            }
            else
            {
                *o = SUB ? (oldv[r] - acc[r]) : acc[r];
            }
        }
    }
    if (dox)
    {
        xs += __shfl_xor(xs, 32);
        xm0 += __shfl_xor(xm0, 32);
        xm1 += __shfl_xor(xm1, 32);
        xm2 += __shfl_xor(xm2, 32);
        const int r = row0 + lj;
        if (lh == 0 && r < n)
        {
            X[r] = ((pred != nullptr && r < 3) ? pred[2 + r] : X[r]) + xs;
            if (pred != nullptr || Mv != nullptr)
            {
                // row r of the pose stripe: [predicted (EKF.cpp:439-443)] then [downdated]
                float a0 = P[(size_t)0 * ldp + r], a1 = P[(size_t)1 * ldp + r], a2 = P[(size_t)2 * ldp + r];
                if (pred != nullptr)
                {
                    if (r >= 3)
                    {
                        if (r - 3 < pred_w)
                        {
                            float o0, o1, o2;
                            predict_stripe_col<float>(pred[0], pred[1], a0, a1, a2, &o0, &o1, &o2);
                            a0 = o0;
                            a1 = o1;
                            a2 = o2;
                        }
                    }
                    else // the pose block: predicted Pvv, row r
                    {
                        a0 = pred[5 + r];
                        a1 = pred[5 + r + 3];
                        a2 = pred[5 + r + 6];
                    }
                }
                if (r >= 3)
                {
                    P[(size_t)0 * ldp + r] = a0 - xm0;
                    P[(size_t)1 * ldp + r] = a1 - xm1;
                    P[(size_t)2 * ldp + r] = a2 - xm2;
                }
                else
                {
                    // the 3 x 3 pose block: the increment W1 W1^T is symmetric bit for bit in the reference's product;
                    // here (r, c) and (c, r) come from different dot products, so the thread of the larger index
                    // applies ITS increment to both
                    const float av[3] = {a0, a1, a2};
                    const float dv[3] = {xm0, xm1, xm2};
#pragma unroll
                    for (int c = 0; c < 3; c++)
                    {
                        if (c == r)
                        {
                            P[(size_t)c * ldp + r] = av[c] - dv[c];
                        }
                        else if (c < r)
                        {
                            const float bcr = (pred != nullptr) ? pred[5 + c + 3 * r] : P[(size_t)r * ldp + c]; // (c, r)
                            P[(size_t)c * ldp + r] = av[c] - dv[c];
                            P[(size_t)r * ldp + c] = bcr - dv[c];
                        }
                    }
                }
            }
        }
    }
