// ekf_panel_mfma_f64_body.inc -- the statements of ekf_panel_mfma_f64<SUB, XUPD> (see there for what they do), kept apart so that the
// counted entry of ekf_counted_kernels.hpp, which reads the observation count from device memory, is built from the
// same text: included inside a function that has the kernel's parameters (and template parameters) in scope.
    // pred != nullptr (gain, XUPD): commits a predict() that the gather and factor kernels applied on the fly, exactly as
    // ekf_panel_mfma_f32 does: pred = {g02, g12, pose (3), Pvv (9)} from the gather kernel.
    const int  lane = threadIdx.x;
    const int  lj   = lane & 15;
    const int  lq   = lane >> 4;
    const int  row0 = blockIdx.x * 16;
    const int  c0   = blockIdx.y * 16;
    const bool cok  = (c0 + lj) < nc;
    const int  cc   = cok ? (c0 + lj) : (nc - 1);
    const bool dox  = XUPD && (blockIdx.y == 0);
    f64x4      acc  = {0.0, 0.0, 0.0, 0.0};
    double     xs = 0.0, xm0 = 0.0, xm1 = 0.0, xm2 = 0.0;
    const double* pa = A + row0 + lj;
    double oldv[4];
    if (SUB)
    {
#pragma unroll
        for (int g = 0; g < 4; g++)
        {
            const int col = c0 + lq + 4 * g;
            oldv[g]       = OUT[(size_t)(col < nc ? col : nc - 1) * ldo + row0 + lj];
        }
    }
    constexpr int NQ = 16; // k-quads per trip: every load of the trip is issued before its first MFMA
    for (int qb = 0; qb < kq; qb += 4 * NQ)
    {
        double b[NQ], g[NQ], uq[NQ], m0[NQ], m1[NQ], m2[NQ];
#pragma unroll
        for (int t = 0; t < NQ; t++)
        {
            const int q  = qb + 4 * t + lq;
            const int qc = (q < kq) ? q : (kq - 1);
            b[t]         = pa[(size_t)qc * lda];
            g[t]         = Bt[(size_t)qc * ldb + cc];
            uq[t]        = (XUPD && dox) ? u[qc] : 0.0;
            if (XUPD && dox && Mv != nullptr)
            {
                m0[t] = Mv[qc];
                m1[t] = Mv[kq + qc];
                m2[t] = Mv[2 * kq + qc];
            }
            else
            {
                m0[t] = m1[t] = m2[t] = 0.0;
            }
        }
#pragma unroll
        for (int t = 0; t < NQ; t++)
        {
            const int    q  = qb + 4 * t + lq;
            const bool   ok = q < kq;
            const double gg = (ok && cok) ? g[t] : 0.0;
            const double bb = ok ? b[t] : 0.0;
            acc             = __builtin_amdgcn_mfma_f64_16x16x4f64(gg, bb, acc, 0, 0, 0);
            xs += bb * uq[t];
            xm0 += bb * m0[t];
            xm1 += bb * m1[t];
            xm2 += bb * m2[t];
        }
    }
#pragma unroll
    for (int g = 0; g < 4; g++)
    {
        const int col = c0 + lq + 4 * g;
        if (col < nc)
        {
            double* o = OUT + (size_t)col * ldo + row0 + lj;
            if (!SUB && Mv != nullptr && row0 + lj < 3) // pose rows of the W1 panel: kept aside, stored as zero
            {
                wv_out[(size_t)(row0 + lj) * nc + col] = acc[g];
                *o                                     = 0.0;
            }
            else
            {
                *o = SUB ? (oldv[g] - acc[g]) : acc[g];
            }
        }
    }
    if (dox)
    {
        xs += __shfl_xor(xs, 16);
        xs += __shfl_xor(xs, 32);
        xm0 += __shfl_xor(xm0, 16);
        xm0 += __shfl_xor(xm0, 32);
        xm1 += __shfl_xor(xm1, 16);
        xm1 += __shfl_xor(xm1, 32);
        xm2 += __shfl_xor(xm2, 16);
        xm2 += __shfl_xor(xm2, 32);
        const int r = row0 + lj;
        if (lq == 0 && r < n)
        {
            X[r] = ((pred != nullptr && r < 3) ? pred[2 + r] : X[r]) + xs;
            if (pred != nullptr || Mv != nullptr)
            {
                // row r of the pose stripe: [predicted (EKF.cpp:439-443)] then [downdated] (xm* are zero without Mv)
                double a0 = Pv[(size_t)0 * ldp + r], a1 = Pv[(size_t)1 * ldp + r], a2 = Pv[(size_t)2 * ldp + r];
                if (pred != nullptr)
                {
                    if (r >= 3)
                    {
                        if (r - 3 < pred_w)
                        {
                            double o0, o1, o2;
                            predict_stripe_col<double>(pred[0], pred[1], a0, a1, a2, &o0, &o1, &o2);
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
                    Pv[(size_t)0 * ldp + r] = a0 - xm0;
                    Pv[(size_t)1 * ldp + r] = a1 - xm1;
                    Pv[(size_t)2 * ldp + r] = a2 - xm2;
                }
                else // the 3 x 3 pose block: one increment for (r, c) and (c, r) (see ekf_panel_mfma_f32)
                {
                    const double av[3] = {a0, a1, a2};
                    const double dv[3] = {xm0, xm1, xm2};
#pragma unroll
                    for (int c = 0; c < 3; c++)
                    {
                        if (c == r)
                        {
                            Pv[(size_t)c * ldp + r] = av[c] - dv[c];
                        }
                        else if (c < r)
                        {
                            const double bcr = (pred != nullptr) ? pred[5 + c + 3 * r] : Pv[(size_t)r * ldp + c]; // (c, r)
                            Pv[(size_t)c * ldp + r] = av[c] - dv[c];
                            Pv[(size_t)r * ldp + c] = bcr - dv[c];
                        }
                    }
                }
            }
        }
    }
