// ekf_gather_kernel_body.inc -- the statements of ekf_gather_kernel<T, KC, OBS> (see there for what they do), kept apart so that the
// counted entry of ekf_counted_kernels.hpp, which reads the observation count from device memory, is built from the
// same text: included inside a function that has the kernel's parameters (and template parameters) in scope.
    // Yout (kc > KC, the template bound): the pending panels are too many to correct for here: this kernel only publishes
    // Y = H*Wc (k x kc, Y[q*k + row]) -- with the coefficients of the (possibly predicted) pose it has anyway -- and the
    // MFMA panel kernel applies PHT -= Wc*Y^T behind it.
    if (flags != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < m)
    {
        const int id = idf[threadIdx.x];
        if (id < 1 || id > ((n - 3) >> 1))
        {
            atomicOr(&flags[0], kFlagBadIdf);
        }
    }
    // Wc / kc (kc <= KC): a FEW pending columns (heading observations: rank-1 columns, ekf_pose_step_kernel)
    // are corrected for right here -- PHT = Ps*H^T - Wc*(H*Wc)^T with H*Wc built per workgroup from the two landmark
    // rows of Wc (its pose rows are zero) -- so that the update keeps its fast path (compact block, fused predict)
    // instead of going through the separate correction kernels.
    // pp.valid: a predict() is pending (see PredictArgs): this kernel works on the PREDICTED pose and pose rows of P,
    // formed on the fly from the stored ones (which the gain kernel replaces afterwards); nothing is written to X or P.
    // sub (optional, m <= 32): the (3 + 2m) x 2m block of PHT that S = H*PHT reads -- rows 0,1,2 and the two rows
    // of every observed landmark -- stored compactly as sub[slot*2m + col] (slot 3+2o+a <-> row fx_o + a), so that
    // the one-workgroup factor kernel loads 17 KB of contiguous data instead of 2000 scattered cache lines.
    __shared__ T   s_coef[OBS * 10];
    __shared__ int s_fx[OBS];
    __shared__ int s_idf[32];
    int            o0 = blockIdx.y * OBS;
    int            no = min(OBS, m - o0);
    __shared__ unsigned s_cand; // observations whose landmark rows fall into this block's 256 rows
    if (sub != nullptr && threadIdx.x == 0)
    {
        s_cand = 0u;
    }
    // Everything this thread reads from P depends on the landmark ids only, not on the observation model: it is
    // requested here, so that the P round trip and the idf -> X -> atan2 chain of the model below run side by side
    // instead of one after the other (the kernel is a chain of dependent round trips, nothing else).
    const int i  = blockIdx.x * 256 + threadIdx.x;
    const int il = min(i, n - 1); // (rows past n: clamped loads, no stores)
    int       fxe[OBS];
    T         ea[OBS], eb[OBS];
    T         sa[OBS][3], sb[OBS][3]; // pp.valid, i < 3: rows 0..2 of the landmark's two columns
    T         Pvv[9];
    const T   phi_old = X[2];
#pragma unroll
    for (int oo = 0; oo < OBS; oo++)
    {
        fxe[oo] = 3 + 2 * clamp_idf(idf[o0 + min(oo, no - 1)], n) - 2; // as observe_model_pose
        ea[oo]  = p_get<T>(P, Pv, ldp, il, fxe[oo], lower);
        eb[oo]  = p_get<T>(P, Pv, ldp, il, fxe[oo] + 1, lower);
    }
    T p0 = Pv[(size_t)0 * ldp + il], p1 = Pv[(size_t)1 * ldp + il], p2 = Pv[(size_t)2 * ldp + il];
    T wc[KC];
#pragma unroll
    for (int q = 0; q < KC; q++)
    {
        wc[q] = (q < kc && Yout == nullptr) ? Wc[(size_t)q * ldwc + il] : (T)0;
    }
    __shared__ T s_y[OBS][2][KC];
    // (kc > 0, in-kernel correction) the two landmark rows of pending column q that thread (oo, q) turns into Y below:
    // requested here with everything else (the landmark id fixes the rows)
    T         ywa = (T)0, ywb = (T)0;
    const int yoo = threadIdx.x / KC, yq = threadIdx.x % KC;
    if (kc > 0 && Yout == nullptr && yoo < no && yq < kc)
    {
        const int fy = 3 + 2 * clamp_idf(idf[o0 + yoo], n) - 2;
        ywa          = Wc[(size_t)yq * ldwc + fy];
        ywb          = Wc[(size_t)yq * ldwc + fy + 1];
    }
    if (pp.valid && i < 3)
    {
        for (int cc = 0; cc < 3; cc++)
        {
            for (int r = 0; r < 3; r++)
            {
                Pvv[r + 3 * cc] = Pv[(size_t)cc * ldp + r];
            }
        }
#pragma unroll
        for (int oo = 0; oo < OBS; oo++)
        {
            for (int r = 0; r < 3; r++)
            {
                sa[oo][r] = Pv[(size_t)r * ldp + fxe[oo]];
                sb[oo][r] = Pv[(size_t)r * ldp + fxe[oo] + 1];
            }
        }
    }
    if ((int)threadIdx.x < no)
    {
        T v[2];
        int o = o0 + threadIdx.x;
        T px, py, pphi;
        predicted_pose<T>(pp, X, &px, &py, &pphi);
        observe_model_pose<T>(X, n, idf[o], Z[2 * o], Z[2 * o + 1], px, py, pphi, &s_coef[threadIdx.x * 10], v,
                              &s_fx[threadIdx.x]);
    }
    if (sub != nullptr)
    {
        __syncthreads(); // s_cand = 0 above
        if ((int)threadIdx.x < m && threadIdx.x < 32)
        {
            const int id        = clamp_idf(idf[threadIdx.x], n);
            s_idf[threadIdx.x]  = id;
            const int fxo       = 3 + 2 * id - 2; // first state row of that landmark
            const int i0        = blockIdx.x * 256;
            if (fxo + 1 >= i0 && fxo < i0 + 256)
            {
                atomicOr(&s_cand, 1u << threadIdx.x);
            }
        }
    }
    __syncthreads();
    if (Yout != nullptr && blockIdx.x == 0) // (workgroup-uniform) one workgroup per observation publishes its two rows of Y
    {
        for (int e = threadIdx.x; e < no * kc; e += 256)
        {
            const int oo = e / kc, q = e - oo * kc;
            const T*  c  = &s_coef[oo * 10];
            const T   wa = Wc[(size_t)q * ldwc + s_fx[oo]], wb = Wc[(size_t)q * ldwc + s_fx[oo] + 1];
            T         y0 = c[3] * wa;
            y0 += c[4] * wb;
            T y1 = c[8] * wa;
            y1 += c[9] * wb;
            if (sgn != nullptr && sgn[q] != 0)
            {
                y0 = -y0;
                y1 = -y1;
            }
            Yout[(size_t)q * (2 * m) + 2 * (o0 + oo)]     = y0;
            Yout[(size_t)q * (2 * m) + 2 * (o0 + oo) + 1] = y1;
        }
    }
    if (kc > 0 && Yout == nullptr) // (workgroup-uniform)
    {
        // Y = H*Wc for this workgroup's observations: only the landmark columns of H meet non-zero rows of Wc
        if ((int)threadIdx.x < no * KC)
        {
            const int oo = yoo, q = yq;
            T         y0 = (T)0, y1 = (T)0;
            if (q < kc)
            {
                const T* c  = &s_coef[oo * 10];
                const T  wa = ywa, wb = ywb;
                y0          = c[3] * wa;
                y0 += c[4] * wb;
                y1 = c[8] * wa;
                y1 += c[9] * wb;
                if (sgn != nullptr && sgn[q] != 0)
                {
                    y0 = -y0;
                    y1 = -y1;
                }
            }
            s_y[oo][0][q] = y0;
            s_y[oo][1][q] = y1;
        }
        __syncthreads();
    }
    if (i >= n)
    {
        return;
    }
    T g02 = (T)0, g12 = (T)0;
    if (pp.valid)
    {
        predict_gv<T>(pp, phi_old, &g02, &g12);
        if (i >= 3)
        {
            if (i - 3 < pp.w) // column i of the stripe (= row i of the pose columns, by symmetry)
            {
                T o0, o1, o2;
                predict_stripe_col<T>(g02, g12, p0, p1, p2, &o0, &o1, &o2);
                p0 = o0;
                p1 = o1;
                p2 = o2;
            }
        }
        else // row i of Pvv
        {
            T out[9];
            predict_pvv<T>(pp, phi_old, Pvv, out);
            p0 = out[i];
            p1 = out[i + 3];
            p2 = out[i + 6];
            if (pred_out != nullptr && i == 0 && blockIdx.y == 0)
            {
                // for the factor kernel (predicted pose) and the gain kernel (which commits the predict without racing
                // on X[2]): {g02, g12, predicted pose (3), predicted Pvv (9)}
                T px, py, pphi;
                predicted_pose<T>(pp, X, &px, &py, &pphi);
                pred_out[0] = g02;
                pred_out[1] = g12;
                pred_out[2] = px;
                pred_out[3] = py;
                pred_out[4] = pphi;
                for (int e = 0; e < 9; e++)
                {
                    pred_out[5 + e] = out[e];
                }
            }
        }
    }
    unsigned hit = 0; // observations whose landmark owns row i
    if (sub != nullptr && i >= 3)
    {
        const int lm1 = ((i - 3) >> 1) + 1; // 1-based landmark id of row i
        unsigned  cc  = s_cand;
        while (cc)
        {
            const int o = __builtin_ctz(cc);
            hit |= (s_idf[o] == lm1) ? (1u << o) : 0u;
            cc &= cc - 1;
        }
    }
#pragma unroll
    for (int oo = 0; oo < OBS; oo++)
    {
        if (oo >= no)
        {
            break;
        }
        const T* c  = &s_coef[oo * 10];
        int      fx = fxe[oo];
        T        a  = ea[oo];
        T        b  = eb[oo];
        if (pp.valid && i < 3) // pose rows of the landmark's two columns: elements of the predicted stripe
        {
            T o[3];
            if (fx - 3 < pp.w)
            {
                predict_stripe_col<T>(g02, g12, sa[oo][0], sa[oo][1], sa[oo][2], &o[0], &o[1], &o[2]);
                a = o[i];
            }
            if (fx + 1 - 3 < pp.w)
            {
                predict_stripe_col<T>(g02, g12, sb[oo][0], sb[oo][1], sb[oo][2], &o[0], &o[1], &o[2]);
                b = o[i];
            }
        }
        // same summation order as the dense product: columns 0,1,2,fx,fx+1 ascending
        T s0 = p0 * c[0];
        s0 += p1 * c[1];
        s0 += p2 * c[2];
        s0 += a * c[3];
        s0 += b * c[4];
        T s1 = p0 * c[5];
        s1 += p1 * c[6];
        s1 += p2 * c[7];
        s1 += a * c[8];
        s1 += b * c[9];
        if (kc > 0 && Yout == nullptr)
        {
            T c0 = (T)0, c1 = (T)0;
#pragma unroll
            for (int q = 0; q < KC; q++)
            {
                c0 += wc[q] * s_y[oo][0][q];
                c1 += wc[q] * s_y[oo][1][q];
            }
            s0 -= c0;
            s1 -= c1;
        }
        int col = 2 * (o0 + oo);
        PHT[(size_t)col * ldw + i]       = s0;
        PHT[(size_t)(col + 1) * ldw + i] = s1;
        if (sub != nullptr)
        {
            const int k = 2 * m;
            if (i < 3)
            {
                sub[i * k + col]     = s0;
                sub[i * k + col + 1] = s1;
            }
            unsigned hh = hit;
            while (hh)
            {
                const int o    = __builtin_ctz(hh);
                const int slot = 3 + 2 * o + ((i - 3) & 1);
                sub[slot * k + col]     = s0;
                sub[slot * k + col + 1] = s1;
                hh &= hh - 1;
            }
        }
    }
