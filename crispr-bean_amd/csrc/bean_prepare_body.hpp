// The body of k_prepare (bean_kernels.hpp) and of k_prepare_ens (bean_ensemble.hpp): NOT a header of its own - it is
// included INSIDE a kernel that has `DevArgs c` in scope.  Kept as text, like bean_param_body.hpp, so that the single-fit
// kernel stays, token for token, what it was before the per-member form existed.
#ifndef BEAN_PREPARE_BODY_INCLUDED_BY_KERNEL
#error "bean_prepare_body.hpp is the text of a kernel body: include it from inside k_prepare / k_prepare_ens only"
#endif
    __shared__ double scratch[16];
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n_rg = (long)c.R * c.G;
    double v = 0.0;
    if (idx < n_rg) {
        const int r = (int)(idx / c.G), g = (int)(idx % c.G);
        const bool rgm = c.rg[idx] != 0;
        double n = 0.0, lf = 0.0, nb = 0.0, lfb = 0.0;
        for (int b = 0; b < c.B; ++b) {
            const double x = (double)c.X[((long)r * c.B + b) * c.G + g];
            n += x;
            lf += lgamma(1.0 + x);
            if (c.flags & kUseBc) {
                const double y = (double)c.Xbc[((long)r * c.B + b) * c.G + g];
                nb += y;
                lfb += lgamma(1.0 + y);
            }
        }
        if (rgm && n > (double)c.mask_thres) v -= lgamma(1.0 + n) - lf;
        if ((c.flags & kUseBc) && rgm && nb > (double)c.mask_thres) v -= lgamma(1.0 + nb) - lfb;
        if (c.tot_const) {
            if (rgm && n > (double)c.mask_thres) v += lgamma_digamma_diff(c.a0[g], n).d;
            if ((c.flags & kUseBc) && rgm && nb > (double)c.mask_thres) v += lgamma_digamma_diff(c.a0_bc[g], nb).d;
        }
        if (c.wrow && r == 0) {
            // wave forms: per-guide count of unmasked replicates (the kPNrg row is data)
            double cnt = 0.0;
            for (int rr = 0; rr < c.R; ++rr) cnt += c.rg[(long)rr * c.G + g] != 0 ? 1.0 : 0.0;
            c.part[(long)kPNrg * c.G + g] = cnt;
        }
        if (c.nobs) {
            c.nobs[idx] = (rgm && n > (double)c.mask_thres) ? n : -1.0;
            c.nobs[n_rg + idx] = ((c.flags & kUseBc) && rgm && nb > (double)c.mask_thres) ? nb : -1.0;
        }
        if ((c.family == kMixture || c.family == kMultiMixture) && rgm) {
            for (int cc = 0; cc < c.C; ++cc) {
                double tot = 0.0, l = 0.0;
                for (int a = 0; a < c.A; ++a) {
                    const double y = (double)c.allele[(((long)r * c.C + cc) * c.G + g) * c.A + a];
                    tot += y;
                    l += lgamma(1.0 + y);
                }
                v -= lgamma(1.0 + tot) - l;
            }
        }
    }
    const double tot = block_sum(v, scratch);
    if (threadIdx.x == 0) fixed_add(c.const_acc, tot);
    if (blockIdx.x == 0 && (int)threadIdx.x < c.B && !c.survival) {
        const double zh = c.z_hi[threadIdx.x], zl = c.z_lo[threadIdx.x];
        const double ch = isinf(zh) ? 1.0 : norm_cdf(zh);
        const double cl = isinf(zl) ? 0.0 : norm_cdf(zl);
        c.P0[threadIdx.x] = ch - cl;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && c.ue_z && !c.survival) {
        int n = 0;
        for (int k = 0; k < 2 * c.B; ++k) {
            const double z = k < c.B ? c.z_hi[k] : c.z_lo[k - c.B];
            int idx = -1;
            if (!isinf(z)) {
                for (int q = 0; q < n; ++q)
                    if (c.ue_z[q] == z) idx = q;
                if (idx < 0) {
                    idx = n;
                    c.ue_z[n++] = z;
                }
            }
            c.ue_idx[k] = idx;
        }
        c.ue_idx[2 * c.B] = n;
    }
