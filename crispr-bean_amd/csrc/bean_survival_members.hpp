// k_simulate_survival_members: K replicate screens of one survival fit in one launch - the screens of a survival
// screen's parametric bootstrap.
//
// gridDim.x and lanes as k_simulate_survival (bean_survival_predictive.hpp): a single-wave workgroup is 64 consecutive
// guides of one replicate, XCD-aware decode of blockIdx.x.  gridDim.y = K and blockIdx.y is the member (the convention of
// bean_ensemble.hpp and k_simulate_members), so a workgroup is 64 guides of one replicate of one member.  Member k writes
// plane k of x_out / xbc_out, (K, R, B, G) float32 member-major; there is no alpha_out.
//
// WHICH DRAW IS WHOSE.  With ctrB->step = first_draw:
//   * mu_t, lpn, gam / gsum: those of the ONE PREP k_param launch (draw first_draw, or the injected values), shared by
//     the K members;
//   * the baseline u_g (MixtureNormal): with eps_u_in, c.u_g - that value for every member.  Otherwise redrawn here for
//     draw first_draw + k with PREP's own expression (bean_param_body.hpp, the kSiteAux site), so member 0 equals c.u_g;
//     it is the one survival site without a variational factor, so a screen of the fitted model gets its own;
//   * pi (kSitePi), the gammas (kSiteSimGamma) and the categorical draws (kSiteSimCat): draw first_draw + k wherever
//     k_simulate_survival uses ctr.step;
//   * pi_in and x0_in are every member's; member 0 alone writes pi_out (BEAN_FLAG_DUMP_PI) and x0_out.  The kernel
//     writes no u_g, eps_u or eps_u_out.
// Plane k is therefore bit for bit what k_simulate_survival leaves for draw first_draw + k when the shared sites are
// injected (and plane 0 whatever is injected).
//
// The forward lines and the draw tail are WRITTEN AGAIN in survival_members_body, which this kernel alone uses: every
// kernel that existed before this header keeps its code object byte for byte.  LDS per wave is simulate_survival_lds(B),
// laid out as in k_simulate_survival.  No scratch, no atomics; results leave through plain vector stores.
#pragma once

namespace bean {

// One lane of one member: (replicate, guide) of the workgroup blockIdx.x, drawn as draw `step` into x_out / xbc_out
// (the member's planes).  `first` is member 0: it alone writes pi_out and x0_out.
template <int FAM, bool ACC>
__device__ __forceinline__ void survival_members_body(const DevArgs& c, float* x_out, float* xbc_out,
                                                      const unsigned long long step, const bool first, double* ssl) {
    constexpr bool MIX = FAM == kMixture;
    const int lane = threadIdx.x;
    const int G = c.G, B = c.B, R = c.R;
    const int wg = blockIdx.x;
    const int kk = wg >> 3;
    const int r = kk % R;
    const int tile = (kk / R) * 8 + (wg & 7);
    if (tile * 64 >= G) return;
    const int g = tile * 64 + lane;
    const bool valid = g < G;
    const bool use_bc = (c.flags & kUseBc) != 0;
    const bool q0lik = !MIX && c.surv_q0lik;
    double* cst = ssl;                                  // [4][B]: sf, sf_bc, sample mask, time
    double* p0s = cst + 4 * B + lane;                   // exp(u t_b)          at p0s[b * 64]
    double* p1s = cst + 4 * B + B * 64 + lane;          // exp((u + mu_t) t_b) at p1s[b * 64]
    double* col = cst + 4 * B + 2 * B * 64 + lane;      // concentration, gamma, cumulative at col[b * 64]
    float* xs = (float*)(cst + 4 * B + (size_t)3 * B * 64) + lane;  // xs[b * 64]
    {
        const int kq = lane >> 3, bq = lane & 7;
        if (kq < 4) {
            const double* src = kq == 0 ? c.sf + r * B : (kq == 1 ? (use_bc ? c.sf_bc : c.sf) + r * B
                                                                  : (kq == 2 ? c.smask + r * B : c.time));
            for (int b2 = bq; b2 < B; b2 += 8) cst[kq * B + b2] = src[b2];
        }
    }
    __syncthreads();
    if (!valid) return;
    const double* c_sm = cst + 2 * B;
    const double* c_tm = cst + 3 * B;
    const long rgi = (long)r * G + g;
    const unsigned long long sub = (unsigned long long)r * c.G_tot + (c.g_off + g);

    // ---- the pi draw of this member's step and its transform: the head of k_guide_survival_wave
    double pi0 = 0.0, pi1 = 1.0, pe1 = 1.0;
    if (MIX) {
        if (c.pi_in) {
            pi0 = c.pi_in[rgi * 2];
            pi1 = c.pi_in[rgi * 2 + 1];
        } else {
            const float api0 = c.p[4][2 * g], api1 = c.p[4][2 * g + 1];
            const double pa0 = c.pi_a0[g];
            uint4 philox_first = philox_block(c.seed, ((unsigned long long)kSitePi << 48) + sub, step * 256ull);
            const double al0 = (double)expf(api0), al1 = (double)expf(api1);
            const double rs = frcp(al0 + al1) * pa0;
            const double cp0 = al0 * rs, cp1 = al1 * rs;
            const double cq0 = cp0 < 1e-5 ? 1e-5 : cp0, cq1 = cp1 < 1e-5 ? 1e-5 : cp1;
            Rng rng(c.seed, kSitePi, sub, step * 256ull);
            const GammaPair gp = sample_gamma_pair_inl(cq0, cq1, rng, &philox_first);
            const double gm0 = fmax(gp.g0, kDblMin), gm1 = fmax(gp.g1, kDblMin);
            const double rs2 = frcp(gm0 + gm1);
            pi0 = fmin(fmax(gm0 * rs2, kDblMin), kOneMinus);
            pi1 = fmin(fmax(gm1 * rs2, kDblMin), kOneMinus);
        }
        if (first && (c.flags & kDumpPi) && c.pi_out) {
            c.pi_out[rgi * 2] = pi0;
            c.pi_out[rgi * 2 + 1] = pi1;
        }
        pe1 = pi1;
        if (ACC) {
            const double kacc = c.kacc[g];
            const double s1 = pi1 * kacc;
            const double p1c = fmin(fmax(s1, 1e-3), 1.0 - 1e-3);
            const double l = flog(p1c * frcp(1.0 - p1c)) + c.lpn[g];
            const double el = exp(l);
            const double pn = el * frcp(1.0 + el);
            pe1 = fmin(fmax(pn, 1e-3), 1.0 - 1e-3);
        }
    }
    // ---- the draw of the Dirichlet-over-all-guides site: float32 semantics of torch's sampler
    double x0 = 1.0;
    if (MIX || q0lik) {
        const double gam = c.gam[rgi];
        x0 = c.x0_in ? gam : (double)fminf(fmaxf((float)(gam * frcp(c.gsum[r])), 1.17549435e-38f), 0.99999994f);
        if (first && c.x0_out) c.x0_out[rgi] = x0;
    }
    // ---- growth of the two components over the timepoints
    {
        double mu_t = c.mu_t[c.g2t[g]];
        // survival NormalModel: mu of negative-control guides is forced to 0
        if (q0lik && c.negctrl && c.negctrl[g] != 0) mu_t = 0.0;
        // the baseline of this member: the injected one, or the draw PREP would make at this member's step
        double u = 0.0;
        if (MIX) {
            if (c.eps_u_in) {
                u = c.u_g[g];
            } else {
                const double eps = (double)normal2_at(c.seed, ((unsigned long long)kSiteAux << 48) + (unsigned long long)(c.g_off + g),
                                                      step * 4ull).x;
                u = (double)(float)c.neg_loc + eps * (double)(float)c.neg_scale;
            }
        }
        const double mu1 = u + mu_t;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const double tb = c_tm[b];
            p1s[b * 64] = exp(mu1 * tb);
            if (MIX) p0s[b * 64] = exp(u * tb);
        }
    }
    // weights of the two growth columns in e_b = w0 P0_b + w1 P1_b
    const double w0 = MIX ? (ACC ? 1.0 - pe1 : pi0) : 0.0;
    const double w1 = MIX ? (ACC ? pe1 : pi1) : (q0lik ? x0 : 1.0);
    const double epsB = kEps / (double)B;

#pragma unroll 1
    for (int lik = 0; lik < 2; ++lik) {
        if (lik == 1 && !use_bc) break;
        const float* X = lik ? c.Xbc : c.X;
        float* out = lik ? xbc_out : x_out;
        const double* sf = cst + lik * B;
        const double a0 = lik ? c.a0_bc[g] : c.a0[g];
        double S = 0.0, n = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            S += fma(w0, MIX ? p0s[b * 64] : 0.0, w1 * p1s[b * 64]) * sf[b];
            n += (double)X[((long)r * B + b) * G + g];
        }
        const double inv = frcp(S + kEps);
        const double ai = a0 * inv;
        const auto conc = [&](int b) {
            const double ar = alpha_raw(w0, MIX ? p0s[b * 64] : 0.0, w1, p1s[b * 64], sf[b], epsB, ai * c_sm[b]);
            return ar < kEps ? kEps : ar;
        };
#pragma unroll 1
        for (int b = 0; b < B; ++b) col[b * 64] = conc(b);
        // ---- p ~ Dirichlet(alpha): gammas two bins at a time, then the cumulative
        const unsigned long long dl = step * 2ull + (unsigned long long)lik;
        double gsum = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; b += 2) {
            const bool two = b + 1 < B;
            const double al0 = col[b * 64], al1 = two ? col[(b + 1) * 64] : 1.0;
            Rng rng(c.seed, kSiteSimGamma, sub, (dl * kSimPairSlots + (unsigned long long)(b >> 1)) * kSimGammaWords);
            const GammaPair gp = sample_gamma_pair_inl(al0, al1, rng);
            const double gm0 = fmax(gp.g0, kDblMin);
            col[b * 64] = gm0;
            gsum += gm0;
            if (two) {
                const double gm1 = fmax(gp.g1, kDblMin);
                col[(b + 1) * 64] = gm1;
                gsum += gm1;
            }
        }
        double rs = frcp(gsum);
        if (gsum < kSimLogBelow) {
            // every gamma at or near the kDblMin floor: the same draws again in logs, from the same counters (the
            // boost's block first, then the rounds), less their maximum - see simulate_pair_body
            double mx = -INFINITY;
#pragma unroll 1
            for (int b = 0; b < B; b += 2) {
                const bool two = b + 1 < B;
                const double al0 = conc(b), al1 = two ? conc(b + 1) : 1.0;
                const bool lo0 = al0 < 1.0, lo1 = al1 < 1.0;
                const unsigned long long off = (dl * kSimPairSlots + (unsigned long long)(b >> 1)) * kSimGammaWords;
                Rng rng(c.seed, kSiteSimGamma, sub, off + ((lo0 || lo1) ? 4ull : 0ull));
                const uint4 ub = philox_block(c.seed, rng.sub, off);
                const GammaPair gp = sample_gamma_pair_inl(lo0 ? al0 + 1.0 : al0, lo1 ? al1 + 1.0 : al1, rng);
                const double lg0 = log(gp.g0) + (lo0 ? log(Rng::to_unit(ub.x, ub.y)) / al0 : 0.0);
                col[b * 64] = lg0;
                mx = fmax(mx, lg0);
                if (two) {
                    const double lg1 = log(gp.g1) + (lo1 ? log(Rng::to_unit(ub.z, ub.w)) / al1 : 0.0);
                    col[(b + 1) * 64] = lg1;
                    mx = fmax(mx, lg1);
                }
            }
            gsum = 0.0;
#pragma unroll 1
            for (int b = 0; b < B; ++b) {
                const double w = exp(col[b * 64] - mx);
                col[b * 64] = w;
                gsum += w;
            }
            rs = 1.0 / gsum;
        }
        double cum = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            cum += col[b * 64] * rs;
            col[b * 64] = cum;
            xs[b * 64] = 0.f;
        }
        // ---- x_rep ~ Multinomial(n, p): four categorical draws per Philox block
        const long n_i = (long)n;
        const long n_blk = (n_i + 3) >> 2;
        const unsigned long long cat_sub = ((unsigned long long)kSiteSimCat << 48) + sub;
        const unsigned long long cat_off = dl * kSimCatWords;
#pragma unroll 1
        for (long t = 0; t < n_blk; ++t) {
            const uint4 w = philox_block(c.seed, cat_sub, cat_off + 4ull * (unsigned long long)t);
            const double u0 = ((double)w.x + 0.5) * 2.3283064365386963e-10;
            const double u1 = ((double)w.y + 0.5) * 2.3283064365386963e-10;
            const double u2 = ((double)w.z + 0.5) * 2.3283064365386963e-10;
            const double u3 = ((double)w.w + 0.5) * 2.3283064365386963e-10;
            int k0 = 0, k1 = 0, k2 = 0, k3 = 0;
#pragma unroll 1
            for (int b = 0; b < B - 1; ++b) {
                const double cb = col[b * 64];
                k0 += u0 >= cb ? 1 : 0;
                k1 += u1 >= cb ? 1 : 0;
                k2 += u2 >= cb ? 1 : 0;
                k3 += u3 >= cb ? 1 : 0;
            }
            const long rem = n_i - 4 * t;
            xs[k0 * 64] += 1.f;
            if (rem > 1) xs[k1 * 64] += 1.f;
            if (rem > 2) xs[k2 * 64] += 1.f;
            if (rem > 3) xs[k3 * 64] += 1.f;
        }
#pragma unroll 1
        for (int b = 0; b < B; ++b) out[((long)r * B + b) * G + g] = xs[b * 64];
    }
}

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_simulate_survival_members(DevArgs c, SimArgs s) {
    extern __shared__ double ssm[];
    const StepCtr ctr = *c.ctrB;
    const unsigned member = blockIdx.y;
    const size_t plane = (size_t)member * (size_t)c.R * (size_t)c.B * (size_t)c.G;
    survival_members_body<FAM, ACC>(c, s.x_out + plane, s.xbc_out ? s.xbc_out + plane : nullptr,
                                    ctr.step + (unsigned long long)member, member == 0, ssm);
}

}  // namespace bean
