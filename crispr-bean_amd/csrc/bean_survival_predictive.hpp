// k_simulate_survival: replicate counts of the survival variant families (NormalModel, MixtureNormalModel with or
// without accessibility), drawn on the device - the posterior predictive check of a survival screen.
//
// For one draw d of the latent sites - the draw bean_hip_elbo_grad(seed, step = d) evaluates, prepared by the same
// k_set_step + PREP k_param launches (the Normal sites, the baseline u_g, the gamma draws of the Dirichlet-over-all-
// guides site and their sums, lpn) - every (replicate, guide) forms the Dirichlet-Multinomial concentrations of its
// likelihoods (X and, with the flag, X_bcmatch) over the TIMEPOINTS as k_guide_survival_wave does, then draws
//     p ~ Dirichlet(alpha),    x_rep ~ Multinomial(n_obs, p),    n_obs = sum_b x_b of the observed counts
// through dm_draw_tail (bean_predictive.hpp), the draw tail simulate_pair_body ends in: the same sites, counter layout,
// floors, log branch and inversion.  k_simulate_survival_members (at the end): K such screens in one launch, the member
// on blockIdx.y - the screens of a survival screen's parametric bootstrap.  Both kernels are simulate_survival_body.
//
//   * grid and lanes as k_guide_survival_wave: a single-wave workgroup is 64 consecutive guides of one replicate,
//     XCD-aware decode of blockIdx.x, a lane is one (replicate, guide); a lane beyond G writes nothing.
//   * pi (MixtureNormal): guide_pair_draw<FAM> - site kSitePi, subsequence r G_tot + g_off + g, offset step * 256, the
//     clamps of the guide kernel; DevArgs::pi_in is honoured, with BEAN_FLAG_DUMP_PI pi_out is written; the
//     accessibility transform with lpn is accessible_pi1, as in the sorting body.
//   * q_0 (NormalModel, surv_q0lik): x0 = float32-clamped gam / gsum[r], or gam itself with x0_in - the weight of the
//     one growth column.  x0_out is written where bound (MixtureNormal too, where the draw does not enter the
//     concentrations: drawn_noise() after the call is then wholly the noise of draw d).
//   * negative-control guides of the NormalModel: mu_t = 0.
//   * growth columns P0_b = exp(u t_b), P1_b = exp((u + mu_t) t_b); S = sum_b e_b sf_b, a0 / (S + kEps), alpha_raw with
//     the operands of k_guide_survival_wave in its order, the sample mask, the floor at kEps.
//   * masks do not enter the draw: a pair masked by repguide_mask or n <= mask_thres is simulated like any other.
//   * COST: as k_simulate_wave2 - the categorical loop runs ceil(n_obs / 4) times per lane, a wave lasts as long as its
//     largest total.
//   * LDS: [4][B] per-replicate constants (sf, sf_bc, sample mask, time) | three thread-private columns of B doubles
//     (P0, P1; concentration, then gamma, then cumulative) | one column of B floats (the counts drawn).
//     No scratch, no atomics; results leave through plain vector stores.
#pragma once

namespace bean {

__host__ __device__ inline size_t simulate_survival_lds(int B) {
    return ((size_t)4 * B + (size_t)3 * B * 64) * sizeof(double) + (size_t)B * 64 * sizeof(float);
}

// One lane of one screen: (replicate, guide) of the workgroup blockIdx.x, drawn as draw `step` into the planes of `s`.
// `first` gates the writes of pi_out (BEAN_FLAG_DUMP_PI) and x0_out: one handle has one of each.  MEMBERS: without an
// injected eps_u the baseline u_g is drawn again for draw `step` (see k_simulate_survival_members); else it is c.u_g.
template <int FAM, bool ACC, bool MEMBERS>
__device__ __forceinline__ void simulate_survival_body(const DevArgs& c, const SimArgs& s, const unsigned long long step,
                                                       const bool first, double* ssl) {
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

    // ---- the pi draw of this step and its transform: the head of k_guide_survival_wave
    double pi0 = 0.0, pi1 = 1.0, pe1 = 1.0;
    if (MIX) {
        const float api0 = c.p[4][2 * g], api1 = c.p[4][2 * g + 1];
        const double pa0 = c.pi_a0[g];
        uint4 philox_first = make_uint4(0u, 0u, 0u, 0u);
        if (!c.pi_in) philox_first = philox_block(c.seed, ((unsigned long long)kSitePi << 48) + sub, step * 256ull);
        StepCtr ctr{};
        ctr.step = step;  // all guide_pair_draw reads of it
        double cp0, cp1;
        guide_pair_draw<FAM>(c, ctr, r, g, api0, api1, pa0, &philox_first, &cp0, &cp1, pi0, pi1);
        if (c.pi_in) {
            pi0 = c.pi_in[rgi * 2];
            pi1 = c.pi_in[rgi * 2 + 1];
        }
        if (first && (c.flags & kDumpPi) && c.pi_out) {
            c.pi_out[rgi * 2] = pi0;
            c.pi_out[rgi * 2 + 1] = pi1;
        }
        pe1 = pi1;
        if (ACC) pe1 = accessible_pi1(pi1, c.kacc[g], c.lpn[g]);
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
        // the baseline: PREP's (drawn or injected), or - a member without an injected one - the draw PREP would make at
        // this member's step, with PREP's own expression (bean_param_body.hpp, the kSiteAux site)
        double u = 0.0;
        if (MIX) {
            if (!MEMBERS || c.eps_u_in) {
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
        float* out = lik ? s.xbc_out : s.x_out;
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
        for (int b = 0; b < B; ++b) {
            const double al = conc(b);
            col[b * 64] = al;
            if (s.alpha_out) s.alpha_out[(((long)lik * R + r) * B + b) * G + g] = al;
        }
        dm_draw_tail(c.seed, sub, step * 2ull + (unsigned long long)lik, B, (long)n, col, xs, conc);
#pragma unroll 1
        for (int b = 0; b < B; ++b) out[((long)r * B + b) * G + g] = xs[b * 64];
    }
}

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_simulate_survival(DevArgs c, SimArgs s) {
    extern __shared__ double ssl[];
    const StepCtr ctr = *c.ctrB;
    simulate_survival_body<FAM, ACC, false>(c, s, ctr.step, true, ssl);
}

// k_simulate_survival_members: K replicate screens of one survival fit in one launch.  gridDim.x and lanes as
// k_simulate_survival; gridDim.y = K and blockIdx.y is the member (the convention of bean_ensemble.hpp and
// k_simulate_members), so a workgroup is 64 guides of one replicate of one member.  Member k writes plane k of x_out /
// xbc_out, (K, R, B, G) float32 member-major; there is no alpha_out.
//
// WHICH DRAW IS WHOSE.  With ctrB->step = first_draw:
//   * mu_t, lpn, gam / gsum: those of the ONE PREP k_param launch (draw first_draw, or the injected values), shared by
//     the K members;
//   * the baseline u_g (MixtureNormal): with eps_u_in, c.u_g - that value for every member.  Otherwise redrawn in the
//     body for draw first_draw + k with PREP's own expression, so member 0 equals c.u_g; it is the one survival site
//     without a variational factor, so a screen of the fitted model gets its own;
//   * pi (kSitePi), the gammas (kSiteSimGamma) and the categorical draws (kSiteSimCat): draw first_draw + k wherever
//     k_simulate_survival uses ctr.step;
//   * pi_in and x0_in are every member's; member 0 alone writes pi_out (BEAN_FLAG_DUMP_PI) and x0_out.  The kernel
//     writes no u_g, eps_u or eps_u_out.
// Plane k is therefore bit for bit what k_simulate_survival leaves for draw first_draw + k when the shared sites are
// injected (and plane 0 whatever is injected).  LDS, scratch, atomics and stores as k_simulate_survival.
template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_simulate_survival_members(DevArgs c, SimArgs s) {
    extern __shared__ double ssl[];
    const StepCtr ctr = *c.ctrB;
    const unsigned member = blockIdx.y;
    const size_t plane = (size_t)member * (size_t)c.R * (size_t)c.B * (size_t)c.G;
    SimArgs sm;
    sm.x_out = s.x_out + plane;
    sm.xbc_out = s.xbc_out ? s.xbc_out + plane : nullptr;
    sm.alpha_out = nullptr;
    simulate_survival_body<FAM, ACC, true>(c, sm, ctr.step + (unsigned long long)member, member == 0, ssl);
}

}  // namespace bean
