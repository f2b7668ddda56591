// k_logw_consts + k_logw_pairs + k_logw_targets: log p(x, z) - log q(z) of S draws from the fitted guide, PER TARGET (importance-sampling
// check of the mean-field posterior: PSIS k-hat and importance-corrected moments, model/importance.py).
//
// In the sorting variant families the targets share no parameter, so the log weight of a draw is a sum over targets:
//     logw[d, t] = log p(mu_t) - log q(mu_t) + log p(sd_t) - log q(sd_t)
//                + sum over the target's guides g: (+Acc) log p(noise_g) - log q(noise_g), the Dirichlet normalisers of
//                  the pi site, nrg (log p side) and R (log q side) of them
//                + sum over replicates r and the target's guides g: the pair's likelihood terms and pi-site terms,
// and  - sum_t logw[d, t]  is the loss bean_hip_elbo_grad(seed, step = d) reports (its data-only constant included).
//
// Draw d is the draw bean_hip_elbo_grad(seed, step = d) evaluates - same sites, counters, operands and bits - formed by
// the lanes themselves: no k_set_step / PREP launch per draw, no Phi table in memory, nothing of the workspace written.
//   * target sites: normal2_at(seed, kSiteTarget..., d * 4) -> tgt_draw, as the PREP branch of k_param forms mu_t, y_t;
//   * table entries: phi_inv_sigma / planted_phi_entry at the lane's own (mu_t, y_t) - the route of k_simulate_power;
//   * pi: guide_pair_draw<FAM> with ctr.step = d;
//   * +Acc: the noise site as param_guide_mix PREP draws lpn (site kSiteNoise, offset d * 4), fitted or prior noise;
//   * DevArgs::eps_mu_in / eps_sd_in / pi_in / eps_noise_in are honoured as the simulators honour them: every draw of a
//     call is then the same draw.
// No new RNG site and no new counter window: the layout next to RngSite (bean_special.hpp) is unchanged.
//
// k_logw_consts: the count-only constants of a pair - the multinomial coefficients k_prepare adds up once for the whole
// screen; here they must be split per target - are data and the same for every draw: formed ONCE per call, one lane per
// (replicate, guide), and stored into the pair's slot of every draw's plane of pair_out.
//
// k_logw_pairs<FAM, ACC>: grid of k_simulate_members (gridDim.x padded tiles x R, XCD-aware decode; blockIdx.y = j is
// draw first_draw + j), a lane is one (replicate, guide) of one draw.  It adds the pair's terms - exactly what
// guide_pair_math adds to nll, with the opposite sign; the total term lgamma(A0 + n) - lgamma(A0) is evaluated at the
// pair's own A0 whether DevArgs::tot_const is set or not - to the constant it finds in ITS OWN slot pair_out[(j, r, g)]
// (no other lane reads or writes that slot); the lane with r = 0 that owns its target's first guide also stores
// mu_out / y_out[(j, t)].
// LDS as simulate_wave2_lds: [4][B] per-bin constants | [B][64] doubles, the lane's table entries | [B][64] floats, the
// counts of the likelihood at hand.  No scratch, no atomics; plain vector stores.
//
// k_logw_targets: one lane per (draw, target); adds the target's pair terms in a fixed order (replicate outer, guide
// inner), its own two sites with tgt_prior_terms' operations (--prior-params priors included), and its guides' per-guide
// terms; stores logw_out[(j, t)].
#pragma once

namespace bean {

struct LogwArgs {
    unsigned long long first_draw;
    int n_draws;
    double* logw_out;  // (n_draws, T)
    double* mu_out;    // (n_draws, T)
    double* y_out;     // (n_draws, T) or null
    double* pair_out;  // (n_draws, R, G)
};

struct LogwTarget {
    double eps1, eps2, mu, y;
};
// the target sites of draw d: what k_param's PREP branch leaves in eps_mu, eps_sd, mu_t, y_t
__device__ __forceinline__ LogwTarget logw_target_draw(const DevArgs& c, int t, unsigned long long d) {
    LogwTarget o;
    if (c.eps_mu_in) {
        o.eps1 = c.eps_mu_in[t];
        o.eps2 = c.eps_sd_in[t];
    } else {
        const float2 nrm = normal2_at(c.seed, ((unsigned long long)kSiteTarget << 48) + (unsigned long long)(c.t_off + t),
                                      d * 4ull);
        o.eps1 = (double)nrm.x;
        o.eps2 = (double)nrm.y;
    }
    o.mu = tgt_draw(c.p[0][t], o.eps1, c.p[1][t]);
    o.y = tgt_draw(c.p[2][t], o.eps2, c.p[3][t]);
    return o;
}
// the guide-noise site of draw d (+Acc): eps, the guide's scale and lpn as param_guide_mix PREP forms them
__device__ __forceinline__ void logw_noise_draw(const DevArgs& c, int g, unsigned long long d, double& eps, double& ns,
                                                double& lpn) {
#pragma clang fp contract(off)
    const bool fit_noise = (c.flags & kFitNoise) != 0;
    if (c.eps_noise_in) {
        eps = c.eps_noise_in[g];
    } else {
        eps = (double)normal2_at(c.seed, ((unsigned long long)kSiteNoise << 48) + (unsigned long long)(c.g_off + g),
                                 d * 4ull).x;
    }
    ns = fit_noise ? exp((double)c.p[6][g]) : kPiNoiseSd;
    lpn = (fit_noise ? (double)c.p[5][g] : 0.0) + eps * ns;
}

constexpr int kLogwBlock = 256;

// lgamma(1 + x) of a count
__device__ __forceinline__ double logw_lfact(double x) { return lgamma_digamma_diff(1.0, x).d; }

__global__ __launch_bounds__(kLogwBlock)
void k_logw_consts(DevArgs c, LogwArgs a) {
    const long idx = (long)blockIdx.x * kLogwBlock + threadIdx.x;
    const int G = c.G, B = c.B, R = c.R;
    if (idx >= (long)R * G) return;
    const int r = (int)(idx / G), g = (int)(idx - (long)r * G);
    const bool rgm = c.rg[idx] != 0;
    double v = 0.0;
    for (int lik = 0; lik < 2; ++lik) {
        if (lik == 1 && !(c.flags & kUseBc)) break;
        const float* X = lik ? c.Xbc : c.X;
        double n = 0.0, lf = 0.0;
        for (int b = 0; b < B; ++b) {
            const double x = (double)X[((long)r * B + b) * G + g];
            n += x;
            lf += logw_lfact(x);
        }
        // the mask of the site, as k_logw_pairs forms it (n is a sum of integers: exact in any order)
        if (rgm && n > (double)c.mask_thres) v += logw_lfact(n) - lf;
    }
    if (c.family == kMixture && rgm) {
        for (int cc = 0; cc < c.C; ++cc) {
            const float* al = c.allele + (((long)r * c.C + cc) * G + g) * 2;
            const double y0 = (double)al[0], y1 = (double)al[1];
            v += logw_lfact(y0 + y1) - logw_lfact(y0) - logw_lfact(y1);
        }
    }
    for (int j = 0; j < a.n_draws; ++j) a.pair_out[((size_t)j * R + r) * G + g] = v;
}

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_logw_pairs(DevArgs c, LogwArgs a) {
    extern __shared__ double sim_lds[];
    constexpr bool MIX = FAM == kMixture;
    const int wg = blockIdx.x;
    const int kk = wg >> 3;
    const int r = kk % c.R;
    const int tile = (kk / c.R) * 8 + (wg & 7);
    if (tile >= c.n_tiles) return;
    const int lane = threadIdx.x;
    const int G = c.G, B = c.B, R = c.R;
    const int g = tile * 64 + lane - c.g_sh;
    const bool valid = g >= 0 && g < G;
    const bool use_bc = (c.flags & kUseBc) != 0;
    double* cst = sim_lds;                                      // [4][B]: sf, sf_bc, sample mask, P0
    double* col = cst + 4 * B + lane;                           // col[b * 64]: the lane's table entry of bin b
    float* xs = (float*)(cst + 4 * B + (size_t)B * 64) + lane;  // xs[b * 64]: the counts of the likelihood at hand
    {
        const int kq = lane >> 3, bq = lane & 7;
        if (kq < 4) {
            const double* src = kq == 0 ? c.sf + r * B : (kq == 1 ? (use_bc ? c.sf_bc : c.sf) + r * B
                                                                  : (kq == 2 ? c.smask + r * B : c.P0));
            for (int b2 = bq; b2 < B; b2 += 8) cst[kq * B + b2] = (MIX || kq != 3) ? src[b2] : 0.0;
        }
    }
    __syncthreads();
    if (!valid) return;
    const unsigned j = blockIdx.y;
    if ((int)j >= a.n_draws) return;
    const unsigned long long d = a.first_draw + (unsigned long long)j;
    StepCtr ctr;
    ctr.step = d;
    ctr.slot = 0;
    ctr.step_size = 0.f;
    ctr.pad_ = 0.f;
    const double* c_sm = cst + 2 * B;
    const double* c_p0 = cst + 3 * B;
    const long rgi = (long)r * G + g;
    const bool rgm = c.rg[rgi] != 0;
    const unsigned long long sub = (unsigned long long)r * c.G_tot + (c.g_off + g);

    // ---- the pi draw of draw d and its transform: guide_pair_draw + the head of guide_pair_math
    double pi0 = 0.0, pi1 = 1.0, pe1 = 1.0, cp0 = 0.0, cp1 = 0.0;
    if (MIX) {
        const float api0 = c.p[4][2 * g], api1 = c.p[4][2 * g + 1];
        const double pa0 = c.pi_a0[g];
        uint4 philox_first = make_uint4(0u, 0u, 0u, 0u);
        if (!c.pi_in) philox_first = philox_block(c.seed, ((unsigned long long)kSitePi << 48) + sub, ctr.step * 256ull);
        guide_pair_draw<FAM>(c, ctr, r, g, api0, api1, pa0, &philox_first, &cp0, &cp1, pi0, pi1);
        if (c.pi_in) {
            pi0 = c.pi_in[rgi * 2];
            pi1 = c.pi_in[rgi * 2 + 1];
        }
        pe1 = pi1;
        if (ACC) {
            // scale_pi_by_accessibility + add_noise_to_pi, A = 2 (utils.py:106-178)
            double eps_n, ns, lpn;
            logw_noise_draw(c, g, d, eps_n, ns, lpn);
            const double kacc = c.kacc[g];
            const double s1 = pi1 * kacc;
            const double p1c = fmin(fmax(s1, 1e-3), 1.0 - 1e-3);
            const double l = flog(p1c * frcp(1.0 - p1c)) + lpn;
            const double el = exp(l);
            const double pn = el * frcp(1.0 + el);
            pe1 = fmin(fmax(pn, 1e-3), 1.0 - 1e-3);
        }
    }
    const double w0 = MIX ? (ACC ? 1.0 - pe1 : pi0) : 0.0;  // weight of the wild-type component
    const double w1 = MIX ? (ACC ? pe1 : pi1) : 1.0;        // weight of the edited component
    const double epsB = kEps / (double)B;

    // ---- the target's draw and this lane's B table entries
    const int t = c.g2t[g];
    const LogwTarget td = logw_target_draw(c, t, d);
    if (r == 0 && g == c.toff[t]) {
        a.mu_out[(size_t)j * c.T + t] = td.mu;
        if (a.y_out) a.y_out[(size_t)j * c.T + t] = td.y;
    }
    const double inv_sigma = phi_inv_sigma(c, td.y);
#pragma unroll 1
    for (int b = 0; b < B; ++b) col[b * 64] = planted_phi_entry(c, b, td.mu, inv_sigma);

    double term = 0.0;  // the pair's part of log p - log q
#pragma unroll 1
    for (int lik = 0; lik < 2; ++lik) {
        if (lik == 1 && !use_bc) break;
        const float* X = lik ? c.Xbc : c.X;
        const double* sf = cst + lik * B;
        const double a0 = lik ? c.a0_bc[g] : c.a0[g];
        // pass 1: n = sum x_b (data) and S = sum_b e_b sf_b; the counts are parked in the lane's column
        double S = 0.0, n = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const double e = fma(w0, MIX ? c_p0[b] : 0.0, w1 * col[b * 64]);
            S += e * sf[b];
            const float x = X[((long)r * B + b) * G + g];
            xs[b * 64] = x;
            n += (double)x;
        }
        // the site is masked by (sum_b x > mask_thres) & repguide_mask (model.py:526-547): lane by lane
        if (!(rgm && n > (double)c.mask_thres)) continue;
        const double inv = frcp(S + kEps);
        const double ai = a0 * inv;
        double A0 = 0.0, lsum = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const double ar = alpha_raw(w0, MIX ? c_p0[b] : 0.0, w1, col[b * 64], sf[b], epsB, ai * c_sm[b]);
            const double al = ar < kEps ? kEps : ar;
            const double x = (double)xs[b * 64];
            A0 += al;
            lsum += lgamma_digamma_diff(al, x).d;  // lgamma(alpha_b + x_b) - lgamma(alpha_b)
        }
        // log DirichletMultinomial less its multinomial coefficient (k_logw_consts): the per-bin terms less the total term
        term += lsum - lgamma_digamma_diff(A0, n).d;
    }
    if (MIX) {
        const double cq0 = cp0 < 1e-5 ? 1e-5 : cp0, cq1 = cp1 < 1e-5 ? 1e-5 : cp1;
        const double lpi0 = flog(pi0), lpi1 = flog(pi1);
        if (rgm) {
            // Multinomial(probs = pi) on control allele counts (model.py:470-474): torch renormalises the
            // probabilities and clamps them to [eps, 1 - eps]; the counts summed over the control conditions
            const double s = pi0 + pi1;
            const double ls = s == 1.0 ? 0.0 : flog(s);
            const double rs = s == 1.0 ? 1.0 : frcp(s);
            double cnt0 = 0.0, cnt1 = 0.0;
            for (int cc = 0; cc < c.C; ++cc) {
                const float* al = c.allele + (((long)r * c.C + cc) * G + g) * 2;
                cnt0 += (double)al[0];
                cnt1 += (double)al[1];
            }
            const double pr0 = pi0 * rs, pr1 = pi1 * rs;
            const bool in0 = pr0 > kProbEps && pr0 < 1.0 - kProbEps;
            const bool in1 = pr1 > kProbEps && pr1 < 1.0 - kProbEps;
            const double lg0 = in0 ? lpi0 - ls : flog(fmin(fmax(pr0, kProbEps), 1.0 - kProbEps));
            const double lg1 = in1 ? lpi1 - ls : flog(fmin(fmax(pr1, kProbEps), 1.0 - kProbEps));
            term += cnt0 * lg0;
            term += cnt1 * lg1;
            // + log p(pi): Dirichlet(c_p) under the repguide mask (model.py:454-463); its normaliser is per guide
            term += (cp0 - 1.0) * lpi0 + (cp1 - 1.0) * lpi1;
        }
        // - log q(pi): Dirichlet(c_q), unmasked in the guide (model.py:839-847)
        term -= (cq0 - 1.0) * lpi0 + (cq1 - 1.0) * lpi1;
    }
    double* slot = a.pair_out + ((size_t)j * R + r) * G + g;
    *slot = *slot + term;  // the pair's constant (k_logw_consts) plus its terms of this draw
}

__global__ __launch_bounds__(kLogwBlock)
void k_logw_targets(DevArgs c, LogwArgs a) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * kLogwBlock + threadIdx.x;
    if (idx >= (long)a.n_draws * c.T) return;
    const int j = (int)(idx / c.T), t = (int)(idx - (long)j * c.T);
    const unsigned long long d = a.first_draw + (unsigned long long)j;
    const int G = c.G, R = c.R;
    const int g0 = c.toff[t], g1 = c.toff[t + 1];
    double lw = 0.0;
    for (int r = 0; r < R; ++r) {
        const double* row = a.pair_out + ((size_t)j * R + r) * G;
        for (int g = g0; g < g1; ++g) lw += row[g];
    }
    // the target's own sites: - (- log p + log q) of tgt_prior_terms
    {
        const LogwTarget td = logw_target_draw(c, t, d);
        double dlogp_mu, dlogp_dy, loss;
        tgt_prior_terms(c, t, tgt_sd_prior(c, t), td.mu, td.y, td.eps1, td.eps2, c.p[1][t], c.p[3][t], dlogp_mu, dlogp_dy,
                        loss);
        lw -= loss;
    }
    if (c.family == kMixture) {
        const bool acc_on = (c.flags & kAcc) != 0;
        const double Rf = (double)R;
        for (int g = g0; g < g1; ++g) {
            // the pi site's normalisers, per guide as param_guide_mix adds them: nrg on the model side, R on the guide's
            const double al0 = (double)expf(c.p[4][2 * g]), al1 = (double)expf(c.p[4][2 * g + 1]);
            const double s = al0 + al1, pa0 = c.pi_a0[g];
            const double cp0 = al0 / s * pa0, cp1 = al1 / s * pa0;
            const bool clamped = cp0 < 1e-5 || cp1 < 1e-5;
            const double cq0 = cp0 < 1e-5 ? 1e-5 : cp0, cq1 = cp1 < 1e-5 ? 1e-5 : cp1;
            double lgS_p, lg_p0, lg_p1, dg;
            lgamma_digamma(cp0 + cp1, lgS_p, dg);
            lgamma_digamma(cp0, lg_p0, dg);
            lgamma_digamma(cp1, lg_p1, dg);
            double lgS_q = lgS_p, lg_q0 = lg_p0, lg_q1 = lg_p1;
            if (clamped) {
                lgamma_digamma(cq0 + cq1, lgS_q, dg);
                lgamma_digamma(cq0, lg_q0, dg);
                lgamma_digamma(cq1, lg_q1, dg);
            }
            double nrg = 0.0;
            for (int r = 0; r < R; ++r) nrg += c.rg[(long)r * G + g] != 0 ? 1.0 : 0.0;
            const double lp = nrg * (lgS_p - lg_p0 - lg_p1);
            const double lq = Rf * (lgS_q - lg_q0 - lg_q1);
            lw += lp - lq;
            if (acc_on) {
                double eps, ns, lpn;
                logw_noise_draw(c, g, d, eps, ns, lpn);
                // Normal(0, 0.655) prior held in float32 by the reference (utils.py:158-161)
                const float nsf = 0.655f;
                const double nvar = (double)(nsf * nsf);
                const double logp = -lpn * lpn / (2.0 * nvar) - (double)logf(nsf) - kHalfLog2PiC;
                const double logq = -0.5 * eps * eps - log(ns) - kHalfLog2PiC;
                lw += logp - logq;
            }
        }
    }
    a.logw_out[idx] = lw;
}

}  // namespace bean
