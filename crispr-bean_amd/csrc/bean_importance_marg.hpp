// k_logw_pairs_marg + k_logw_targets_marg + k_logw_unresolved: the importance weights of (mu_t, sd_t) alone, pi
// integrated out of the model (MixtureNormal).
//
//     logw_marg[d, t] = log p(mu_t) - log q(mu_t) + log p(sd_t) - log q(sd_t)
//                     + sum_g [ log p(noise_g) - log q(noise_g) ]                    (+Acc: the noise stays a drawn site)
//                     + sum_g nrg_g (lgamma(c_p0 + c_p1) - lgamma(c_p0) - lgamma(c_p1))    (the normaliser of Dirichlet(c_p),
//                                                                                   once per pair under the repguide mask)
//                     + sum_r sum_g ( const[r, g] + [rg] log int f(pi) dpi )
//     f(pi) = DirMult(x | alpha(pi))^[n > mask_thres] (and X_bcmatch) Multinomial(control counts | pi) pi_0^(c_p0 - 1) pi_1^(c_p1 - 1)
// No term of q(pi): neither - (c_q - 1) log pi nor its R normalisers.  (mu_t, y_t) and the +Acc noise are the draws
// k_logw_pairs forms for (seed, d); const is k_logw_consts', unchanged.
//
// The integral, per (draw, replicate, guide), in u = logit(pi_1):  int exp(h(u)) du  with
//     h(u) = [n > mask_thres] (log DirMult less its coefficient)(pi(u)) + sum_a (cnt_a log clamp(pi_a) + c_p,a log pi_a),
// the Jacobian pi_0 pi_1 turning the Beta-shaped factor into pi_0^a0' pi_1^a1', a' = c_p + control counts (log-concave, no
// endpoint singularity).  Rule: n_nodes-point Gauss-Hermite centred at the mode of h and scaled by its curvature there.
// From the Beta factor's centre u0 = log(a1' / a0') and scale s = sqrt(1 / a0' + 1 / a1'): kMargNewton Newton steps -
// a FIXED count, so the lanes of a wave stay together - with gradient and curvature from central differences at
// +- kMargFd s (a gradient step g s^2 where the second difference is not negative), each clamped to +- kMargStepCap s;
// the second difference at the end point gives sigma = (- h'')^(-1/2); where it is not negative the Beta centre and scale
// are kept.  Nodes are combined by a running log-sum-exp.  3 (kMargNewton + 1) + n_nodes evaluations of h per lane.
//
// Validity: the rule holds where min(a0', a1') >= kMargMinConc and fails where a component of a' is well below 1 (a slowly
// decaying exponential tail in u; tests/test_marginal_reference.py).  The predicate does not depend on the draw:
// k_logw_unresolved counts, once per call and in integers, the pairs of a target under the repguide mask that fail it.
// The kernel evaluates the rule for them all the same; the host does not report their targets.
//
// k_logw_pairs_marg<ACC>: grid and tile decode of k_logw_pairs; a lane is one (replicate, guide) of one draw and loops
// over its own nodes.  LDS: simulate_wave2_lds' layout with the count columns of BOTH likelihoods ([2][B][64] floats),
// filled once.  The lane's B table entries are formed once.  Adds log int f to the constant in ITS OWN slot of pair_out;
// plain vector stores, no atomics, no scratch.
#pragma once

#include "bean_gauss_hermite.hpp"

namespace bean {

constexpr double kMargMinConc = 2.0;
constexpr int kMargNewton = 4;
constexpr double kMargFd = 0.1;
constexpr double kMargStepCap = 2.0;
constexpr int kMargMaxNodes = 64;

struct MargArgs {
    int n_nodes;                    // 16, 32 or 64
    int* unresolved_out;            // (T)
    double x[kMargMaxNodes / 2];    // the positive nodes, ascending (gauss_hermite_half)
    double lw[kMargMaxNodes / 2];   // log w_i + x_i^2
};

__host__ __device__ inline size_t logw_marg_lds(int B) { return simulate_wave2_lds(B) + (size_t)B * 64 * sizeof(float); }

// what a lane keeps across its evaluations of h
struct MargPair {
    const double* cst;   // [4][B]: sf, sf_bc, sample mask, P0
    const double* col;   // col[b * 64]: the lane's table entry of bin b
    const float* xs;     // xs[(lik * B + b) * 64]: the lane's counts
    int B;
    bool on0, on1;       // the site of X / X_bcmatch is unmasked: n > mask_thres (under the repguide mask)
    double n0, n1, a00, a01;  // (scalars, not arrays: a lane's state stays in registers)
    double cnt0, cnt1, cp0, cp1;
    double kacc, lpn, epsB;
};

// the model-side concentrations of the pi site, with guide_pair_draw's operations
__device__ __forceinline__ void marg_model_conc(const DevArgs& c, int g, double& cp0, double& cp1) {
    const double al0 = (double)expf(c.p[4][2 * g]), al1 = (double)expf(c.p[4][2 * g + 1]);
    const double rs = frcp(al0 + al1) * c.pi_a0[g];
    cp0 = al0 * rs;
    cp1 = al1 * rs;
}
__device__ __forceinline__ void marg_ctrl_counts(const DevArgs& c, int r, int g, double& cnt0, double& cnt1) {
    cnt0 = 0.0;
    cnt1 = 0.0;
    for (int cc = 0; cc < c.C; ++cc) {
        const float* al = c.allele + (((long)r * c.C + cc) * c.G + g) * 2;
        cnt0 += (double)al[0];
        cnt1 += (double)al[1];
    }
}

// h(u): the functions k_logw_pairs evaluates at its drawn pi, at pi(u)
template <bool ACC>
__device__ __forceinline__ double marg_h(const MargPair& p, const double u) {
    // pi(u) and its logs without cancellation at either end: e = exp(-|u|), the larger share 1 / (1 + e)
    const double e = exp(-fabs(u));
    const double l1p = log1p(e);
    const double big = 1.0 / (1.0 + e), small = e * big;
    const bool pos = u >= 0.0;
    const double pi1 = pos ? big : small, pi0 = pos ? small : big;
    const double lpi1 = (pos ? 0.0 : u) - l1p, lpi0 = (pos ? -u : 0.0) - l1p;
    double w0 = pi0, w1 = pi1;
    if (ACC) {
        // scale_pi_by_accessibility + add_noise_to_pi, A = 2, at the drawn noise (as k_logw_pairs)
        const double s1 = pi1 * p.kacc;
        const double p1c = fmin(fmax(s1, 1e-3), 1.0 - 1e-3);
        const double l = flog(p1c * frcp(1.0 - p1c)) + p.lpn;
        const double el = exp(l);
        const double pn = el * frcp(1.0 + el);
        w1 = fmin(fmax(pn, 1e-3), 1.0 - 1e-3);
        w0 = 1.0 - w1;
    }
    const int B = p.B;
    const double* c_sm = p.cst + 2 * B;
    const double* c_p0 = p.cst + 3 * B;
    // log DirichletMultinomial less its multinomial coefficient: the two bin passes of k_logw_pairs
    auto lik_term = [&](const double* sf, const float* xs, const double a0, const double n) -> double {
        double S = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) S += fma(w0, c_p0[b], w1 * p.col[b * 64]) * sf[b];
        const double ai = a0 * frcp(S + kEps);
        double A0 = 0.0, lsum = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const double ar = alpha_raw(w0, c_p0[b], w1, p.col[b * 64], sf[b], p.epsB, ai * c_sm[b]);
            const double al = ar < kEps ? kEps : ar;
            A0 += al;
            lsum += lgamma_digamma_diff(al, (double)xs[b * 64]).d;
        }
        return lsum - lgamma_digamma_diff(A0, n).d;
    };
    double h = 0.0;
    if (p.on0) h += lik_term(p.cst, p.xs, p.a00, p.n0);
    if (p.on1) h += lik_term(p.cst + B, p.xs + (size_t)B * 64, p.a01, p.n1);
    // Multinomial(probs = pi) on the control allele counts, torch's clamp of the probabilities to [eps, 1 - eps]
    const bool in0 = pi0 > kProbEps && pi0 < 1.0 - kProbEps;
    const bool in1 = pi1 > kProbEps && pi1 < 1.0 - kProbEps;
    const double lg0 = in0 ? lpi0 : log(fmin(fmax(pi0, kProbEps), 1.0 - kProbEps));
    const double lg1 = in1 ? lpi1 : log(fmin(fmax(pi1, kProbEps), 1.0 - kProbEps));
    h += p.cnt0 * lg0;
    h += p.cnt1 * lg1;
    // Dirichlet(c_p) less its normaliser, times the Jacobian pi_0 pi_1 of u
    h += p.cp0 * lpi0 + p.cp1 * lpi1;
    return h;
}

template <bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_logw_pairs_marg(DevArgs c, LogwArgs a, MargArgs q) {
    extern __shared__ double sim_lds[];
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
    float* xs = (float*)(cst + 4 * B + (size_t)B * 64) + lane;  // xs[(lik * B + b) * 64]: the lane's counts
    {
        const int kq = lane >> 3, bq = lane & 7;
        if (kq < 4) {
            const double* src = kq == 0 ? c.sf + r * B : (kq == 1 ? (use_bc ? c.sf_bc : c.sf) + r * B
                                                                  : (kq == 2 ? c.smask + r * B : c.P0));
            for (int b2 = bq; b2 < B; b2 += 8) cst[kq * B + b2] = src[b2];
        }
    }
    __syncthreads();
    if (!valid) return;
    const unsigned j = blockIdx.y;
    if ((int)j >= a.n_draws) return;
    const unsigned long long d = a.first_draw + (unsigned long long)j;
    const long rgi = (long)r * G + g;

    // ---- the target's draw, as k_logw_pairs forms and stores it
    const int t = c.g2t[g];
    const LogwTarget td = logw_target_draw(c, t, d);
    if (r == 0 && g == c.toff[t]) {
        a.mu_out[(size_t)j * c.T + t] = td.mu;
        if (a.y_out) a.y_out[(size_t)j * c.T + t] = td.y;
    }
    if (c.rg[rgi] == 0) return;  // the pair's sites are masked: its slot keeps the constant (0)

    MargPair p;
    p.cst = cst;
    p.col = col;
    p.xs = xs;
    p.B = B;
    p.epsB = kEps / (double)B;
    p.kacc = 1.0;
    p.lpn = 0.0;
    if (ACC) {
        double eps_n, ns;
        logw_noise_draw(c, g, d, eps_n, ns, p.lpn);
        p.kacc = c.kacc[g];
    }
    const double inv_sigma = phi_inv_sigma(c, td.y);
#pragma unroll 1
    for (int b = 0; b < B; ++b) col[b * 64] = planted_phi_entry(c, b, td.mu, inv_sigma);
    // the counts of both likelihoods into the lane's columns, once; n = sum x_b masks the site (n > mask_thres)
    auto park_counts = [&](const float* X, float* dst) -> double {
        double n = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const float x = X[((long)r * B + b) * G + g];
            dst[b * 64] = x;
            n += (double)x;
        }
        return n;
    };
    p.n0 = park_counts(c.X, xs);
    p.on0 = p.n0 > (double)c.mask_thres;
    p.a00 = c.a0[g];
    p.n1 = 0.0;
    p.on1 = false;
    p.a01 = 0.0;
    if (use_bc) {
        p.n1 = park_counts(c.Xbc, xs + (size_t)B * 64);
        p.on1 = p.n1 > (double)c.mask_thres;
        p.a01 = c.a0_bc[g];
    }
    marg_model_conc(c, g, p.cp0, p.cp1);
    marg_ctrl_counts(c, r, g, p.cnt0, p.cnt1);

    // ---- centre and scale: the Beta factor's, then Newton towards the mode of h
    const double a0p = p.cp0 + p.cnt0, a1p = p.cp1 + p.cnt1;
    const double u0 = log(a1p / a0p);
    const double s = sqrt(1.0 / a0p + 1.0 / a1p);
    const double dl = kMargFd * s, cap = kMargStepCap * s;
    double m = u0, curv = 0.0;
#pragma unroll 1
    for (int it = 0; it <= kMargNewton; ++it) {
        double hm = 0.0, h0 = 0.0, hp = 0.0;
#pragma unroll 1
        for (int k = 0; k < 3; ++k) {
            const double v = marg_h<ACC>(p, m + (double)(k - 1) * dl);
            if (k == 0) hm = v;
            else if (k == 1) h0 = v;
            else hp = v;
        }
        const double grad = (hp - hm) / (2.0 * dl);
        curv = (hp - 2.0 * h0 + hm) / (dl * dl);
        if (it == kMargNewton) break;
        const double step = curv < 0.0 ? -grad / curv : grad * s * s;
        m += fmin(fmax(step, -cap), cap);
    }
    const bool ok = curv < 0.0;
    const double sc = 1.4142135623730951 * (ok ? 1.0 / sqrt(-curv) : s);
    if (!ok) m = u0;

    // ---- the nodes, combined by a running log-sum-exp
    double mx = -INFINITY, acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < q.n_nodes; ++k) {
        const int i = k >> 1;
        const double x = (k & 1) ? -q.x[i] : q.x[i];
        const double v = marg_h<ACC>(p, fma(sc, x, m)) + q.lw[i];
        if (v == -INFINITY) continue;
        if (v > mx) {
            acc = fma(acc, exp(mx - v), 1.0);
            mx = v;
        } else {
            acc += exp(v - mx);
        }
    }
    double* slot = a.pair_out + ((size_t)j * R + r) * G + g;
    *slot = *slot + (log(sc) + mx + log(acc));  // the pair's constant (k_logw_consts) plus log int f
}

// the pairs of a target that fail the validity predicate, under the repguide mask: one lane per target, once per call
__global__ __launch_bounds__(kLogwBlock)
void k_logw_unresolved(DevArgs c, MargArgs q) {
    const int t = blockIdx.x * kLogwBlock + threadIdx.x;
    if (t >= c.T) return;
    int n = 0;
    for (int g = c.toff[t]; g < c.toff[t + 1]; ++g) {
        double cp0, cp1;
        marg_model_conc(c, g, cp0, cp1);
        for (int r = 0; r < c.R; ++r) {
            if (c.rg[(long)r * c.G + g] == 0) continue;
            double cnt0, cnt1;
            marg_ctrl_counts(c, r, g, cnt0, cnt1);
            if (!(fmin(cp0 + cnt0, cp1 + cnt1) >= kMargMinConc)) ++n;
        }
    }
    q.unresolved_out[t] = n;
}

// k_logw_targets without the guide side of the pi site: the target's pair terms in the same fixed order, its own two
// sites, nrg model-side Dirichlet normalisers per guide and, with +Acc, the noise site
__global__ __launch_bounds__(kLogwBlock)
void k_logw_targets_marg(DevArgs c, LogwArgs a) {
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
    {
        const LogwTarget td = logw_target_draw(c, t, d);
        double dlogp_mu, dlogp_dy, loss;
        tgt_prior_terms(c, t, tgt_sd_prior(c, t), td.mu, td.y, td.eps1, td.eps2, c.p[1][t], c.p[3][t], dlogp_mu, dlogp_dy,
                        loss);
        lw -= loss;
    }
    const bool acc_on = (c.flags & kAcc) != 0;
    for (int g = g0; g < g1; ++g) {
        double cp0, cp1;
        marg_model_conc(c, g, cp0, cp1);
        double lgS, lg0, lg1, dg;
        lgamma_digamma(cp0 + cp1, lgS, dg);
        lgamma_digamma(cp0, lg0, dg);
        lgamma_digamma(cp1, lg1, dg);
        double nrg = 0.0;
        for (int r = 0; r < R; ++r) nrg += c.rg[(long)r * G + g] != 0 ? 1.0 : 0.0;
        lw += nrg * (lgS - lg0 - lg1);
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
    a.logw_out[idx] = lw;
}

}  // namespace bean
