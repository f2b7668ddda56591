// k_grid_pairs + k_grid_targets: the log joint of a target at GIVEN (mu_t, y_t = log sd_t), pi integrated out of the
// model - the grid posterior of (mu, sd) per target (bean_hip_marginal_grid).
//
//     lj[n, t] = log p(mu) + log p(sd) + y                                          (a density in (mu, y))
//              + sum_g nrg_g (lgamma(c_p0 + c_p1) - lgamma(c_p0) - lgamma(c_p1))
//              + sum_r sum_g ( const[r, g] + [rg] log int f(pi) dpi )
// const, f, the quadrature rule and the validity predicate are those of bean_importance_marg.hpp, unchanged; there is no
// draw, no seed and no term of q.  Node n = i * n_y + k of target t:
//     mu = centre_mu[t] + (i - (n_mu - 1) / 2) step_mu[t],   y = centre_y[t] + (k - (n_y - 1) / 2) step_y[t],
// float64, contraction off: every target has its own affine grid.
//
// k_grid_pairs<FAM>: grid and tile decode of k_logw_pairs_marg (padded tiles x R, XCD-aware); blockIdx.y is a chunk of
// kGridChunk nodes; a lane is one (replicate, guide).  Everything that depends only on the data or on alpha_pi - the
// per-bin constants, the counts of both likelihoods in the lane's LDS columns (logw_marg_lds), c_p, the control counts,
// the Beta centre u0 and scale s - is formed ONCE per lane; the lane then loops over the nodes of its chunk: the B table
// entries at the node's (mu, y), section 21's rule (marg_h<false>, kMargNewton steps then n_nodes nodes: fixed counts, the
// lanes of a wave stay together), and the result added to the constant in ITS OWN slot pair_out[(n, r, g)].
// BEAN_FAMILY_NORMAL has no pi: the pair's term is k_logw_pairs' likelihood term with w0 = 0, w1 = 1.
// Plain vector stores, no atomics, no scratch.
//
// kGridChunk = 4: what a lane forms once costs less than one of the 3 (kMargNewton + 1) + n_nodes evaluations of h a
// node takes, so four nodes already hide it, and a 17 x 17 zoom grid of a one-tile screen still spreads over 73 x R
// x 8 workgroups.
//
// k_grid_targets: one lane per (node, target); adds the pair terms in k_logw_targets_marg's fixed order (replicate outer,
// guide inner), the target's two prior terms (grid_log_priors: the log p side of tgt_prior_terms, --prior-params
// included), + y, and the nrg model-side normalisers per guide.
#pragma once

namespace bean {

constexpr int kGridChunk = 4;

struct GridArgs {
    int n_mu, n_y;
    const double* centre_mu;  // (T)
    const double* centre_y;   // (T)
    const double* step_mu;    // (T)
    const double* step_y;     // (T)
    double* lj_out;           // (n_mu * n_y, T)
    double* pair_out;         // (n_mu * n_y, R, G)
};

// (mu, y) of node n of target t
__device__ __forceinline__ void grid_node(const GridArgs& a, int t, int n, double& mu, double& y) {
#pragma clang fp contract(off)
    const int i = n / a.n_y, k = n - i * a.n_y;
    const double di = (double)i - (double)(a.n_mu - 1) / 2.0;
    const double dk = (double)k - (double)(a.n_y - 1) / 2.0;
    mu = a.centre_mu[t] + di * a.step_mu[t];
    y = a.centre_y[t] + dk * a.step_y[t];
}

// log p(mu) and log p(sd) of the target's two sites: the log p side of tgt_prior_terms, with its operations
__device__ __forceinline__ void grid_log_priors(const DevArgs& c, int t, const TgtPrior& pr, double mu, double y,
                                                double& logp_mu, double& logp_sd) {
#pragma clang fp contract(off)
    if (c.flags & kPriorNormalMu) {
        const double pl = c.pr_mu_loc ? c.pr_mu_loc[t] : 0.0;
        const double ps = c.pr_mu_scale ? c.pr_mu_scale[t] : 1.0;
        const double zz = (mu - pl) / ps;
        logp_mu = -0.5 * zz * zz - log(ps) - kHalfLog2PiC;
    } else {
        logp_mu = -kLog2 - fabs(mu);
    }
    const double dy0 = y - pr.l0;
    logp_sd = -y - pr.logs0 - kHalfLog2PiC - dy0 * dy0 / (2.0 * pr.var0);
}

// log DirichletMultinomial less its multinomial coefficient of one likelihood at component weights (w0, w1): the two
// bin passes of k_logw_pairs on the lane's parked counts
__device__ __forceinline__ double grid_lik_term(const MargPair& p, const double w0, const double w1, const double* sf,
                                                const float* xs, const double a0, const double n) {
    const int B = p.B;
    const double* c_sm = p.cst + 2 * B;
    const double* c_p0 = p.cst + 3 * B;
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
}

template <int FAM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_grid_pairs(DevArgs c, GridArgs a, MargArgs q) {
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
    float* xs = (float*)(cst + 4 * B + (size_t)B * 64) + lane;  // xs[(lik * B + b) * 64]: the lane's counts
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
    const int N = a.n_mu * a.n_y;
    const int n_first = (int)blockIdx.y * kGridChunk;
    if (n_first >= N) return;
    const int n_end = min(n_first + kGridChunk, N);
    const long rgi = (long)r * G + g;
    if (c.rg[rgi] == 0) return;  // the pair's sites are masked: its slots keep the constant (0)
    const int t = c.g2t[g];

    // ---- what depends on the data and on alpha_pi alone: once per lane
    MargPair p;
    p.cst = cst;
    p.col = col;
    p.xs = xs;
    p.B = B;
    p.epsB = kEps / (double)B;
    p.kacc = 1.0;
    p.lpn = 0.0;
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
    p.cp0 = p.cp1 = p.cnt0 = p.cnt1 = 0.0;
    double u0 = 0.0, s = 1.0;
    if (MIX) {
        marg_model_conc(c, g, p.cp0, p.cp1);
        marg_ctrl_counts(c, r, g, p.cnt0, p.cnt1);
        // the Beta factor's centre and scale
        const double a0p = p.cp0 + p.cnt0, a1p = p.cp1 + p.cnt1;
        u0 = log(a1p / a0p);
        s = sqrt(1.0 / a0p + 1.0 / a1p);
    }
    const double dl = kMargFd * s, cap = kMargStepCap * s;

    // ---- the nodes of the chunk
#pragma unroll 1
    for (int n = n_first; n < n_end; ++n) {
        double mu, y;
        grid_node(a, t, n, mu, y);
        const double inv_sigma = phi_inv_sigma(c, y);
#pragma unroll 1
        for (int b = 0; b < B; ++b) col[b * 64] = planted_phi_entry(c, b, mu, inv_sigma);
        double term;
        if (MIX) {
            // Newton towards the mode of h from the Beta centre, then the nodes: k_logw_pairs_marg's rule
            double m = u0, curv = 0.0;
#pragma unroll 1
            for (int it = 0; it <= kMargNewton; ++it) {
                double hm = 0.0, h0 = 0.0, hp = 0.0;
#pragma unroll 1
                for (int k = 0; k < 3; ++k) {
                    const double v = marg_h<false>(p, m + (double)(k - 1) * dl);
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
            double mx = -INFINITY, acc = 0.0;
#pragma unroll 1
            for (int k = 0; k < q.n_nodes; ++k) {
                const int i = k >> 1;
                const double x = (k & 1) ? -q.x[i] : q.x[i];
                const double v = marg_h<false>(p, fma(sc, x, m)) + q.lw[i];
                if (v == -INFINITY) continue;
                if (v > mx) {
                    acc = fma(acc, exp(mx - v), 1.0);
                    mx = v;
                } else {
                    acc += exp(v - mx);
                }
            }
            term = log(sc) + mx + log(acc);
        } else {
            term = 0.0;
            if (p.on0) term += grid_lik_term(p, 0.0, 1.0, cst, xs, p.a00, p.n0);
            if (p.on1) term += grid_lik_term(p, 0.0, 1.0, cst + B, xs + (size_t)B * 64, p.a01, p.n1);
        }
        double* slot = a.pair_out + ((size_t)n * R + r) * G + g;
        *slot = *slot + term;  // the pair's constant (k_logw_consts) plus its term at this node
    }
}

__global__ __launch_bounds__(kLogwBlock)
void k_grid_targets(DevArgs c, GridArgs a) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * kLogwBlock + threadIdx.x;
    if (idx >= (long)a.n_mu * a.n_y * c.T) return;
    const int n = (int)(idx / c.T), t = (int)(idx - (long)n * c.T);
    const int G = c.G, R = c.R;
    const int g0 = c.toff[t], g1 = c.toff[t + 1];
    double lj = 0.0;
    for (int r = 0; r < R; ++r) {
        const double* row = a.pair_out + ((size_t)n * R + r) * G;
        for (int g = g0; g < g1; ++g) lj += row[g];
    }
    {
        double mu, y, logp_mu, logp_sd;
        grid_node(a, t, n, mu, y);
        grid_log_priors(c, t, tgt_sd_prior(c, t), mu, y, logp_mu, logp_sd);
        lj += logp_mu;
        lj += logp_sd;
        lj += y;
    }
    if (c.family == kMixture) {
        for (int g = g0; g < g1; ++g) {
            double cp0, cp1;
            marg_model_conc(c, g, cp0, cp1);
            double lgS, lg0, lg1, dg;
            lgamma_digamma(cp0 + cp1, lgS, dg);
            lgamma_digamma(cp0, lg0, dg);
            lgamma_digamma(cp1, lg1, dg);
            double nrg = 0.0;
            for (int r = 0; r < R; ++r) nrg += c.rg[(long)r * G + g] != 0 ? 1.0 : 0.0;
            lj += nrg * (lgS - lg0 - lg1);
        }
    }
    a.lj_out[idx] = lj;
}

}  // namespace bean
