// k_logw_pairs_marg_tail: the Gauss-Jacobi rule of bean_jacobi.hpp for the marginal importance weights
// (bean_hip_log_weights_marginal_tail).
//
// The tail pairs - the pairs under the repguide mask that fail section 21's predicate - their compact list and the
// 64 + 48 nodes per pair are those of bean_jacobi.hpp (k_logw_unresolved, k_tail_offsets, k_tail_list, k_tail_nodes),
// formed once per call: they depend on alpha_pi and the control counts alone, not on the draw.  What differs from
// k_grid_pairs_tail is where (mu, y) comes from - the target's draw, logw_target_draw(c, t, first_draw + j) - and that
// the importance weights admit accessibility: with ACC the lane draws its guide's noise (logw_noise_draw) and the
// integrand is marg_h<true>, whose clamp of the scaled share at 1e-3 is a kink inside the mass of the rule's weight
// (section 25 measures what that costs; |J64 - J48| reports it per pair and draw).
//
// A lane is one (tail pair k, draw j): idx = j * n_tail + k over a one-dimensional grid, so that a handful of tail
// pairs still fills waves and the lanes of a wave write neighbouring slots of pair_err.  The block stages the
// [R][4][B] constants of every replicate as k_grid_pairs_tail does (logw_tail_lds; the host refuses above 64 KiB); the
// lane stages its counts, c_p, control counts, lbeta and tail_pair_const with that kernel's operations, then its B
// table entries, then the 64 + 48 evaluations with two running log-sum-exps.  The pair's slot of pair_out - which
// k_logw_pairs_marg has filled with the constant plus the Gauss-Hermite value - is OVERWRITTEN with
// const + lbeta + J64, and |J64 - J48| goes to pair_err[j * n_tail + k].  Slots of resolved pairs are not touched.
// Plain vector stores, no atomics, no scratch.  A lane's value is a function of (k, first_draw + j) alone: it does not
// depend on the launch geometry, on n_draws, or on how the caller chunks the draws.
#pragma once

namespace bean {

template <bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_logw_pairs_marg_tail(DevArgs c, LogwArgs a, TailArgs ta) {
    extern __shared__ double sim_lds[];
    const int lane = threadIdx.x;
    const int G = c.G, B = c.B, R = c.R;
    const bool use_bc = (c.flags & kUseBc) != 0;
    // [R][4][B]: sf, sf_bc, sample mask, P0 of EVERY replicate (the pairs of a block belong to different ones)
    for (int i = lane; i < R * 4 * B; i += 64) {
        const int rr = i / (4 * B), kq = (i - rr * 4 * B) / B, b = i - (rr * 4 + kq) * B;
        const double* src = kq == 0 ? c.sf + rr * B : (kq == 1 ? (use_bc ? c.sf_bc : c.sf) + rr * B
                                                              : (kq == 2 ? c.smask + rr * B : c.P0));
        sim_lds[i] = src[b];
    }
    __syncthreads();
    const long idx = (long)blockIdx.x * 64 + lane;
    if (idx >= (long)ta.n_tail * a.n_draws) return;
    const int j = (int)(idx / ta.n_tail), k = (int)(idx - (long)j * ta.n_tail);
    const unsigned long long d = a.first_draw + (unsigned long long)j;
    const int rgi = ta.pair[k];
    const int r = rgi / G, g = rgi - r * G;
    const int t = c.g2t[g];
    double* cst = sim_lds + (size_t)r * 4 * B;                             // the pair's replicate: [4][B]
    double* col = sim_lds + (size_t)R * 4 * B + lane;                      // col[b * 64]: the lane's table entry of bin b
    float* xs = (float*)(sim_lds + (size_t)R * 4 * B + (size_t)B * 64) + lane;  // xs[(lik * B + b) * 64]: its counts

    // ---- what depends on the data and on alpha_pi alone (k_grid_pairs_tail's staging)
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
    marg_model_conc(c, g, p.cp0, p.cp1);
    marg_ctrl_counts(c, r, g, p.cnt0, p.cnt1);
    const double a0p = p.cp0 + p.cnt0, a1p = p.cp1 + p.cnt1;
    const bool side1 = ta.side[k] != 0;
    const double a_small = side1 ? a1p : a0p, a_big = side1 ? a0p : a1p;
    double lbeta;
    {
        double lg0, lg1, lgS, dg;
        lgamma_digamma(a0p, lg0, dg);
        lgamma_digamma(a1p, lg1, dg);
        lgamma_digamma(a0p + a1p, lgS, dg);
        lbeta = lg0 + lg1 - lgS;
    }
    const double cnst = tail_pair_const(c, r, g);
    const double* zk = ta.z + (size_t)k * kTailAll;
    const double* lwk = ta.lw + (size_t)k * kTailAll;

    // ---- the draw: the target's (mu, y), with ACC the guide's noise, the B table entries
    const LogwTarget td = logw_target_draw(c, t, d);
    if (ACC) {
        double eps_n, ns;
        logw_noise_draw(c, g, d, eps_n, ns, p.lpn);
        p.kacc = c.kacc[g];
    }
    const double inv_sigma = phi_inv_sigma(c, td.y);
#pragma unroll 1
    for (int b = 0; b < B; ++b) col[b * 64] = planted_phi_entry(c, b, td.mu, inv_sigma);

    // ---- the 64 + 48 evaluations, two running log-sum-exps (k_grid_pairs_tail's loop)
    double j64 = 0.0, j48 = 0.0;
#pragma unroll 1
    for (int rule = 0; rule < 2; ++rule) {
        const int base = rule ? kTailNodes : 0, Q = rule ? kTailCheckNodes : kTailNodes;
        double mx = -INFINITY, acc = 0.0;
#pragma unroll 1
        for (int i = 0; i < Q; ++i) {
            const double z = zk[base + i];
            const double lz = log(z), l1z = log1p(-z);
            const double uu = lz - l1z;
            const double v = marg_h<ACC>(p, side1 ? uu : -uu) - a_small * lz - a_big * l1z + lwk[base + i];
            if (v == -INFINITY) continue;
            if (v > mx) {
                acc = fma(acc, exp(mx - v), 1.0);
                mx = v;
            } else {
                acc += exp(v - mx);
            }
        }
        const double val = mx + log(acc);
        if (rule) j48 = val;
        else j64 = val;
    }
    a.pair_out[((size_t)j * R + r) * G + g] = cnst + (lbeta + j64);
    ta.pair_err[(size_t)j * ta.n_tail + k] = fabs(j64 - j48);
}

}  // namespace bean
