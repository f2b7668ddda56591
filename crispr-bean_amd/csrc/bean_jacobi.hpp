// k_tail_offsets + k_tail_list + k_tail_nodes + k_grid_pairs_tail + k_grid_targets_tail: a Gauss-Jacobi rule for the
// (replicate, guide) pairs that section 21's predicate leaves out (bean_hip_marginal_grid_tail).
//
// A tail pair is a pair under the repguide mask with min(a0', a1') < kMargMinConc, a' = c_p + control counts.  Its
// integrand is  f(pi) = pi_0^(a0' - 1) pi_1^(a1' - 1) G(pi_1)  with G smooth on [0, 1]; with b = min(a0', a1'),
// a = max(a0', a1') and z the share of the smaller exponent's side (side = 1: pi_1, ties included; side = 0: pi_0),
//     log int f = lbeta(a0', a1') + logsumexp_i( lw_i + lg(z_i) ),
//     lg(z)     = h(u(z)) - a0' log pi_0 - a1' log pi_1,     u = +- (log z - log1p(-z)),     h = marg_h<false>,
// z_i, lw_i the nodes and log weights of the Gauss-Jacobi rule for z^(b - 1) (1 - z)^(a - 1) on (0, 1), the weights
// normalised to sum 1: the endpoint singularity is in the weight, the singular end is always z = 0, and neither log z
// nor log1p(-z) cancels.  kTailNodes = 64 nodes give the value, kTailCheckNodes = 48 a second, independent one;
// a pair's tail_err at a grid node is |J64 - J48|.  112 evaluations of h per (tail pair, grid node).
//
// The nodes depend on alpha_pi and the control counts alone: they are formed once per call, on the device, in double.
// Jacobi matrix of the weight, al = a - 1, be = b - 1, c = al + be, s_n = 2 n + c (forms without a 1 + t cancellation):
//     d_0 = (1 + be) / (c + 2),   d_n = (2 n (n + c + 1) + c (1 + be)) / (s_n (s_n + 2)),
//     e_1^2 = (1 + al) (1 + be) / ((3 + c) (2 + c)^2),   e_n^2 = n (n + al) (n + be) (n + c) / ((s_n - 1) (s_n + 1) s_n^2).
// Node j is the j-th smallest eigenvalue: kTailBisect bisections of (0, 1) on the Sturm sequence - a fixed count, no
// initial guess to get wrong - then kTailPolish Newton steps on the orthonormal recurrence
//     p_0 = 1,   e_(k+1) p_(k+1) = (x - d_k) p_k - e_k p_(k-1),
// and the Christoffel number 1 / sum_(k < Q) p_k(x)^2 as the weight (bean_gauss_hermite.hpp is the pattern).  The
// coefficients are formed on the fly: no array, no scratch.
//
// The list of tail pairs is compact and ordered: target, then guide, then replicate - the order in which
// k_logw_unresolved counts them.  k_tail_offsets: one block; the exclusive scan of unresolved_out (T) into toff (T + 1).
// k_tail_list: one lane per target writes its pairs' indices r * G + g and sides from toff[t] on.  k_tail_nodes: one
// lane per (pair, node of the 64 + 48).  Workspace per call: kTailPairBytes = 1 792 + 8 bytes per tail pair (z and lw of
// 112 nodes; the index and the side) plus 8 N bytes per tail pair for the tail_pair_err plane of an N-node call, plus
// 4 (T + 1) for toff; a call whose workspace would exceed kTailMaxBytes is refused.
//
// k_grid_pairs_tail: after k_grid_pairs.  A lane is one (tail pair, chunk of kTailChunk grid nodes).  The pairs of a
// block belong to different replicates, so the block stages the [4][B] constants of every replicate in LDS beside the
// lanes' table and count columns (logw_tail_lds); otherwise the once-per-lane staging is k_grid_pairs'.  Per grid node: the B table entries,
// the 64 + 48 evaluations with two running log-sum-exps; the pair's slot of pair_out is OVERWRITTEN with the pair's
// constant (k_logw_consts' operations) plus the tail term, and |J64 - J48| goes to tail_pair_err[n, k].  Slots of
// resolved pairs are not touched.  k_grid_targets_tail: one lane per (grid node, target) sums tail_pair_err over the
// target's tail pairs (contiguous in the list) into tail_err[n, t]; lj itself is k_grid_targets', launched as it is.
// Plain vector stores, no atomics, no scratch; no result depends on the launch geometry.
#pragma once

namespace bean {

constexpr int kTailNodes = 64;
constexpr int kTailCheckNodes = 48;
constexpr int kTailAll = kTailNodes + kTailCheckNodes;
constexpr int kTailBisect = 80;   // (0, 1) halved 80 times: below an ulp of any node above 1e-8
constexpr int kTailPolish = 2;
constexpr int kTailChunk = 1;     // grid nodes per lane: few lanes, each 112 evaluations long - the call waits for the longest
constexpr int kTailScanBlock = 256;
constexpr uint64_t kTailPairBytes = (uint64_t)kTailAll * 16 + 8;
constexpr uint64_t kTailMaxBytes = 256ull << 20;

struct TailArgs {
    int n_tail;            // the number of tail pairs (known to the host: sum of unresolved_out)
    int N;                 // grid nodes of the call
    const int* unresolved; // (T)
    int* toff;             // (T + 1): the first list entry of target t
    int* pair;             // (n_tail): r * G + g
    int* side;             // (n_tail): 1 where the smaller exponent is pi_1's
    double* z;             // (n_tail, kTailAll): the 64 nodes ascending, then the 48
    double* lw;            // (n_tail, kTailAll)
    double* pair_err;      // (N, n_tail)
    double* tail_err_out;  // (N, T)
};

__host__ __device__ inline size_t logw_tail_lds(int R, int B) {
    return (size_t)R * 4 * B * sizeof(double) + (size_t)B * 64 * sizeof(double) + (size_t)2 * B * 64 * sizeof(float);
}

__global__ __launch_bounds__(kTailScanBlock)
void k_tail_offsets(int T, TailArgs ta) {
    __shared__ int part[kTailScanBlock];
    const int tid = threadIdx.x;
    const int per = (T + kTailScanBlock - 1) / kTailScanBlock;
    const int t0 = min(tid * per, T), t1 = min(t0 + per, T);
    int s = 0;
    for (int t = t0; t < t1; ++t) s += ta.unresolved[t];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < kTailScanBlock; ++i) {
            const int v = part[i];
            part[i] = run;
            run += v;
        }
        ta.toff[T] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int t = t0; t < t1; ++t) {
        ta.toff[t] = run;
        run += ta.unresolved[t];
    }
}

// the exponents of a pair's Beta-shaped factor, with k_logw_unresolved's operations
__device__ __forceinline__ void tail_exponents(const DevArgs& c, int r, int g, double& a0p, double& a1p) {
    double cp0, cp1, cnt0, cnt1;
    marg_model_conc(c, g, cp0, cp1);
    marg_ctrl_counts(c, r, g, cnt0, cnt1);
    a0p = cp0 + cnt0;
    a1p = cp1 + cnt1;
}

__global__ __launch_bounds__(kLogwBlock)
void k_tail_list(DevArgs c, TailArgs ta) {
    const int t = blockIdx.x * kLogwBlock + threadIdx.x;
    if (t >= c.T) return;
    int k = ta.toff[t];
    const int k_end = min(ta.toff[t + 1], ta.n_tail);
    for (int g = c.toff[t]; g < c.toff[t + 1]; ++g) {
        for (int r = 0; r < c.R; ++r) {
            if (c.rg[(long)r * c.G + g] == 0) continue;
            double a0p, a1p;
            tail_exponents(c, r, g, a0p, a1p);
            if (!(fmin(a0p, a1p) >= kMargMinConc) && k < k_end) {
                ta.pair[k] = r * c.G + g;
                ta.side[k] = a1p <= a0p ? 1 : 0;
                ++k;
            }
        }
    }
}

// the Jacobi matrix's diagonal and squared off-diagonal entries
__device__ __forceinline__ double jacobi_d(int n, double be, double c) {
    if (n == 0) return (1.0 + be) / (c + 2.0);
    const double fn = (double)n, s = 2.0 * fn + c;
    return (2.0 * fn * (fn + c + 1.0) + c * (1.0 + be)) / (s * (s + 2.0));
}
__device__ __forceinline__ double jacobi_e2(int n, double al, double be, double c) {
    if (n == 1) return (1.0 + al) * (1.0 + be) / ((3.0 + c) * (2.0 + c) * (2.0 + c));
    const double fn = (double)n, s = 2.0 * fn + c;
    return fn * (fn + al) * (fn + be) * (fn + c) / ((s - 1.0) * (s + 1.0) * s * s);
}

__global__ __launch_bounds__(kLogwBlock)
void k_tail_nodes(DevArgs c, TailArgs ta) {
    const long idx = (long)blockIdx.x * kLogwBlock + threadIdx.x;
    if (idx >= (long)ta.n_tail * kTailAll) return;
    const int k = (int)(idx / kTailAll), i = (int)(idx - (long)k * kTailAll);
    const int Q = i < kTailNodes ? kTailNodes : kTailCheckNodes;
    const int j = i < kTailNodes ? i : i - kTailNodes;
    const int rgi = ta.pair[k];
    const int r = rgi / c.G, g = rgi - r * c.G;
    double a0p, a1p;
    tail_exponents(c, r, g, a0p, a1p);
    const double al = fmax(a0p, a1p) - 1.0, be = fmin(a0p, a1p) - 1.0, cc = al + be;
    // the j-th smallest eigenvalue: bisection on the Sturm sequence (the count of eigenvalues below mid)
    double lo = 0.0, hi = 1.0;
#pragma unroll 1
    for (int it = 0; it < kTailBisect; ++it) {
        const double mid = 0.5 * (lo + hi);
        int below = 0;
        double q = jacobi_d(0, be, cc) - mid;
        if (q < 0.0) ++below;
#pragma unroll 1
        for (int n = 1; n < Q; ++n) {
            if (q == 0.0) q = 1e-300;
            q = jacobi_d(n, be, cc) - mid - jacobi_e2(n, al, be, cc) / q;
            if (q < 0.0) ++below;
        }
        if (below > j) hi = mid;
        else lo = mid;
    }
    double x = 0.5 * (lo + hi), total = 1.0;
#pragma unroll 1
    for (int pass = 0; pass <= kTailPolish; ++pass) {
        double pm = 0.0, p = 1.0, dm = 0.0, dp = 0.0, ek = 0.0;
        total = 1.0;
#pragma unroll 1
        for (int n = 0; n < Q; ++n) {
            const double en = sqrt(jacobi_e2(n + 1, al, be, cc));
            const double xd = x - jacobi_d(n, be, cc);
            const double pn = (xd * p - ek * pm) / en;
            const double dn = (xd * dp + p - ek * dm) / en;
            pm = p;
            p = pn;
            dm = dp;
            dp = dn;
            ek = en;
            if (n + 1 < Q) total += p * p;
        }
        if (pass < kTailPolish) x -= p / dp;
    }
    ta.z[idx] = x;
    ta.lw[idx] = -log(total);
}

// the pair's data-only constant: k_logw_consts' operations, for a pair under the repguide mask (MixtureNormal)
__device__ __forceinline__ double tail_pair_const(const DevArgs& c, int r, int g) {
    const int G = c.G, B = c.B;
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
        if (n > (double)c.mask_thres) v += logw_lfact(n) - lf;
    }
    for (int cn = 0; cn < c.C; ++cn) {
        const float* al = c.allele + (((long)r * c.C + cn) * G + g) * 2;
        const double y0 = (double)al[0], y1 = (double)al[1];
        v += logw_lfact(y0 + y1) - logw_lfact(y0) - logw_lfact(y1);
    }
    return v;
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_grid_pairs_tail(DevArgs c, GridArgs a, TailArgs ta) {
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
    const int k = (int)blockIdx.x * 64 + lane;
    if (k >= ta.n_tail) return;
    const int N = a.n_mu * a.n_y;
    const int n_first = (int)blockIdx.y * kTailChunk;
    if (n_first >= N) return;
    const int n_end = min(n_first + kTailChunk, N);
    const int rgi = ta.pair[k];
    const int r = rgi / G, g = rgi - r * G;
    const int t = c.g2t[g];
    double* cst = sim_lds + (size_t)r * 4 * B;                             // the pair's replicate: [4][B]
    double* col = sim_lds + (size_t)R * 4 * B + lane;                      // col[b * 64]: the lane's table entry of bin b
    float* xs = (float*)(sim_lds + (size_t)R * 4 * B + (size_t)B * 64) + lane;  // xs[(lik * B + b) * 64]: its counts

    // ---- what depends on the data and on alpha_pi alone: once per lane (k_grid_pairs' staging)
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

    // ---- the grid nodes of the chunk
#pragma unroll 1
    for (int n = n_first; n < n_end; ++n) {
        double mu, y;
        grid_node(a, t, n, mu, y);
        const double inv_sigma = phi_inv_sigma(c, y);
#pragma unroll 1
        for (int b = 0; b < B; ++b) col[b * 64] = planted_phi_entry(c, b, mu, inv_sigma);
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
                const double v = marg_h<false>(p, side1 ? uu : -uu) - a_small * lz - a_big * l1z + lwk[base + i];
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
        a.pair_out[((size_t)n * R + r) * G + g] = cnst + (lbeta + j64);
        ta.pair_err[(size_t)n * ta.n_tail + k] = fabs(j64 - j48);
    }
}

__global__ __launch_bounds__(kLogwBlock)
void k_grid_targets_tail(DevArgs c, TailArgs ta) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * kLogwBlock + threadIdx.x;
    if (idx >= (long)ta.N * c.T) return;
    const int n = (int)(idx / c.T), t = (int)(idx - (long)n * c.T);
    double e = 0.0;
    const int k_end = min(ta.toff[t + 1], ta.n_tail);
    for (int k = ta.toff[t]; k < k_end; ++k) e += ta.pair_err[(size_t)n * ta.n_tail + k];
    ta.tail_err_out[idx] = e;
}

}  // namespace bean
