// k_simulate_wave2: replicate counts of the variant sorting families, drawn on the device (posterior predictive check);
// k_simulate_members (at the end): K such screens in one launch, the member on blockIdx.y (parametric bootstrap);
// k_simulate_design (after it): D x K screens in one launch, K draws at each of D read depths (depth study);
// k_simulate_power (last): D x K screens in one launch, K draws at each of D planted effects (power study).
//
// For one draw d of the latent sites - the draw bean_hip_elbo_grad(seed, step = d) evaluates, prepared by the same
// k_set_step + PREP k_param launches - every (replicate, guide) forms the Dirichlet-Multinomial concentrations of its
// likelihoods (X and, with the flag, X_bcmatch) as guide_pair_math does, then draws
//     p ~ Dirichlet(alpha),    x_rep ~ Multinomial(n_obs, p),    n_obs = sum_b x_b of the observed counts.
//
//   * grid and lanes as k_guide_wave2: a single-wave workgroup is 64 consecutive guides (GLOBAL index) of one
//     replicate, XCD-aware decode of blockIdx.x, a lane is one (replicate, guide); a lane beyond G writes nothing.
//   * the pi site: guide_pair_draw<FAM>, same site, subsequence and offset; DevArgs::pi_in and the injected target
//     noise (lpn, formed by k_param) are honoured as guide_pair_math honours them.
//   * concentrations: the forward lines of guide_pair_math - accessibility transform, the S = sum_b e_b sf_b pre-pass,
//     a0 / (S + eps), the sample mask, alpha_raw with the same operands, floor at kEps.
//   * Dirichlet: B gammas from the Marsaglia-Tsang pair sampler on site kSiteSimGamma (bins two by two), floored at
//     kDblMin, normalised in float64.  A concentration on the 1e-5 floor takes the sampler's alpha < 1 boost
//     U^(1 / alpha), which underflows to zero for all but ~0.7 % of the draws: such a bin then holds the kDblMin floor,
//     i.e. a probability below 1e-300 - what Gamma(1e-5) is.  Where EVERY bin of a pair underflows (concentrations of
//     1e-3 in all of them: 8e-4 of the draws at a0 = 0.01) the floors would make the bins equal; such a pair is drawn
//     again in logs from the same counters (kSimLogBelow), so that the largest gamma takes the reads as it must.
//   * Multinomial: n_obs categorical draws by inversion on the float64 cumulative of p; one Philox block of site
//     kSiteSimCat gives four uniforms u = (w + 0.5) 2^-32; the bin is the number of cumulative values <= u among
//     the first B - 1, so the last bin takes what the cumulative leaves.  Exact for any n: no approximation branch,
//     no rejection, and the counts of a pair add up to n_obs by construction.
//   * COST: the draw loop runs ceil(n_obs / 4) times per lane, so a wave takes as long as its LARGEST total; lanes
//     that are done idle (a screen's totals inside a tile are of one magnitude; one deep guide costs its wave alone).
//   * masks do not enter: a pair masked by repguide_mask or n <= mask_thres is simulated like any other (the summary
//     leaves it out); the sample mask enters the concentrations exactly as in the ELBO.
//   * LDS: [4][B] per-bin constants of the replicate (as k_guide_wave2 stages them) | [B][64] doubles, a
//     thread-private column: table value, then concentration, gamma, cumulative | [B][64] floats, the counts drawn.
//     No scratch, no atomics; results leave through plain vector stores.
// Counter layout: next to RngSite (bean_special.hpp).
// The Dirichlet and Multinomial steps are dm_draw_tail and the accessibility transform is accessible_pi1: the survival
// simulators (bean_survival_predictive.hpp) call the same two functions.
#pragma once

namespace bean {

struct SimArgs {
    float* x_out;       // (R, B, G), the layout of BEAN_BUF_X
    float* xbc_out;     // (R, B, G) or null (no BEAN_FLAG_USE_BCMATCH)
    double* alpha_out;  // (2, R, B, G) floored concentrations or null
};

constexpr unsigned long long kSimGammaWords = 512;   // words reserved per pair of bins
constexpr unsigned long long kSimPairSlots = 32;     // pairs of bins per (likelihood, draw)
constexpr unsigned long long kSimCatWords = 1ull << 24;  // words per (likelihood, draw): one per categorical draw
// A pair whose floored gammas add up to less than this is normalised in logs.  Above it a floored bin's share is below
// kDblMin / 1e-290 = 2e-18 whether floored or not: no read lands there either way, and the draw keeps its bits.
constexpr double kSimLogBelow = 1e-290;
static_assert(kBCap <= 2 * kSimPairSlots, "the gamma windows hold kBCap conditions");

// scale_pi_by_accessibility + add_noise_to_pi, A = 2 (utils.py:106-178), as the guide kernels of both selections
// form it: the edited share scaled by the guide's accessibility factor, the injected or drawn noise `lpn` added to its
// logit, both clamps.
__device__ __forceinline__ double accessible_pi1(const double pi1, const double kacc, const double lpn) {
    const double s1 = pi1 * kacc;
    const double p1c = fmin(fmax(s1, 1e-3), 1.0 - 1e-3);
    const double l = flog(p1c * frcp(1.0 - p1c)) + lpn;
    const double el = exp(l);
    const double pn = el * frcp(1.0 + el);
    return fmin(fmax(pn, 1e-3), 1.0 - 1e-3);
}

// The draw tail of every count simulator: p ~ Dirichlet(alpha), x ~ Multinomial(n_i, p) for one lane.
//   seed, sub   the call's seed and the lane's subsequence r G_tot + g_off + g
//   dl          2 draw + likelihood: which window of kSiteSimGamma / kSiteSimCat
//   col         the lane's column col[b * 64] of B doubles, holding the floored concentrations; left as the cumulative
//   xs          the lane's column xs[b * 64] of B floats: the counts drawn are left here, the caller stores them
//   conc(b)     bin b's floored concentration formed again with the caller's operands, for the log branch
// Reads nothing of DevArgs: the sorting and the survival bodies hand it what it needs.
template <typename Conc>
__device__ __forceinline__ void dm_draw_tail(const unsigned long long seed, const unsigned long long sub,
                                             const unsigned long long dl, const int B, const long n_i, double* col,
                                             float* xs, const Conc& conc) {
    // ---- p ~ Dirichlet(alpha): gammas two bins at a time, then the cumulative
    double gsum = 0.0;
#pragma unroll 1
    for (int b = 0; b < B; b += 2) {
        const bool two = b + 1 < B;
        const double al0 = col[b * 64], al1 = two ? col[(b + 1) * 64] : 1.0;
        Rng rng(seed, kSiteSimGamma, sub, (dl * kSimPairSlots + (unsigned long long)(b >> 1)) * kSimGammaWords);
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
        // every gamma of this pair is at or near the kDblMin floor (concentrations of ~1e-3 and below in every bin):
        // floored, the bins would share the reads evenly, where the Dirichlet gives nearly all of them to the bin
        // with the largest gamma.  The same draws again in logs: log gamma = log(Marsaglia-Tsang draw of alpha + 1)
        // + log U / alpha, from the same counters (the boost's block first, then the rounds), less their maximum.
        // The column holds the gammas by now, so the caller forms the concentrations again (`conc`).
        double mx = -INFINITY;
#pragma unroll 1
        for (int b = 0; b < B; b += 2) {
            const bool two = b + 1 < B;
            const double al0 = conc(b), al1 = two ? conc(b + 1) : 1.0;
            const bool lo0 = al0 < 1.0, lo1 = al1 < 1.0;
            const unsigned long long off = (dl * kSimPairSlots + (unsigned long long)(b >> 1)) * kSimGammaWords;
            Rng rng(seed, kSiteSimGamma, sub, off + ((lo0 || lo1) ? 4ull : 0ull));
            const uint4 ub = philox_block(seed, rng.sub, off);
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
    const long n_blk = (n_i + 3) >> 2;
    const unsigned long long cat_sub = ((unsigned long long)kSiteSimCat << 48) + sub;
    const unsigned long long cat_off = dl * kSimCatWords;
#pragma unroll 1
    for (long t = 0; t < n_blk; ++t) {
        const uint4 w = philox_block(seed, cat_sub, cat_off + 4ull * (unsigned long long)t);
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
}

__host__ __device__ inline size_t simulate_wave2_lds(int B) {
    return ((size_t)4 * B + (size_t)B * 64) * sizeof(double) + (size_t)B * 64 * sizeof(float);
}

// The total a pair draws at read depth `depth`: floor(depth * n_obs + 0.5) in float64, at most kSimCatWords - 1 (the
// categorical window of a (likelihood, draw), and the largest count a float32 plane holds exactly next to its
// neighbours).  The host refuses depths that would reach the clamp (HipSVI.simulate_design); the kernel holds it anyway.
__device__ __forceinline__ long design_total(const double n_obs, const double depth) {
    const double t = floor(fma(depth, n_obs, 0.5));
    return (long)fmin(t, (double)(kSimCatWords - 1ull));
}

// The per-lane body of the simulators: the workgroup blockIdx.x of one screen, drawn as draw `ctr.step` into the
// planes of `s`.  `dump_pi` gates the BEAN_FLAG_DUMP_PI write (one screen has one pi_out).  One function, so that a plane
// of k_simulate_members is bit for bit the screen k_simulate_wave2 leaves for the same draw (as guide_pair_math is the
// one body of the guide kernels).  DEPTH (k_simulate_design alone): the pair draws design_total(n_obs, depth) reads
// instead of n_obs; nothing else of the draw - pi, concentrations, gammas, which word is which read - looks at it.
// PLANT (k_simulate_power alone): a lane whose target is planted (`plant` null, or plant[target] != 0) takes
// planted_phi_entry at mu = `effect` and the target's drawn y_t wherever the body reads the table - pass 1 and the
// concentrations the log branch forms again; every other lane, and everything else of the draw, is untouched.
template <int FAM, bool ACC, bool DEPTH = false, bool PLANT = false>
__device__ __forceinline__ void simulate_pair_body(const DevArgs& c, const SimArgs& s, const StepCtr& ctr, double* sim_lds,
                                                   const bool dump_pi, const double depth = 1.0, const double effect = 0.0,
                                                   const uint8_t* plant = nullptr) {
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
    double* cst = sim_lds;                                    // [4][B]: sf, sf_bc, sample mask, P0
    double* col = cst + 4 * B + lane;                         // col[b * 64]
    float* xs = (float*)(cst + 4 * B + (size_t)B * 64) + lane;  // xs[b * 64]
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
    const double* c_sm = cst + 2 * B;
    const double* c_p0 = cst + 3 * B;
    const long rgi = (long)r * G + g;
    const unsigned long long sub = (unsigned long long)r * c.G_tot + (c.g_off + g);

    // ---- the pi draw of this step and its transform: guide_pair_draw + the head of guide_pair_math
    double pi0 = 0.0, pi1 = 1.0, pe1 = 1.0;
    if (MIX) {
        const float api0 = c.p[4][2 * g], api1 = c.p[4][2 * g + 1];
        const double pa0 = c.pi_a0[g];
        uint4 philox_first = make_uint4(0u, 0u, 0u, 0u);
        if (!c.pi_in) philox_first = philox_block(c.seed, ((unsigned long long)kSitePi << 48) + sub, ctr.step * 256ull);
        double cp0, cp1;
        guide_pair_draw<FAM>(c, ctr, r, g, api0, api1, pa0, &philox_first, &cp0, &cp1, pi0, pi1);
        if (c.pi_in) {
            pi0 = c.pi_in[rgi * 2];
            pi1 = c.pi_in[rgi * 2 + 1];
        }
        if (dump_pi && (c.flags & kDumpPi) && c.pi_out) {
            c.pi_out[rgi * 2] = pi0;
            c.pi_out[rgi * 2 + 1] = pi1;
        }
        pe1 = pi1;
        if (ACC) pe1 = accessible_pi1(pi1, c.kacc[g], c.lpn[g]);
    }
    const double w0 = MIX ? (ACC ? 1.0 - pe1 : pi0) : 0.0;  // weight of the wild-type component
    const double w1 = MIX ? (ACC ? pe1 : pi1) : 1.0;        // weight of the edited component
    const double epsB = kEps / (double)B;
    const long tcol = c.g2t[g];
    // the table value of bin b: the shared table's, or - PLANT, a planted target - this lane's own entry at the effect
    const bool planted = PLANT && (!plant || plant[tcol] != 0);
    const double plant_inv = planted ? phi_inv_sigma(c, c.y_t[tcol]) : 0.0;
    const auto tab = [&](int b) {
        if (PLANT && planted) return planted_phi_entry(c, b, effect, plant_inv);
        return c.tabP[(long)b * c.T + tcol];
    };

#pragma unroll 1
    for (int lik = 0; lik < 2; ++lik) {
        if (lik == 1 && !use_bc) break;
        const float* X = lik ? c.Xbc : c.X;
        float* out = lik ? s.xbc_out : s.x_out;
        const double* sf = cst + lik * B;
        const double a0 = lik ? c.a0_bc[g] : c.a0[g];
        // pass 1: n = sum x_b (data) and S = sum_b e_b sf_b; the table value is parked in the column
        double S = 0.0, n = 0.0;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const double p1 = tab(b);
            const double e = fma(w0, MIX ? c_p0[b] : 0.0, w1 * p1);
            S += e * sf[b];
            n += (double)X[((long)r * B + b) * G + g];
            col[b * 64] = p1;
        }
        const double inv = frcp(S + kEps);
        const double ai = a0 * inv;
#pragma unroll 1
        for (int b = 0; b < B; ++b) {
            const double ar = alpha_raw(w0, MIX ? c_p0[b] : 0.0, w1, col[b * 64], sf[b], epsB, ai * c_sm[b]);
            const double al = ar < kEps ? kEps : ar;
            col[b * 64] = al;
            if (s.alpha_out) s.alpha_out[(((long)lik * R + r) * B + b) * G + g] = al;
        }
        // the concentrations again, for the log branch (the column holds the gammas by then): same operands, same bits
        const auto conc = [&](int b) {
            const double ar = alpha_raw(w0, MIX ? c_p0[b] : 0.0, w1, tab(b), sf[b], epsB, ai * c_sm[b]);
            return ar < kEps ? kEps : ar;
        };
        dm_draw_tail(c.seed, sub, ctr.step * 2ull + (unsigned long long)lik, B, DEPTH ? design_total(n, depth) : (long)n, col,
                     xs, conc);
#pragma unroll 1
        for (int b = 0; b < B; ++b) out[((long)r * B + b) * G + g] = xs[b * 64];
    }
}

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_simulate_wave2(DevArgs c, SimArgs s) {
    extern __shared__ double sim_lds[];
    const StepCtr ctr = *c.ctrB;
    simulate_pair_body<FAM, ACC>(c, s, ctr, sim_lds, true);
}

// k_simulate_members: K replicate screens of one fit in one launch (a parametric bootstrap's screens).  gridDim.x as
// k_simulate_wave2, gridDim.y = K; blockIdx.y is the member (the convention of bean_ensemble.hpp), so a single-wave
// workgroup is 64 guides of one replicate of one member.  The per-target and per-guide Normal sites, the tables and lpn
// are those of the ONE PREP k_param launch (draw ctrB->step, or the injected values); member k's per-(replicate, guide)
// sites - the pi draw, the gammas, the categorical draws - use draw ctrB->step + k wherever k_simulate_wave2 uses
// ctr.step: a StepCtr copy with that step is all simulate_pair_body and guide_pair_draw read.  Member k writes plane k of
// x_out / xbc_out, (K, R, B, G) member-major: what bean_hip_bind_member_counts binds.  pi_in is every member's; with
// BEAN_FLAG_DUMP_PI member 0 alone writes pi_out.  LDS, scratch, atomics and stores as k_simulate_wave2.
template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_simulate_members(DevArgs c, SimArgs s) {
    extern __shared__ double sim_lds[];
    StepCtr ctr = *c.ctrB;
    const unsigned member = blockIdx.y;
    ctr.step += (unsigned long long)member;
    const size_t plane = (size_t)member * (size_t)c.R * (size_t)c.B * (size_t)c.G;
    SimArgs sm;
    sm.x_out = s.x_out + plane;
    sm.xbc_out = s.xbc_out ? s.xbc_out + plane : nullptr;
    sm.alpha_out = nullptr;
    simulate_pair_body<FAM, ACC>(c, sm, ctr, sim_lds, member == 0);
}

// k_simulate_design: K replicate screens at each of D read depths in one launch (a depth study's screens).  gridDim.x
// as k_simulate_members, gridDim.y = D * K; member m = blockIdx.y = i * K + j is depth i, draw j, and writes plane (i, j)
// of x_out / xbc_out, (D, K, R, B, G) member-major.  The depth factors travel by value in the argument struct (D <= 64
// doubles, read through scalar loads of the kernel arguments): no caller-owned device pointer, no copy to wait for.
// Member (i, j) is member j of k_simulate_members in everything but its totals: the shared Normal sites, pi_in and
// DUMP_PI (member 0 alone) as there, draw ctrB->step + j for the pi, gamma and categorical sites AT EVERY DEPTH (common
// random numbers across depths), and design_total(n_obs, depth[i]) reads per pair.  From the counter layout:
//   (a) depth[i] == 1: plane (i, j) is bit for bit plane j of k_simulate_members (fma(1, n, 0.5) floors to n);
//   (b) depth[a] <= depth[b]: plane (a, j) <= plane (b, j) elementwise - categorical draw t is word t of the pair's
//       window and p does not depend on the total, so the deeper screen is the shallower one plus further reads;
//   (c) every (replicate, guide) of plane (i, j) sums to design_total(n_obs, depth[i]) exactly.
// COST: as k_simulate_members, with the largest n_i of a 64-guide tile in place of its largest n_obs - a wave of depth 4
// runs four times as long as its depth-1 twin.  LDS, scratch, atomics and stores as k_simulate_wave2.
struct DesignArgs {
    int K;                               // draws per depth
    int D;                               // depths
    double depth[kEnsembleMaxMembers];   // [D]
};
static_assert(sizeof(DevArgs) + sizeof(SimArgs) + sizeof(DesignArgs) <= 4096, "the kernel arguments fit their segment");

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_simulate_design(DevArgs c, SimArgs s, DesignArgs dz) {
    extern __shared__ double sim_lds[];
    StepCtr ctr = *c.ctrB;
    const unsigned member = blockIdx.y;
    const unsigned i = member / (unsigned)dz.K, j = member - i * (unsigned)dz.K;
    if (i >= (unsigned)dz.D) return;
    ctr.step += (unsigned long long)j;
    const size_t plane = (size_t)member * (size_t)c.R * (size_t)c.B * (size_t)c.G;
    SimArgs sm;
    sm.x_out = s.x_out + plane;
    sm.xbc_out = s.xbc_out ? s.xbc_out + plane : nullptr;
    sm.alpha_out = nullptr;
    simulate_pair_body<FAM, ACC, true>(c, sm, ctr, sim_lds, member == 0, dz.depth[i]);
}

// k_simulate_power: K replicate screens at each of D planted effects in one launch (a power study's screens).  gridDim.x
// as k_simulate_members, gridDim.y = D * K; member m = blockIdx.y = i * K + j is effect i, draw j, and writes plane (i, j)
// of x_out / xbc_out, (D, K, R, B, G) member-major.  The effects travel by value in the argument struct (D <= 64 doubles,
// read through scalar loads of the kernel arguments, indexed by the uniform blockIdx.y / K); `plant` is a device array of
// T bytes (non-zero: planted) or null (every target planted).  Member (i, j) is member j of k_simulate_members in
// everything but the table entries of its planted targets: the shared Normal sites (y_t among them), pi_in and DUMP_PI
// (member 0 alone) as there, draw ctrB->step + j for the pi, gamma and categorical sites AT EVERY EFFECT (common random
// numbers across effects).  A (replicate, guide) lane of a planted target forms Phi(u_hi) - Phi(u_lo) at mu = effect[i] -
// the value itself, not a shift of the fitted mu - and the target's drawn y_t, with write_phi_entry's operations, in
// pass 1 and again in the log branch; 2 B normal CDFs per likelihood next to ceil(n_obs / 4) categorical trips.  So
//   (a) with nothing planted, plane (i, j) is bit for bit plane j of k_simulate_members;
//   (b) plane (i, j) is bit for bit plane j of k_simulate_members on a handle whose PREP launch drew mu_t = effect[i]
//       on the planted targets (mu_loc = float32(effect[i]), eps_mu = 0) and is equal in everything else;
//   (c) every (replicate, guide) sums to n_obs exactly;
//   (d) the lanes of unplanted targets are those of k_simulate_members in every plane.
// The variant families share no parameter between targets and S = sum_b e_b sf_b normalises per guide, so planting every
// target at once leaves each target's counts what they are with it alone planted.  LDS, scratch, atomics and stores as
// k_simulate_wave2.
struct PowerArgs {
    int K;                               // draws per effect
    int D;                               // effects
    const uint8_t* plant;                // [T] or null: every target
    double effect[kEnsembleMaxMembers];  // [D]
};
static_assert(sizeof(DevArgs) + sizeof(SimArgs) + sizeof(PowerArgs) <= 4096, "the kernel arguments fit their segment");

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_simulate_power(DevArgs c, SimArgs s, PowerArgs pw) {
    extern __shared__ double sim_lds[];
    StepCtr ctr = *c.ctrB;
    const unsigned member = blockIdx.y;
    const unsigned i = member / (unsigned)pw.K, j = member - i * (unsigned)pw.K;
    if (i >= (unsigned)pw.D) return;
    ctr.step += (unsigned long long)j;
    const size_t plane = (size_t)member * (size_t)c.R * (size_t)c.B * (size_t)c.G;
    SimArgs sm;
    sm.x_out = s.x_out + plane;
    sm.xbc_out = s.xbc_out ? s.xbc_out + plane : nullptr;
    sm.alpha_out = nullptr;
    simulate_pair_body<FAM, ACC, false, true>(c, sm, ctr, sim_lds, member == 0, 1.0, pw.effect[i], pw.plant);
}

}  // namespace bean
