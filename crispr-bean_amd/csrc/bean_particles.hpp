// Multi-particle SVI: P draws of every latent site per step, ONE ClippedAdam update with the mean of their gradients
// (bean_hip_svi_run_particles; Pyro's Trace_ELBO(num_particles = P)).
//
// The particles are members of the `_ens` kernels (bean_ensemble.hpp: gridDim.y = P, blockIdx.y the particle) that SHARE
// one set of parameters and moments.  Particle p has its own workspace copy, tsum, loss accumulators, row of loss
// values and seed, as an ensemble member has, and its p[] / m[] / v[] are the caller's single-fit buffers, the same P
// times; its g[] is row p of a library-owned (P, n) float32 scratch per parameter array.  A step is four launches:
//
//   k_param_ens<false, false, true, KIND>   the draws and tables of every particle from the shared parameters
//   k_guide_wave2_ens<FAM, ACC>
//   k_param_ens<true, false, false, KIND>   every particle's gradients into its scratch row, its loss parts
//   k_particle_adam                         the mean gradient in float64, particle order; one update; the step counters
//
// which is, per particle, the launch sequence of bean_hip_elbo_grad: same code, draws, summation order and bits.
// The step counters: k_param reads ctrA and leaves (step, slot) - FINISH: (step + 1, slot + 1) - in ctrB; the guide
// kernel reads ctrB and publishes it to ctrA.  With FINISH and PREP in separate launches nobody carries the advanced
// counter from ctrB back to ctrA before the next PREP launch reads it: k_particle_adam does, for every particle, after
// it has taken the update's t = step + 1 from particle 0's ctrB (no block of the launch reads ctrA, none writes ctrB).
#pragma once

namespace bean {

// the bound parameter arrays of a fit, end to end: array i covers the elements [start[i], start[i + 1])
struct ParticleArrays {
    float* p[8];
    float* g[8];  // the caller's gradient buffers: the mean of the last step
    float* m[8];
    float* v[8];
    const float* scratch[8];  // (P, n_i) float32: row q holds particle q's gradient
    long start[9];
};

// mean of P float32 values in float64: start from the first, add the others in particle order, one multiply by 1 / P,
// one rounding to float32
__device__ __forceinline__ float particle_mean(const float* col, long stride, int P) {
#pragma clang fp contract(off)
    double acc = (double)col[0];
    for (int q = 1; q < P; ++q) acc += (double)col[(long)q * stride];
    return (float)(acc * (1.0 / (double)P));
}

__global__ __launch_bounds__(256) void k_particle_adam(const DevArgs* particles, int P, ParticleArrays a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // (the FINISH launch in front of this one has left step + 1 in ctrB: the update's t)
    const unsigned long long t = particles[0].ctrB->step;
    if (i < a.start[8]) {
        int w = 0;
        while (i >= a.start[w + 1]) ++w;
        const long n = a.start[w + 1] - a.start[w], j = i - a.start[w];
        const float gm = particle_mean(a.scratch[w] + j, n, P);
        a.g[w][j] = gm;
        const AdamCoef k = adam_coef(particles[0], t);
        float pp = a.p[w][j], mm = a.m[w][j], vv = a.v[w][j];
        adam_update(pp, mm, vv, gm, k);
        a.p[w][j] = pp;
        a.m[w][j] = mm;
        a.v[w][j] = vv;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < P) {
        const DevArgs& c = particles[threadIdx.x];
        *c.ctrA = *c.ctrB;
    }
}

// loss_hist[first + i] = mean over the particles of their loss of that step, for the n steps of a call: float64 sum in
// particle order, times 1 / P (behind k_loss_finalize_ens, which has closed the particles' rows)
__global__ __launch_bounds__(256) void k_particle_loss(const DevArgs* particles, int P, double* out, unsigned long long first,
                                                       unsigned long long n) {
#pragma clang fp contract(off)
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double acc = particles[0].loss_hist[first + i];
    for (int q = 1; q < P; ++q) acc += particles[q].loss_hist[first + i];
    out[first + i] = acc * (1.0 / (double)P);
}

}  // namespace bean
