// k_guide_survival_wave: the per-(replicate, guide) kernel of the survival variant families in the
// wave form of k_guide_wave2 (bean_guide_v2.hpp): one single-wave workgroup per (64-guide tile,
// replicate), rolled loops over the timepoints with thread-private LDS columns, per-replicate rows
// (summed over replicates by k_param), XCD-aware 1-D grid.  It replaces the block form
// k_guide_survival<B, ...> (R waves per block, per-thread arrays e[B], ge[B], P0[B], P1[B]: 216 VGPRs
// at six timepoints, two waves per SIMD), which stays selectable (BEAN_HIP_SURVIVAL=block) as the A/B
// reference.
//
// Reference semantics: bean/model/survival_model.py - NormalModel 15-130 (+ guide 629-648),
// ControlNormalModel 133-212, MixtureNormalModel 215-424 (+ guide 651-739): component "bin
// probabilities" are exp(mu_a t_b) with mu = [u_g, u_g + mu_t]; control_allele_count ~
// Multinomial(pi exp(mu t_ctrl)); the Dirichlet-over-all-guides site is handled per (rep, guide).
//
// Likelihood algebra (same as k_guide_wave2, with the total term first so that no per-timepoint
// value has to be kept): with alpha_b = max((e_b sf_b + eps/B) k m_b, eps), k = a0 / (S + eps):
//   pre-pass   S = sum e_b sf_b;  A0 = sum alpha_b;  d0 = lgamma/digamma difference of (A0, n)
//   main loop  ga_b = d0.dp - dpsi_b (0 on the floor);  S_Q += ga_b k m_b sf_b Q_b;  t_Q += sf_b Q_b;
//              Wa += ga_b alpha_b                         for Q in {P0, P1, t P1}
//   close      d nll / d(weight of Q) = S_Q - Wa inv t_Q
#pragma once

namespace bean {

// LDS per wave: the per-timepoint constants and the two growth columns only (6.3 KB at six timepoints).
// The counts and the per-guide constants used to be staged there too (11.4 KB: 14 single-wave workgroups
// per CU, fewer than the 16 its 128 VGPRs allow); the counts are read from global memory where they are
// used (coalesced rows, twice per step).  BASELINE config 5: 92.7 -> 85.8 us per step.  The kernel is
// VALU-bound (SQ_INSTS_VALU x 4 cycles / 1 024 SIMDs = 39 us) and its 4 689 waves still do not fit the
// 4 096 slots of four waves per SIMD; five waves per SIMD (96 VGPRs: 52 spilled) measured 88.2 us, six
// (80 VGPRs: 78 spilled) 96.3 us.  Two timepoints per iteration through lgamma_digamma_diff2 (the metric kernel's
// two side-by-side chains): 85.8 against 86.2-86.5 us, with 33 instead of 11 spilled registers - not adopted THEN;
// round 5, on the kernel without spills: adopted (the likelihood loop below).
// What the launch's 66 us are (scripts/stamps_surv_guide.py, every wave's start and end on the real-time clock):
// 4 096 waves are resident for the first 25 us; the four waves of a SIMD finish one after another (25, 37, 45,
// 53 us: the oldest wave issues first), and the 593 waves that are left start on the SIMDs that free up first and
// run until 66 us - 593 of the 1 024 SIMDs do five waves' work (5 x 13.2 us) and the others four.  Raising the late
// waves' priority (s_setprio) makes THEM finish early and the older waves of the same SIMDs late: 64.2 us.
// The launch is at its issue bound for whole-wave work items; the balance is a property of 4 689 / 1 024.
// (round 4) + kSurvPark thread-private columns in which values that are loaded with the first batch but needed
// only after the likelihoods wait (log of the observed t0 abundance, the gamma draw of the Dirichlet-over-guides
// site, pi_a0, alpha_pi, q0; with accessibility scaling the two derivatives of the transform): the kernel needed
// 128 VGPRs + 11 spilled (27 with accessibility) to carry them through the timepoint loops; 8.9 KB per wave
// still lets sixteen single-wave workgroups share a CU.
constexpr int kSurvPark = 7;
__host__ __device__ inline size_t guide_survival_wave_lds(int B) {
    return ((size_t)4 * B + (size_t)2 * B * 64 + (size_t)kSurvPark * 64) * sizeof(double);
}

#ifndef BEAN_SURV_EU
#define BEAN_SURV_EU 4
#endif
template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_SURV_EU)))
void k_guide_survival_wave(DevArgs c) {
#define BEAN_SURVIVAL_BODY_INCLUDED_BY_KERNEL
#include "bean_survival_body.hpp"
#undef BEAN_SURVIVAL_BODY_INCLUDED_BY_KERNEL
}

}  // namespace bean
