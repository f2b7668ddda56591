// Seed ensembles: K independent SVI fits of ONE screen in the same launches (bean_hip_svi_run_ensemble).
//
// The pair path of the sorting variant families (k_set_step, k_param<FINISH, ADAM, PREP, KIND>, k_guide_wave2<FAM, ACC>,
// k_loss_finalize) with a member axis: gridDim.y = K, and blockIdx.y is the member.  gridDim.x and blockIdx.x are those
// of a single fit, so every member has the tiles, the block roles and with them the summation order of a single fit
// with guide_offset = 0: member k leaves the bits of bean_hip_svi_run(seed = seeds[k]).
//
// The members' arguments are an array of K DevArgs in global memory (bean_hip_ctx::members_dev).  They differ in what a
// step writes - parameters, gradients, moments, the workspace (each member has a whole private copy of it, taken behind
// bean_hip_prepare, so the data-only rows in it are there for everybody), tsum, the loss accumulators, its row of
// loss_hist - and in the seed; every data pointer, toff, g2t and tdesc are the same K times (with per-member masks bound,
// bean_hip_bind_member_masks, `rg` and `smask` point at the member's slice: see k_prepare_ens).  A block reads its member's
// copy through the scalar cache into SGPRs (dev_args_in_sgprs: nothing in a launch writes the array), which is where a
// kernel argument lives, and runs the body the single-fit kernel runs.  The single-fit kernels themselves are the same
// code objects as before (DESIGN.md lists their register figures side by side).
#pragma once

namespace bean {

constexpr int kEnsembleMaxMembers = 64;  // BEAN_HIP_MAX_MEMBERS of include/bean_hip.h

__global__ __launch_bounds__(256) void k_set_step_ens(const DevArgs* members, unsigned long long step, unsigned long long slot,
                                                      unsigned long long n) {
    const DevArgs c = dev_args_in_sgprs(members + blockIdx.y);
    set_step_body(c, step, slot, n);
}

template <bool FINISH, bool ADAM, bool PREP, int KIND>
__global__ __launch_bounds__(kParamBlock) __attribute__((amdgpu_waves_per_eu(1)))
void k_param_ens(const DevArgs* members, int n_target_blocks) {
    static_assert(KIND == 0 || KIND == 1 || KIND == 2,
                  "the sorting variant families run the generic build or KIND 1, the survival variant ones the generic "
                  "build or KIND 2 (bean_survival_ensemble.hpp)");
    const DevArgs c = dev_args_in_sgprs(members + blockIdx.y);
#define BEAN_PARAM_BODY_INCLUDED_BY_KERNEL
#include "bean_param_body.hpp"
#undef BEAN_PARAM_BODY_INCLUDED_BY_KERNEL
}

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_WAVE_EU)))
void k_guide_wave2_ens(const DevArgs* members) {
    const DevArgs c = dev_args_in_sgprs(members + blockIdx.y);
    const StepCtr ctr = *c.ctrB;
    int tile, r, t0, nt;
    double tot;
    if (!guide_wave2_body<FAM, ACC, 0>(c, ctr, tile, r, t0, nt, tot)) return;
    if (threadIdx.x == 0) {
        wave_loss_out(c, ctr.slot, blockIdx.x, tot);
        if (blockIdx.x == 0) publish_ctr(c, ctr);  // (the member's own counters)
    }
}

// Per-member masks (bean_hip_bind_member_masks): members may also differ in `rg` and `smask`, the two mask arrays the
// kernels above already read through the member's DevArgs.  Three data-only words that k_prepare leaves depend on `rg` -
// the loss constant, the kPNrg row and nobs - so bean_hip_prepare runs k_prepare's body once per member, each on its own
// masks and into its own workspace copy (whose const_acc the host has zeroed; P0 and the bin edges come out as before).
__global__ __launch_bounds__(256) void k_prepare_ens(const DevArgs* members) {
    const DevArgs c = dev_args_in_sgprs(members + blockIdx.y);
#define BEAN_PREPARE_BODY_INCLUDED_BY_KERNEL
#include "bean_prepare_body.hpp"
#undef BEAN_PREPARE_BODY_INCLUDED_BY_KERNEL
}

__global__ __launch_bounds__(256) void k_loss_finalize_ens(const DevArgs* members, unsigned long long first,
                                                           unsigned long long n, int cur) {
    const DevArgs c = dev_args_in_sgprs(members + blockIdx.y);
    loss_finalize_body(c, first, n, cur);
}

}  // namespace bean
