// Survival member fits: K SVI fits of ONE survival variant screen in the same launches (bean_hip_svi_run_ensemble on a
// handle bean_hip_survival_members_supported admits).
//
// The survival variant pair path - k_param<FINISH, ADAM, PREP, 2 | 0>, k_guide_survival_wave<FAM, ACC> and, for the
// NormalModel, k_sum_q - with the member axis of bean_ensemble.hpp: gridDim.y = K, blockIdx.y is the member, gridDim.x and
// blockIdx.x are those of a single fit.  Member k has the tiles, the block roles (q0 blocks first, then the alpha_pi blocks,
// then the target blocks) and the summation order of a single fit, and leaves the bits of bean_hip_svi_run(seed =
// seeds[k]) on its own counts and masks.  k_param_ens (bean_ensemble.hpp) is the parameter kernel; its KIND 2 is the
// survival MixtureNormal build.
//
// Everything a survival step writes is a region of the workspace - u_g, eps_u, gam, gpart, gsum, gq, sq, q0_ctr, wrow,
// dgq, dgt, lpart, the step counters - and a member has a private copy of the whole workspace, so the last-arriving-block
// hand-over of q0_draws_and_totals (q0_ctr counts the member's own q0 blocks; gpart and gsum are the member's) never meets
// another member.  The bodies are the single-fit kernels' text (bean_survival_body.hpp, bean_sum_q_body.hpp); they read
// blockIdx.x alone.
#pragma once

namespace bean {

template <int FAM, bool ACC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(BEAN_SURV_EU)))
void k_guide_survival_wave_ens(const DevArgs* members) {
    const DevArgs c = dev_args_in_sgprs(members + blockIdx.y);
#define BEAN_SURVIVAL_BODY_INCLUDED_BY_KERNEL
#include "bean_survival_body.hpp"
#undef BEAN_SURVIVAL_BODY_INCLUDED_BY_KERNEL
}

__global__ __launch_bounds__(1024) void k_sum_q_ens(const DevArgs* members) {
    const DevArgs c = dev_args_in_sgprs(members + blockIdx.y);
#define BEAN_SUM_Q_BODY_INCLUDED_BY_KERNEL
#include "bean_sum_q_body.hpp"
#undef BEAN_SUM_Q_BODY_INCLUDED_BY_KERNEL
}

}  // namespace bean
