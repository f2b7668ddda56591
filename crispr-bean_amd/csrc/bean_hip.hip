// libbean_hip.so: C ABI over the BEAN SVI kernels (see include/bean_hip.h).
//
// Contents, in this order:
//   context              bean_hip_ctx and ArgSet, the kernel-template dispatch, expected_bytes, sync_devargs, the graph
//                        caches, an ArgSet's device array, the list of workspace regions (workspace_regions)
//   create/bind/prepare  bean_hip_create ... bean_hip_prepare
//   launches             launch_timed, launch_param, launch_guide and its forms, set_step / finalize, elbo_grad / adam
//   stepping             what the entry points share (begin_steps / first_draw / mark_resumable, the noise predicates,
//                        capture_graph / build_ladder / replay_pairs), the whole-call launches (k_svi_tile,
//                        k_svi_async), then bean_hip_svi_run, the seed ensemble (_run_ensemble), the particle steps
//                        (_run_particles), bean_hip_svi_resume
//   sharded / comm       bean_hip_sharded_*, bean_hip_comm_*, bean_hip_svi_run_exchanged
//   introspection        step_bytes, dominant_kernel*, profile, diagnostics
// Which entry point replays which graph ladder: the table in DESIGN.md, section 1.
// (Kernel templates are instantiated in the order this file first names them, and that is their order in the code
// object: moving a launcher moves device code, which scripts/kernel_resources_diff.py and a disassembly diff then show.)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: the functions are resolved with dlsym (bean_hip_comm_*)

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/bean_hip.h"
#include "bean_kernels.hpp"
#include "bean_predictive.hpp"  // replicate counts drawn on the device (bean_hip_simulate)
#include "bean_importance.hpp"  // per-target log importance weights (bean_hip_log_weights)
#include "bean_importance_marg.hpp"  // ... with pi integrated out (bean_hip_log_weights_marginal)
#include "bean_grid.hpp"  // the same log joint at given (mu, y) per target and node (bean_hip_marginal_grid)
#include "bean_jacobi.hpp"  // ... with a Gauss-Jacobi rule for the pairs the predicate leaves out (bean_hip_marginal_grid_tail)
#include "bean_importance_tail.hpp"  // that rule for the marginal importance weights (bean_hip_log_weights_marginal_tail)
#include "bean_survival_predictive.hpp"  // replicate counts of a survival screen (bean_hip_simulate_survival, _members)

using namespace bean;

static thread_local std::string g_err;
static int fail(const std::string& msg) {
    g_err = msg;
    return -1;
}
#define HIP_OK(expr)                                                                 \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess)                                                        \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// ------------------------------------------------------------------ context
// The arguments of the n copies of a fit that the `_ens` launches step together - the members of an ensemble, or the
// particles of a fit - and the ladder of graphs that replays those launches.  A handle has one set of each kind, and
// both can be live: a particle handle is also an ensemble of one (bean_hip_svi_run_ensemble).
struct ArgSet {
    DevArgs* dev = nullptr;             // device: DevArgs of the n copies; the launches, captured ones too, hold its address
    std::vector<DevArgs> host;          // what `dev` holds
    std::vector<uint64_t> seeds;        // ... and the seeds it was built with
    bool dirty = true;                  // `dev` is older than the bound buffers
    std::vector<hipGraphExec_t> ladder; // [k]: 2^k units of the set's entry point (the table in DESIGN.md, section 1)
};

// (what is not set here, bean_hip_create sets from the shape and the environment)
struct bean_hip_ctx {
    bean_hip_shape shape = {};
    DevArgs d = {};
    void* slot_ptr[BEAN_BUF_COUNT] = {};
    uint64_t slot_bytes[BEAN_BUF_COUNT] = {};
    void* workspace = nullptr;
    uint64_t workspace_bytes = 0;
    uint64_t loss_capacity = 0;
    bool prepared = false;
    bool fused_guide = true;  // false: BEAN_HIP_GUIDE=split selects the sample / lik / pi-terms launches
    bool wave_guide = false;  // sorting variant families, default: one wave per (guide tile, replicate)
    bool wave2 = false;       // ... in its second form, k_guide_wave2 (BEAN_HIP_GUIDE=wave1 selects the first)
    bool surv_wave = false;   // survival variant families: k_guide_survival_wave (BEAN_HIP_SURVIVAL=block: k_guide_survival)
    bool fused_step = false;  // bean_hip_svi_run steps with ONE launch, k_step_wave2 (bean_step_v2.hpp; BEAN_HIP_STEP=pair: two)
    std::vector<hipGraphExec_t> graphs_fused;  // [k]: 2^(k+1) launches of k_step_wave2
    long long* loss_acc = nullptr;  // library-owned fixed-point loss accumulators, kLossWords per loss_hist slot
    int* tile_targets_dev = nullptr;  // (in the workspace: workspace_regions)
    double* tsum_buf = nullptr;   // DevArgs::tsum / tdesc (sized by bean_hip_prepare: they depend on tile_targets)
    int2* tdesc_buf = nullptr;
    int* live_slots = nullptr;   // tiling: compact list of the allele slots that hold an allele (own allocation, (A - 1) G ints)
    bool tiling_wave = false;  // tiling families, default: k_guide_tiling_wave (BEAN_HIP_TILING=block: k_guide_tiling)
    bool tiling_wide = false;  // more alleles per guide than this build's kAMax: bean_tiling_wide.hpp
    int tiling_rep_w = 0;      // ... with this many waves per workgroup
    bool tiling_rep = false;   // tiling families, default: k_guide_tiling_rep, the replicates of a guide share a wave (bean_tiling_v2.hpp)
    // tiling: the allele tables (tabP, tabPmu, tabPy, mu_a, sig_a) belong to the draw that is on the device.  A PREP launch
    // of k_param<..., 3> with allele blocks leaves them so (round 5); any other PREP launch leaves a new draw and stale
    // tables, and launch_guide runs k_allele first.  BEAN_HIP_ALLELE=split: k_param never has allele blocks (A/B).
    bool alleles_fresh = false;
    bool allele_blocks = true;
    bool resume_head_fresh = false;  // the resume graphs were captured with fresh tables at their head (their first node is a guide launch)
    // in the workspace (workspace_regions); sync_devargs puts the caller's exchange buffer in their place when one is bound
    double* gsum_ws = nullptr;     // normaliser buffer (replaced by BEAN_BUF_XCHG_GSUM when bound)
    double* sq_ws = nullptr;       // projection sums (replaced by BEAN_BUF_XCHG_SQ when bound)
    double* cov_sum_ws = nullptr;  // covariate gradient sums (replaced by BEAN_BUF_XCHG_COV when bound)
    // graph cache: graphs[k] replays 2^k {k_param, guide} pairs
    std::vector<hipGraphExec_t> graphs;
    unsigned long long graph_seed = 0;
    // profiling of the dominant kernel
    bool profile = false;
    bool profile_param = false;  // profile mode 2: time k_param<FINISH, ADAM, PREP> instead of the guide kernel
    std::vector<hipEvent_t> ev;  // start/stop pairs
    // one launch per call for the variant sorting families (bean_tile_svi.hpp): target-aligned tiles
    bool tile_svi = false;    // eligible shape and not switched off (BEAN_HIP_STEP=pair)
    bool tile_ready = false;  // tile table built by bean_hip_prepare
    int* tile_tab = nullptr;  // device: tile_g0[n_tiles + 1], tile_t0[n_tiles + 1]
    int n_tiles = 0, tile_ntm = 0, tile_gbm = 0, tile_blocks = 0;
    float* step_sizes = nullptr;   // device: ClippedAdam step sizes of the steps of one call
    DevArgs* dargs_dev = nullptr;  // device copy of DevArgs for k_svi_tile's out-of-line pieces
    uint64_t step_sizes_cap = 0;
    std::vector<uint64_t> ev_steps;  // profile mode: SVI steps covered by each timed launch
    // RCCL communicator of a guide-sharded fit (bean_hip_comm_init) and graphs of 2^k exchanged steps
    ncclComm_t comm = nullptr;
    int comm_world = 0;
    std::vector<hipGraphExec_t> graphs_xchg;
    // bean_hip_svi_resume: graphs of 2^k {guide, k_param<FINISH, ADAM, PREP>} pairs, and what the last call left
    // prepared on the device: the draw and tables of step resume_next (same seed, same stream)
    std::vector<hipGraphExec_t> graphs_resume;
    bool resume_ok = false;
    uint64_t sharded_steps = 0;  // bean_hip_sharded_update calls since bean_hip_sharded_begin: the slots its last call finalizes
    uint64_t resume_next = 0, resume_seed = 0;
    void* resume_stream = nullptr;
    // all the steps of a call in ONE launch, tile-asynchronous (bean_async_v2.hpp): eligible shape and switched on
    bool async_step = false;
    bool dirgrad_tab = true;  // DevArgs::dgt is allocated and filled (BEAN_HIP_DIRGRAD_TAB=0 at create: not, A/B)
    int* async_ws = nullptr;   // device: 8 queue counters (kAsyncQueueStride apart), the abort word, done[n_tiles]
    int async_blocks = 0;      // grid: resident single-wave workgroups that pull items, a multiple of 8 (0: not yet measured)
    int async_fin_blocks = 0;  // ... and that only finish tiles (0: no roles, the last arriver finishes)
    int async_early = 1;       // the targets' part of a finish ahead of the finisher's poll (BEAN_HIP_ASYNC_EARLY at create: 0 / 1 / 2,
                               // AsyncArgs::early; A/B and the tests' three paths)
    size_t async_ws_ints = 0;
    unsigned long long* async_stamps = nullptr;  // diagnostic builds (-DBEAN_ASYNC_STAMP): the last call's item timeline
    size_t async_stamp_words = 0;
    // seed ensemble (bean_ensemble.hpp): K members stepped by the same launches.  Member 0 is `d` itself; member k >= 1
    // has the k-th private copy of the workspace (member_ws), of tsum_buf and of loss_acc, and the k-th part of the
    // member-major parameter / gradient / moment / loss_hist buffers
    int n_members = 1;
    bool bound_any = false;       // a buffer has been bound: bean_hip_set_members comes too late
    char* member_ws = nullptr;    // (K - 1) copies of the workspace, member_ws_stride bytes apart
    size_t member_ws_stride = 0;
    size_t tsum_stride = 0;       // doubles of tsum per member
    ArgSet members;               // member_args of the K members; ladder of {k_param_ens, k_guide_wave2_ens} pairs
    // per-member masks (bean_hip_bind_member_masks): (K, R, G) uint8 and (K, R, B) float64 of the caller, member-major;
    // null: every member reads the shared BEAN_BUF_REPGUIDE / BEAN_BUF_SAMPLE_MASK
    bool members_set = false;     // bean_hip_set_members has been called
    const uint8_t* member_rg = nullptr;
    const double* member_smask = nullptr;
    // per-member counts (bean_hip_bind_member_counts): (K, R, B, G) float32 of the caller, member-major; null: every
    // member reads the shared BEAN_BUF_X / BEAN_BUF_X_BC
    const float* member_x = nullptr;
    const float* member_xbc = nullptr;
    // multi-particle SVI (bean_particles.hpp): P draws per step, one update with their mean gradient.  The particles are
    // members that share the caller's single-fit parameters and moments; particle p >= 1 has the p-th private copy of the
    // workspace (member_ws), of tsum_buf and of loss_acc, and every particle row p of particle_grad and particle_loss
    int n_particles = 1;
    bool particles_set = false;       // bean_hip_set_particles has been called
    float* particle_grad = nullptr;   // per parameter array a (P, n) float32 block, the arrays end to end (particle_arrays)
    double* particle_loss = nullptr;  // (P, loss_capacity) losses of the particles; the caller's loss_hist holds their mean
    ArgSet particles;                 // particle_args of the P particles; ladder of particle steps (four launches each)
    // bean_hip_marginal_grid_tail (bean_jacobi.hpp): grown on demand, never read by a fit
    int* tail_off = nullptr;          // (T + 1) list offsets, then (T) counts for bean_hip_marginal_tail_nodes
    void* tail_ws = nullptr;          // nodes, log weights, tail_pair_err, pair indices, sides of the last call
    uint64_t tail_ws_bytes = 0;
};

extern "C" const char* bean_hip_version(void) {
    return BEAN_AMAX <= 8 ? "bean_hip 0.1.0 (gfx950)"
                          : (BEAN_AMAX <= 16 ? "bean_hip 0.1.0 (gfx950, 16 alleles per guide / 16 conditions)"
                                             : "bean_hip 0.1.0 (gfx950, 32 alleles per guide / 16 conditions)");
}
extern "C" const char* bean_hip_last_error(void) { return g_err.c_str(); }

static bool is_survival(const bean_hip_shape& s) { return s.selection == BEAN_SELECTION_SURVIVAL; }
static bool is_tiling(const bean_hip_shape& s) { return s.family == BEAN_FAMILY_MULTI_MIXTURE; }
// families with a Dirichlet pi site (reporter models)
// survival NormalModel: the drawn initial guide abundance q_0 ~ Dirichlet over ALL guides enters
// the likelihood (survival_model.py:15-130, 629-648)
static bool is_surv_normal(const bean_hip_shape& s) {
    return s.selection == BEAN_SELECTION_SURVIVAL && s.family == BEAN_FAMILY_NORMAL;
}
static bool is_mixture(const bean_hip_shape& s) {
    return s.family == BEAN_FAMILY_MIXTURE_NORMAL || s.family == BEAN_FAMILY_MULTI_MIXTURE;
}

// The kernel-template dispatch, once each: f is a generic lambda that names its kernel as k<fam(), acc()>.
// family x accessibility of the variant kernels: <kMixture, true>, <kMixture, false>, <kNormal, false>
template <typename F>
static auto with_family_acc(const DevArgs& d, F&& f) {
    if (d.family == kMixture) {
        if (d.flags & kAcc) return f(std::integral_constant<int, kMixture>{}, std::true_type{});
        return f(std::integral_constant<int, kMixture>{}, std::false_type{});
    }
    return f(std::integral_constant<int, kNormal>{}, std::false_type{});
}
// accessibility x survival of the tiling kernels
template <typename F>
static auto with_acc_surv(const DevArgs& d, F&& f) {
    if (d.survival) {
        if (d.flags & kAcc) return f(std::true_type{}, std::true_type{});
        return f(std::false_type{}, std::true_type{});
    }
    if (d.flags & kAcc) return f(std::true_type{}, std::false_type{});
    return f(std::false_type{}, std::false_type{});
}

// Bytes the shape implies for a slot (0 = slot not used by this shape).
static uint64_t expected_bytes(const bean_hip_shape& s, int slot) {
    const uint64_t R = s.n_reps, B = s.n_condits, G = s.n_guides, T = s.n_targets;
    const uint64_t A = s.n_max_alleles, C = s.n_ctrl;
    auto param_elems = [&](int i) -> uint64_t {
        switch (i) {
            case 0: case 1: return T;
            case 2: case 3: return is_survival(s) ? 0 : T;  // survival models have no sd latent
            case 7: return ((is_survival(s) && s.family == BEAN_FAMILY_MIXTURE_NORMAL) || is_surv_normal(s)) ? G : 0;
            case 4: return is_mixture(s) ? G * A : 0;
            case 5: case 6:
                if (s.n_sample_covariates > 0) return (uint64_t)s.n_sample_covariates;  // mu_cov_loc / mu_cov_scale
                return (is_mixture(s) && (s.flags & BEAN_FLAG_SCALE_BY_ACC) && (s.flags & BEAN_FLAG_FIT_NOISE)) ? G : 0;
        }
        return 0;
    };
    if (slot >= BEAN_BUF_P_MU_LOC && slot < BEAN_BUF_P_MU_LOC + 8) return 4 * param_elems(slot - BEAN_BUF_P_MU_LOC);
    if (slot >= BEAN_BUF_G_MU_LOC && slot < BEAN_BUF_G_MU_LOC + 8) return 4 * param_elems(slot - BEAN_BUF_G_MU_LOC);
    if (slot >= BEAN_BUF_M_MU_LOC && slot < BEAN_BUF_M_MU_LOC + 8) return 4 * param_elems(slot - BEAN_BUF_M_MU_LOC);
    if (slot >= BEAN_BUF_V_MU_LOC && slot < BEAN_BUF_V_MU_LOC + 8) return 4 * param_elems(slot - BEAN_BUF_V_MU_LOC);
    switch (slot) {
        case BEAN_BUF_X: return 4 * R * B * G;
        case BEAN_BUF_X_BC: return (s.flags & BEAN_FLAG_USE_BCMATCH) ? 4 * R * B * G : 0;
        case BEAN_BUF_ALLELE_CTRL: return is_mixture(s) ? 4 * R * C * G * A : 0;
        case BEAN_BUF_REPGUIDE: return R * G;
        case BEAN_BUF_SIZE_FACTOR: return 8 * R * B;
        case BEAN_BUF_SIZE_FACTOR_BC: return (s.flags & BEAN_FLAG_USE_BCMATCH) ? 8 * R * B : 0;
        case BEAN_BUF_SAMPLE_MASK: return 8 * R * B;
        case BEAN_BUF_A0: return 8 * G;
        case BEAN_BUF_A0_BC: return (s.flags & BEAN_FLAG_USE_BCMATCH) ? 8 * G : 0;
        case BEAN_BUF_PI_A0: return is_mixture(s) ? 8 * G : 0;
        case BEAN_BUF_Z_HI: case BEAN_BUF_Z_LO: return is_survival(s) ? 0 : 8 * B;
        case BEAN_BUF_TIMEPOINTS: return is_survival(s) ? 8 * B : 0;
        case BEAN_BUF_CONTROL_TIME: return (is_survival(s) && is_mixture(s)) ? 8 * C : 0;
        case BEAN_BUF_LOG_OBS0: return (is_survival(s) && s.family == BEAN_FAMILY_MIXTURE_NORMAL) ? 8 * R * G : 0;
        case BEAN_BUF_X0_IN: case BEAN_BUF_X0_OUT:
            return ((is_survival(s) && s.family == BEAN_FAMILY_MIXTURE_NORMAL) || is_surv_normal(s)) ? 8 * R * G : 0;
        case BEAN_BUF_NEGCTRL_MASK: return is_surv_normal(s) ? G : 0;
        case BEAN_BUF_XCHG_GSUM:
            return ((is_survival(s) && s.family == BEAN_FAMILY_MIXTURE_NORMAL) || is_surv_normal(s)) ? 8 * (R + 1) : 0;
        case BEAN_BUF_XCHG_SQ: return is_surv_normal(s) ? 8 * R : 0;
        case BEAN_BUF_XCHG_TGRAD: return 8 * 2 * T;
        case BEAN_BUF_XCHG_COV: return s.n_sample_covariates > 0 ? 8 * R : 0;
        case BEAN_BUF_EPS_U_IN: case BEAN_BUF_EPS_U_OUT: return (is_survival(s) && is_mixture(s)) ? 8 * G : 0;
        case BEAN_BUF_GUIDE_IDS: return is_tiling(s) ? 4 * G : 0;
        case BEAN_BUF_PRIOR_IA: return (is_surv_normal(s) && s.prior_ia_total > 0.0) ? 8 * G : 0;
        case BEAN_BUF_TARGET_OFFSETS: return is_tiling(s) ? 0 : 4 * (T + 1);
        case BEAN_BUF_GUIDE_TO_TARGET: return is_tiling(s) ? 0 : 4 * G;
        case BEAN_BUF_A2E_PTR: return is_tiling(s) ? 4 * (G * (A - 1) + 1) : 0;
        case BEAN_BUF_A2E_IDX: case BEAN_BUF_E2A_IDX: return is_tiling(s) ? 4 * (uint64_t)s.n_a2e_nnz : 0;
        case BEAN_BUF_E2A_PTR: return is_tiling(s) ? 4 * ((uint64_t)s.n_edits + 1) : 0;
        case BEAN_BUF_ALLELE_MASK: return is_tiling(s) ? G * A : 0;
        case BEAN_BUF_ACCESSIBILITY: return (s.flags & BEAN_FLAG_SCALE_BY_ACC) ? 8 * G : 0;
        case BEAN_BUF_PRIOR_MU_LOC: case BEAN_BUF_PRIOR_MU_SCALE:
        case BEAN_BUF_PRIOR_SD_LOC: case BEAN_BUF_PRIOR_SD_SCALE: return 8 * T;
        case BEAN_BUF_EPS_MU_IN: case BEAN_BUF_EPS_MU_OUT: return 8 * T;
        case BEAN_BUF_EPS_SD_IN: case BEAN_BUF_EPS_SD_OUT: return is_survival(s) ? 0 : 8 * T;
        case BEAN_BUF_PI_IN: case BEAN_BUF_PI_OUT: return is_mixture(s) ? 8 * R * G * A : 0;
        case BEAN_BUF_EPS_NOISE_IN: case BEAN_BUF_EPS_NOISE_OUT:
            if (s.n_sample_covariates > 0) return 8 * (uint64_t)s.n_sample_covariates;  // eps of mu_cov
            return (s.flags & BEAN_FLAG_SCALE_BY_ACC) ? 8 * G : 0;
        case BEAN_BUF_REP_BY_COV: return 8 * R * (uint64_t)(s.n_sample_covariates > 0 ? s.n_sample_covariates : 0);
        case BEAN_BUF_LOSS_HIST: return 8;  // minimum; any multiple of 8 accepted
    }
    return 0;
}

static void sync_devargs(bean_hip_ctx* c) {
    DevArgs& d = c->d;
    auto P = [&](int s) { return c->slot_ptr[s]; };
    d.X = (const float*)P(BEAN_BUF_X);
    d.Xbc = (const float*)P(BEAN_BUF_X_BC);
    d.allele = (const float*)P(BEAN_BUF_ALLELE_CTRL);
    d.rg = (const uint8_t*)P(BEAN_BUF_REPGUIDE);
    d.sf = (const double*)P(BEAN_BUF_SIZE_FACTOR);
    d.sf_bc = (const double*)(P(BEAN_BUF_SIZE_FACTOR_BC) ? P(BEAN_BUF_SIZE_FACTOR_BC) : P(BEAN_BUF_SIZE_FACTOR));
    d.smask = (const double*)P(BEAN_BUF_SAMPLE_MASK);
    d.a0 = (const double*)P(BEAN_BUF_A0);
    d.a0_bc = (const double*)P(BEAN_BUF_A0_BC);
    d.pi_a0 = (const double*)P(BEAN_BUF_PI_A0);
    d.z_hi = (const double*)P(BEAN_BUF_Z_HI);
    d.z_lo = (const double*)P(BEAN_BUF_Z_LO);
    d.acc = (const double*)P(BEAN_BUF_ACCESSIBILITY);
    d.a2e_ptr = (const int*)P(BEAN_BUF_A2E_PTR);
    d.a2e_idx = (const int*)P(BEAN_BUF_A2E_IDX);
    d.e2a_ptr = (const int*)P(BEAN_BUF_E2A_PTR);
    d.e2a_idx = (const int*)P(BEAN_BUF_E2A_IDX);
    d.amask = (const uint8_t*)P(BEAN_BUF_ALLELE_MASK);
    d.toff = (const int*)P(BEAN_BUF_TARGET_OFFSETS);
    d.g2t = (const int*)P(BEAN_BUF_GUIDE_TO_TARGET);
    d.pr_mu_loc = (const double*)P(BEAN_BUF_PRIOR_MU_LOC);
    d.pr_mu_scale = (const double*)P(BEAN_BUF_PRIOR_MU_SCALE);
    d.pr_sd_loc = (const double*)P(BEAN_BUF_PRIOR_SD_LOC);
    d.pr_sd_scale = (const double*)P(BEAN_BUF_PRIOR_SD_SCALE);
    for (int i = 0; i < 8; ++i) {
        d.p[i] = (float*)P(BEAN_BUF_P_MU_LOC + i);
        d.g[i] = (float*)P(BEAN_BUF_G_MU_LOC + i);
        d.m[i] = (float*)P(BEAN_BUF_M_MU_LOC + i);
        d.v[i] = (float*)P(BEAN_BUF_V_MU_LOC + i);
    }
    d.eps_mu_in = (const double*)P(BEAN_BUF_EPS_MU_IN);
    d.eps_sd_in = (const double*)P(BEAN_BUF_EPS_SD_IN);
    d.pi_in = (const double*)P(BEAN_BUF_PI_IN);
    d.eps_noise_in = (const double*)P(BEAN_BUF_EPS_NOISE_IN);
    d.eps_mu_out = (double*)P(BEAN_BUF_EPS_MU_OUT);
    d.eps_sd_out = (double*)P(BEAN_BUF_EPS_SD_OUT);
    d.pi_out = (double*)P(BEAN_BUF_PI_OUT);
    d.eps_noise_out = (double*)P(BEAN_BUF_EPS_NOISE_OUT);
    d.loss_hist = (double*)P(BEAN_BUF_LOSS_HIST);
    d.loss_acc = c->loss_acc;
    d.time = (const double*)P(BEAN_BUF_TIMEPOINTS);
    d.negctrl = (const uint8_t*)P(BEAN_BUF_NEGCTRL_MASK);
    d.rbc = (const double*)P(BEAN_BUF_REP_BY_COV);
    d.prior_ia = (const double*)P(BEAN_BUF_PRIOR_IA);
    d.gid = (const int*)P(BEAN_BUF_GUIDE_IDS);
    d.prior_ia_total = c->shape.prior_ia_total;
    if (P(BEAN_BUF_XCHG_GSUM)) d.gsum = (double*)P(BEAN_BUF_XCHG_GSUM);
    else d.gsum = c->gsum_ws;
    if (P(BEAN_BUF_XCHG_SQ)) d.sq = (double*)P(BEAN_BUF_XCHG_SQ);
    else d.sq = c->sq_ws;
    if (c->cov_sum_ws) d.cov_sum = P(BEAN_BUF_XCHG_COV) ? (double*)P(BEAN_BUF_XCHG_COV) : c->cov_sum_ws;
    d.ctrl_time = (const double*)P(BEAN_BUF_CONTROL_TIME);
    d.log_obs0 = (const double*)P(BEAN_BUF_LOG_OBS0);
    d.x0_in = (const double*)P(BEAN_BUF_X0_IN);
    d.eps_u_in = (const double*)P(BEAN_BUF_EPS_U_IN);
    d.x0_out = (double*)P(BEAN_BUF_X0_OUT);
    d.eps_u_out = (double*)P(BEAN_BUF_EPS_U_OUT);
    d.flags = c->shape.flags & ~kDumpPi;
    if (d.pi_out && (c->shape.flags & BEAN_FLAG_DUMP_PI)) d.flags |= kDumpPi;
}

static void destroy_graphs(std::vector<hipGraphExec_t>& graphs) {
    for (hipGraphExec_t g : graphs)
        if (g) (void)hipGraphExecDestroy(g);
    graphs.clear();
}

static void drop_graph(bean_hip_ctx* c) {
    destroy_graphs(c->graphs);
    destroy_graphs(c->graphs_fused);
    destroy_graphs(c->graphs_xchg);
    destroy_graphs(c->graphs_resume);
    for (ArgSet* a : {&c->members, &c->particles}) {
        destroy_graphs(a->ladder);
        a->dirty = true;
    }
    c->resume_ok = false;  // (called whenever a buffer, the shape-dependent state or the seed changes)
}

// The captured launches hold DevArgs - and with it the seed - BY VALUE, and the four graph families share ONE
// graph_seed: every stepping entry point therefore drops ALL the families when the seed changes, whichever of them
// it replays itself (run(A), resume(B), run(B) used to replay run's graphs with A baked in).
static void drop_graph_on_seed_change(bean_hip_ctx* c, unsigned long long seed) {
    const bool any = !c->graphs.empty() || !c->graphs_fused.empty() || !c->graphs_xchg.empty() || !c->graphs_resume.empty();
    if (any && c->graph_seed != seed) drop_graph(c);
}

// ---- an ArgSet's device array, and bringing it up to date
static void free_args(ArgSet& a) {
    destroy_graphs(a.ladder);  // (they hold the array's address)
    if (a.dev) (void)hipFree(a.dev);
    a.dev = nullptr;
    a.seeds.clear();
    a.dirty = true;
}
static int alloc_args(ArgSet& a, int n) {
    free_args(a);
    HIP_OK(hipMalloc((void**)&a.dev, (size_t)n * sizeof(DevArgs)));
    return 0;
}
// The n copies' arguments, copy k as make(k, seeds[k]) gives it now, to the device array - unless the array was built
// with these seeds and nothing has been bound since.  (The launches hold the ADDRESS of the array: new seeds need no
// new graphs.)
template <typename Make>
static int refresh_args(ArgSet& a, int n, const uint64_t* seeds, hipStream_t stream, Make&& make) {
    bool same = !a.dirty && (int)a.seeds.size() == n;
    for (int k = 0; same && k < n; ++k) same = a.seeds[(size_t)k] == seeds[k];
    if (same) return 0;
    HIP_OK(hipStreamSynchronize(stream));  // no launch in flight reads the array while it changes
    a.host.resize((size_t)n);
    for (int k = 0; k < n; ++k) a.host[(size_t)k] = make(k, seeds[k]);
    HIP_OK(hipMemcpyAsync(a.dev, a.host.data(), (size_t)n * sizeof(DevArgs), hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));
    a.seeds.assign(seeds, seeds + n);
    a.dirty = false;
    return 0;
}

// ---- the workspace: ONE list of its regions
// Every region of the workspace, in allocation order: v(pointer that owns the region, its size in doubles).  The
// pointers are fields of `d` (tile_targets_dev, which is not one, comes back through `tile_targets_dev`).  The list has
// three uses and no second copy: bean_hip_create sums the sizes, then hands out the allocation region by region
// (c->d), and relocate_private moves a member's or particle's pointers to its own copy of the workspace.  A region the
// shape does not have is not visited and its pointer stays null.  Needs the shape-dependent switches of `c` and the
// scalars of `d` that bean_hip_create sets ahead of its first use (n_cov, n_tiles, n_gamma_blocks, n_arrival_ctr,
// n_lpart).
template <typename V>
static void workspace_regions(const bean_hip_ctx* c, DevArgs& d, V&& v, int** tile_targets_dev = nullptr) {
    const bean_hip_shape& s = c->shape;
    const bool tiling = is_tiling(s), surv = is_survival(s);
    const bool surv_mix = surv && s.family == BEAN_FAMILY_MIXTURE_NORMAL, surv_norm = is_surv_normal(s);
    const uint64_t R = (uint64_t)d.R, B = (uint64_t)d.B, G = (uint64_t)d.G, T = (uint64_t)d.T, n_cov = (uint64_t)d.n_cov;
    const uint64_t A1 = tiling ? (uint64_t)(d.A - 1) : 0;
    auto opt = [&](auto& p, uint64_t n) {
        if (n) v(p, n);
    };
    // tables: a column per allele slot, or per target (per replicate and target with sample covariates)
    const uint64_t n_tab = B * (tiling ? A1 * G : T * (n_cov ? R : 1));
    v(d.tabP, n_tab);
    v(d.tabPmu, n_tab);
    v(d.tabPy, n_tab);
    v(d.P0, B);
    v(d.mu_t, T);
    v(d.y_t, T);
    v(d.eps_mu, T);
    v(d.eps_sd, T);
    v(d.part, (uint64_t)(tiling ? (d.A > kAMax ? tq_num(d.A) : kTNumPart) : kNumPart) * G);
    v(d.mu_a, A1 * G);
    v(d.sig_a, A1 * G);
    v(d.lpn, G);
    v(d.eps_noise, G);
    opt(d.kacc, (s.flags & BEAN_FLAG_SCALE_BY_ACC) ? G : 0);  // filled by bean_hip_prepare (k_acc_scale)
    v(d.loss_const, 1);
    v(d.const_acc, kLossWords);
    int* tile_targets = nullptr;  // two ints: k_tile_targets, k_max_target_len
    v(tile_targets, 1);
    if (tile_targets_dev) *tile_targets_dev = tile_targets;
    // arrival counters, n_arrival_ctr ints that k_set_step zeroes from tile_ctr on.  The fused step kernel's: per tile and
    // per tile boundary, half each, then the distinct bin edges.  Tiling: k_param's allele blocks' counters and go flags
    if (c->wave2) {
        v(d.tile_ctr, (uint64_t)d.n_arrival_ctr / 4);
        v(d.bnd_ctr, (uint64_t)d.n_arrival_ctr / 4);
        v(d.ue_z, 2 * B);
        v(d.ue_idx, B + 2);  // 2 B + 1 ints
    } else {
        opt(d.tile_ctr, (uint64_t)d.n_arrival_ctr / 2);
    }
#ifdef BEAN_STAMP
    v(d.dbg, 8 * 2 * R * (((uint64_t)((G + 63) / 64 + 1) + 7) / 8 * 8));
#endif
    // per-replicate rows of the guide kernels
    if (c->tiling_wave || c->tiling_wide) v(d.trow, (uint64_t)(c->tiling_wave ? kTNumPart : tq_num(d.A)) * R * G);
    if (c->wave_guide && c->wave2) {
        v(d.wrow, (uint64_t)kW2Rows * R * G);  // count totals are re-summed in the kernel: no nobs
    } else if (c->wave_guide) {
        v(d.wrow, (uint64_t)kNumPart * R * G);
        v(d.nobs, 2 * R * G);
    } else if (c->surv_wave) {
        v(d.wrow, (uint64_t)kW2Rows * R * G);
    }
    if (!surv && !tiling && !c->fused_guide) {  // the split form
        v(d.rrow, 3 * R * G);
        if (is_mixture(s)) {
            v(d.pi_ws, 2 * R * G);
            v(d.gpi_ws, 2 * R * G);
        }
    }
    // survival: the baseline draw; the Dirichlet-over-all-guides site (gsum: gsum_ws); where q_0 enters the likelihood,
    // its gradient rows and their projection sums (sq: sq_ws)
    if (surv_mix || (surv && tiling)) {
        v(d.u_g, G);
        v(d.eps_u, G);
    }
    if (surv_mix || surv_norm) {
        v(d.gam, R * G);
        v(d.gpart, (uint64_t)d.n_gamma_blocks * (R + 1));
        v(d.gsum, R + 1);
    }
    if (surv_norm) {
        v(d.gq, R * G);
        v(d.sq, R);
    }
    if (n_cov) {
        v(d.cov_mu, n_cov);
        v(d.cov_eps, n_cov);
        v(d.cov_shift, R);
        v(d.cov_sum, R);  // (cov_sum_ws)
    }
    const bool wave_rows = c->wave2 || c->surv_wave;
    opt(d.dgq, (wave_rows && s.family == BEAN_FAMILY_MIXTURE_NORMAL) ? 6 * G : 0);
    opt(d.dgt, (c->dirgrad_tab && wave_rows && s.family == BEAN_FAMILY_MIXTURE_NORMAL) ? 2 * (uint64_t)kDgtRows * G : 0);
    opt(d.dgq_t, (c->tiling_wave || c->tiling_rep) ? (uint64_t)(kAMax + 1) * G : 0);
    opt(d.lpart, 3 * (uint64_t)d.n_lpart);  // per-wave loss parts of the wave-form guide kernels
    v(d.q0_ctr, 1);
    static_assert(sizeof(StepCtr) == 24, "a StepCtr takes three doubles");
    v(d.ctrA, 3);
    v(d.ctrB, 3);
    // Nobody's: the closed formula that sized the workspace before this list counted 2 doubles more than it handed out,
    // and the covariate shifts and sums (2 R) for every shape.  Kept, at the end, so that workspace_bytes and the
    // members' stride are what they were; shrinking it is a change of its own.
    double* spare = nullptr;
    v(spare, 2 + (n_cov ? 0 : 2 * R));
}

// ------------------------------------------------------------------ create / bind / prepare
extern "C" int bean_hip_create(const bean_hip_shape* s, bean_hip_ctx** out) {
    if (!s || !out) return fail("bean_hip_create: null argument");
    if (s->selection != BEAN_SELECTION_SORTING && s->selection != BEAN_SELECTION_SURVIVAL)
        return fail("bean_hip_create: unknown selection");
    if (is_survival(*s) && !(s->negctrl_scale > 0.0)) return fail("bean_hip_create: negctrl_scale must be > 0");
    if (s->family < BEAN_FAMILY_NORMAL || s->family > BEAN_FAMILY_MULTI_MIXTURE)
        return fail("bean_hip_create: unknown family");
    if (s->n_reps < 1 || s->n_guides < 1 || s->n_targets < 1)
        return fail("bean_hip_create: R, G, T must be >= 1");
    if (s->n_condits < 1 || s->n_condits > kBCap)
        return fail("bean_hip_create: n_condits must be in [1, " + std::to_string(kBCap) +
                    "] (libbean_hip.so holds 8 conditions, libbean_hip_a16.so 64)");
    if (s->family == BEAN_FAMILY_MIXTURE_NORMAL && s->n_max_alleles != 2)
        return fail("bean_hip_create: MixtureNormal requires n_max_alleles == 2");
    if (is_tiling(*s)) {
        if (s->n_max_alleles < 2 || s->n_max_alleles > kWideMaxA)
            return fail("bean_hip_create: MultiMixtureNormal requires n_max_alleles in [2, " + std::to_string(kWideMaxA) +
                        "] (up to " + std::to_string(kAMax) + " alleles per guide run in the register-resident kernels "
                        "of this build, more in the allele-parallel ones)");
        if (s->n_edits < 1 || s->n_targets != s->n_edits)
            return fail("bean_hip_create: MultiMixtureNormal requires n_targets == n_edits >= 1");
        if (s->n_a2e_nnz < 0) return fail("bean_hip_create: n_a2e_nnz must be >= 0");
    }
    if (is_mixture(*s) && s->n_ctrl < 1) return fail("bean_hip_create: MixtureNormal requires n_ctrl >= 1");
    if (s->family == BEAN_FAMILY_CONTROL_NORMAL && s->n_targets != 1)
        return fail("bean_hip_create: ControlNormal requires n_targets == 1");
    if (!(s->lrd > 0.0) || !(s->initial_lr > 0.0)) return fail("bean_hip_create: lr and lrd must be > 0");
    if (s->n_sample_covariates < 0 || s->n_sample_covariates > 64)
        return fail("bean_hip_create: n_sample_covariates must be in [0, 64]");
    if (s->n_sample_covariates > 0 && !(s->family == BEAN_FAMILY_NORMAL && s->selection == BEAN_SELECTION_SORTING))
        return fail("bean_hip_create: sample covariates belong to the sorting NormalModel only (bean/model/model.py:73-91)");
    if (s->guide_offset < 0 || s->target_offset < 0 ||
        (s->n_guides_total > 0 && s->guide_offset + s->n_guides > s->n_guides_total))
        return fail("bean_hip_create: shard offsets outside the whole screen");

    bean_hip_ctx* c = new bean_hip_ctx();
    c->shape = *s;
    {
        // diagnostic A/B switch for the sorting variant families: the split (three launch) form
        const char* env = getenv("BEAN_HIP_SPLIT_GUIDE");
        const char* mode = getenv("BEAN_HIP_GUIDE");
        c->fused_guide = !((env && env[0] == '1') || (mode && !strcmp(mode, "split")));
        c->wave_guide = c->fused_guide;
        c->wave2 = !(mode && !strcmp(mode, "wave1"));
        const char* smode = getenv("BEAN_HIP_SURVIVAL");
        c->surv_wave = !(smode && !strcmp(smode, "block"));
        const char* tmode = getenv("BEAN_HIP_TILING");
        c->tiling_wave = !(tmode && !strcmp(tmode, "block"));
#if BEAN_AMAX > 8
        c->tiling_wave = true;  // this build has no block form
#endif
#ifndef BEAN_AB_KERNELS
        // the product build holds the default kernels only; the superseded forms these switches select
        // live in libbean_hip_ab.so (-DBEAN_AB_KERNELS; HipSVI(..., lib_variant="ab"))
        const char* stp = getenv("BEAN_HIP_STEP");
        if (!c->fused_guide || !c->wave2 || !c->surv_wave || !c->tiling_wave ||
            (stp && (!strcmp(stp, "fused") || !strcmp(stp, "tile")))) {
            delete c;
            return fail("bean_hip_create: BEAN_HIP_GUIDE / _SURVIVAL / _TILING=block / _STEP select A/B reference kernels, "
                        "which this build does not contain (build with -DBEAN_AB_KERNELS: libbean_hip_ab.so)");
        }
#endif
    }
    {
        const char* am = getenv("BEAN_HIP_ALLELE");
        c->allele_blocks = !(am && !strcmp(am, "split"));
    }
    DevArgs& d = c->d;
    d.R = s->n_reps; d.B = s->n_condits; d.G = s->n_guides; d.T = s->n_targets;
    d.A = s->n_max_alleles; d.C = s->n_ctrl; d.E = s->n_edits;
    d.family = s->family; d.flags = s->flags; d.mask_thres = s->mask_thres;
    d.wide_targets = (!is_tiling(*s) && (s->n_targets < 64 || s->max_target_len > 256)) ? 1 : 0;
    // lanes per target of k_param's target part: 4 where a target has few rows to add (survival: ~15
    // (guide, replicate) rows; tiling: the alleles carrying an edit - unless the table is unfiltered and an
    // edit sits in dozens of them), 16 otherwise (sorting variant families: the Phi table's 2 B edges)
    d.lpt = kLanesPerTarget;
    if (is_tiling(*s)) {
        if ((int64_t)s->n_a2e_nnz <= 16 * (int64_t)s->n_targets) d.lpt = kLanesPerTargetNarrow;
    } else if (is_survival(*s)) {
        d.lpt = kLanesPerTargetNarrow;
    }
    d.g_off = s->guide_offset; d.t_off = s->target_offset;
    d.G_tot = s->n_guides_total > 0 ? s->n_guides_total : s->n_guides;
    d.sd_prior_scale = s->sd_prior_scale; d.lr0 = s->initial_lr; d.log_lrd = log(s->lrd);
    d.clip = s->clip_norm;
    d.survival = is_survival(*s) ? 1 : 0;
    d.neg_loc = s->negctrl_loc; d.neg_scale = s->negctrl_scale;

    const uint64_t G = d.G;
    const bool surv_mix = is_survival(*s) && s->family == BEAN_FAMILY_MIXTURE_NORMAL;
    const bool surv_norm = is_surv_normal(*s);
    d.surv_q0lik = surv_norm ? 1 : 0;
    d.not_loss_owner = (s->flags & BEAN_FLAG_NOT_LOSS_OWNER) ? 1 : 0;
    // guide blocks of k_param: kParamBlock guides each.  The survival families with a
    // Dirichlet-over-all-guides site have q0 blocks as well (after the alpha_pi blocks of MixtureNormal),
    // kParamBlock guides each: parameter update, gamma draws and normalisers of that site
    // (q0_draws_and_totals)
    d.q0_blocks = (surv_mix || surv_norm) ? 1 : 0;
    d.q0_blk0 = surv_mix ? (int)((G + kParamBlock - 1) / kParamBlock) : 0;
    d.n_gamma_blocks = (int)((G + kParamBlock - 1) / kParamBlock);
    const bool split_ok = !is_survival(*s) && !is_tiling(*s);
    c->wave_guide = c->wave_guide && split_ok;
    c->wave2 = c->wave2 && c->wave_guide;
    if (s->n_sample_covariates > 0 && !c->wave2) {
        delete c;
        return fail("bean_hip_create: sample covariates need the default guide kernel (k_guide_wave2)");
    }
    d.n_cov = s->n_sample_covariates;
    // k_guide_wave2's tiles follow the GLOBAL guide index (bean_guide_v2.hpp): a shard that does not start at a
    // multiple of 64 has g_sh empty lanes at the head of its first tile
    d.g_sh = c->wave2 ? s->guide_offset % 64 : 0;
    d.n_tiles = (int)((d.g_sh + G + 63) / 64);
    {
        const int seg = s->max_target_len < 1 ? 64 : (s->max_target_len > 64 ? 64 : s->max_target_len);
        d.seg_steps = 0;
        while ((1 << d.seg_steps) < seg) ++d.seg_steps;
    }
    c->surv_wave =c->surv_wave && is_survival(*s) && !is_tiling(*s);
    d.rows_v2 = (c->wave2 || c->surv_wave) ? 1 : 0;

    c->tiling_wide = is_tiling(*s) && s->n_max_alleles > kAMax;
    c->tiling_wave = c->tiling_wave && is_tiling(*s) && !c->tiling_wide;
    {
        // default: the replicates of a guide share a wave and every row is reduced there
        // (BEAN_HIP_TILING=wave: the per-replicate wave form + k_sum_trow, the A/B reference)
        const char* tmode = getenv("BEAN_HIP_TILING");
        c->tiling_rep = c->tiling_wave && s->n_reps <= kTilingRepMaxR && !(tmode && !strcmp(tmode, "wave"));
        if (c->tiling_rep) c->tiling_wave = false;
        // BEAN_HIP_TILING_W (1, 2 or 4; experiments only) overrides the number of waves per workgroup
        const int w_env = getenv("BEAN_HIP_TILING_W") ? atoi(getenv("BEAN_HIP_TILING_W")) : 0;
        long n_simd = 0;
        {
            int dev = 0, n_cu = 0;
            if (hipGetDevice(&dev) == hipSuccess &&
                hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
                n_simd = 4l * n_cu;
            else
                (void)hipGetLastError();
        }
        c->tiling_rep_w = (w_env == 1 || w_env == 2 || w_env == 4)
                              ? w_env
                              : tiling_rep_waves(s->n_reps, s->n_condits, (s->flags & BEAN_FLAG_SCALE_BY_ACC) != 0,
                                                 (long)s->n_guides, n_simd);
        if (s->n_condits > 16) c->tiling_rep_w = 1;  // LDS: (3 B + ...) x 64 W doubles per workgroup
    }
    d.wide_alleles = c->tiling_wide ? 1 : 0;
    {
        // =0: every implicit-gradient call forms its x-free factors itself, as before the table (A/B, same bits)
        const char* dt = getenv("BEAN_HIP_DIRGRAD_TAB");
        c->dirgrad_tab = !(dt && !strcmp(dt, "0"));
    }
    {
        // =0: a finisher asks for everything after its poll, as before; =2: the static inputs ahead of it, never the state
        const char* ae = getenv("BEAN_HIP_ASYNC_EARLY");
        c->async_early = (ae && !strcmp(ae, "0")) ? 0 : ((ae && !strcmp(ae, "2")) ? 2 : 1);
    }
    d.trow_summed = (c->tiling_wave || c->tiling_rep) ? 1 : 0;
    {
        const char* tc = getenv("BEAN_HIP_TOT_CONST");  // =0: the total terms are evaluated every step (A/B)
        d.tot_const = ((c->wave2 || c->surv_wave || c->tiling_wave || c->tiling_rep || c->tiling_wide) && !(tc && !strcmp(tc, "0"))) ? 1 : 0;
    }
#ifdef BEAN_AB_KERNELS
    {
        // one launch per step (bean_step_v2.hpp), opt-in (BEAN_HIP_STEP=fused; measured slower than the
        // two-launch path, see the header): the variant sorting families of k_guide_wave2 whose
        // parameters are all per target or per guide, no target longer than a tile
        const char* sm = getenv("BEAN_HIP_STEP");
        c->fused_step = c->wave2 && !d.wide_targets && s->max_target_len <= 64 && s->n_sample_covariates == 0 &&
                        (s->family == BEAN_FAMILY_MIXTURE_NORMAL || s->family == BEAN_FAMILY_NORMAL) &&
                        (sm && !strcmp(sm, "fused"));
    }
    {
        // OPT-IN (BEAN_HIP_STEP=tile): ONE launch per call, a workgroup per tile of targets
        // (bean_tile_svi.hpp).  Bit-identical to the two launches per step and measured slower (see the header).
        const char* sm = getenv("BEAN_HIP_STEP");
        const int gb = s->n_reps <= 64 ? kTileThreads / s->n_reps : 0;
        c->tile_svi = c->wave2 && !d.wide_targets && s->n_sample_covariates == 0 && !c->fused_step &&
                      (s->family == BEAN_FAMILY_MIXTURE_NORMAL || s->family == BEAN_FAMILY_NORMAL) &&
                      gb >= 1 && s->max_target_len <= gb && (sm && !strcmp(sm, "tile"));
    }
#endif
    {
        // ALL the steps of a call in one launch, no grid-wide boundary between steps (bean_async_v2.hpp): the variant
        // sorting families of k_guide_wave2 whose parameters are all per target or per guide, no target longer than a
        // tile.  BEAN_HIP_STEP=async switches it on, =pair off.
        const char* sm = getenv("BEAN_HIP_STEP");
        const long items = (long)d.n_tiles * s->n_reps;
        int dev_ = 0, n_cu_ = 256;
        if (hipGetDevice(&dev_) != hipSuccess || hipDeviceGetAttribute(&n_cu_, hipDeviceAttributeMultiprocessorCount, dev_) != hipSuccess)
            n_cu_ = 256;
        (void)hipGetLastError();
        const bool on = sm ? !strcmp(sm, "async") : async_size_in_range(items, 4l * n_cu_);
        c->async_step = on && c->wave2 && !d.wide_targets && s->max_target_len <= 64 && s->n_sample_covariates == 0 &&
                        !c->fused_step && !c->tile_svi &&
                        (s->family == BEAN_FAMILY_MIXTURE_NORMAL || s->family == BEAN_FAMILY_NORMAL) && !is_survival(*s);
    }
    // the workspace (workspace_regions).  The scalars that go with two of its regions come first: the list takes those
    // regions' sizes from them.  Arrival counters (ints, zero between launches): of the fused step kernel, per tile and
    // per tile boundary - two even halves; tiling: of k_param's allele blocks, counters and go flags, one 128-byte line
    // each (kAlleleCtrLines).  Per-wave loss parts of the wave-form guide kernels: padded tiles x replicates
    const uint64_t tiles8 = ((uint64_t)d.n_tiles + 7) / 8 * 8;
    d.n_arrival_ctr = c->wave2 ? (int)(2 * (tiles8 + 2)) : (is_tiling(*s) ? 2 * kAlleleCtrLines * 16 : 0);
    d.n_lpart = (c->wave2 || c->surv_wave) ? (int)(tiles8 * (uint64_t)d.R) : 0;
    d.tile_targets = 64;
    uint64_t n_measured = 0;
    workspace_regions(c, d, [&](auto&, uint64_t n) { n_measured += n; });
    c->workspace_bytes = n_measured * 8;
    hipError_t e = hipMalloc(&c->workspace, c->workspace_bytes);
    if (e != hipSuccess) {
        delete c;
        return fail(std::string("hipMalloc workspace: ") + hipGetErrorString(e));
    }
    e = hipMemset(c->workspace, 0, c->workspace_bytes);
    if (e != hipSuccess) {
        (void)hipFree(c->workspace);
        delete c;
        return fail(std::string("hipMemset workspace: ") + hipGetErrorString(e));
    }
    double* w = (double*)c->workspace;
    workspace_regions(c, d, [&](auto& p, uint64_t n) {
        p = (std::remove_reference_t<decltype(p)>)w;
        w += n;
    }, &c->tile_targets_dev);
    if ((uint64_t)(w - (double*)c->workspace) != n_measured) {
        const std::string msg = "bean_hip_create: the workspace regions take " + std::to_string(w - (double*)c->workspace) +
                                " doubles, " + std::to_string(n_measured) + " were measured";
        (void)hipFree(c->workspace);
        delete c;
        return fail(msg);
    }
    // the library's own exchange buffers are workspace regions (null where the shape has none)
    c->gsum_ws = d.gsum;
    c->sq_ws = d.sq;
    c->cov_sum_ws = d.cov_sum;
    *out = c;
    return 0;
}

extern "C" int bean_hip_comm_destroy(bean_hip_ctx* c);
extern "C" int bean_hip_destroy(bean_hip_ctx* c) {
    if (!c) return 0;
    drop_graph(c);
    (void)bean_hip_comm_destroy(c);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->workspace) (void)hipFree(c->workspace);
    if (c->tail_off) (void)hipFree(c->tail_off);
    if (c->tail_ws) (void)hipFree(c->tail_ws);
    if (c->tile_tab) (void)hipFree(c->tile_tab);
    if (c->live_slots) (void)hipFree(c->live_slots);
    if (c->tsum_buf) (void)hipFree(c->tsum_buf);
    if (c->tdesc_buf) (void)hipFree(c->tdesc_buf);
    if (c->step_sizes) (void)hipFree(c->step_sizes);
    if (c->dargs_dev) (void)hipFree(c->dargs_dev);
    if (c->async_ws) (void)hipFree(c->async_ws);
    if (c->loss_acc) (void)hipFree(c->loss_acc);
    if (c->member_ws) (void)hipFree(c->member_ws);
    if (c->particle_grad) (void)hipFree(c->particle_grad);
    if (c->particle_loss) (void)hipFree(c->particle_loss);
    free_args(c->members);
    free_args(c->particles);
    delete c;
    return 0;
}

extern "C" int bean_hip_bind(bean_hip_ctx* c, int slot, void* ptr, uint64_t nbytes) {
    if (!c) return fail("bean_hip_bind: null handle");
    if (slot < 0 || slot >= BEAN_BUF_COUNT) return fail("bean_hip_bind: slot out of range");
    if (ptr) {
        const uint64_t want = expected_bytes(c->shape, slot);
        if (want == 0)
            return fail("bean_hip_bind: slot " + std::to_string(slot) + " is not used by this shape");
        const uint64_t K = (uint64_t)c->n_members;
        if (slot == BEAN_BUF_LOSS_HIST) {
            if (nbytes < 8 || nbytes % 8) return fail("bean_hip_bind: loss_hist must hold >= 1 double");
            if (nbytes % (8 * K)) return fail("bean_hip_bind: loss_hist of " + std::to_string(K) + " members is (members, capacity) doubles");
            // (the accumulators of all members in one allocation, member-major like loss_hist itself)
            // (particles: the caller's loss_hist keeps its single-fit size, the library owns the particles' rows)
            const uint64_t Pn = (uint64_t)c->n_particles;
            if (nbytes / 8 / K != c->loss_capacity || !c->loss_acc) {
                if (c->loss_acc) (void)hipFree(c->loss_acc);
                c->loss_acc = nullptr;
                HIP_OK(hipMalloc((void**)&c->loss_acc, (nbytes / 8) * Pn * kLossSub * kLossWords * sizeof(long long)));
                HIP_OK(hipMemset(c->loss_acc, 0, (nbytes / 8) * Pn * kLossSub * kLossWords * sizeof(long long)));
                if (c->particle_loss) (void)hipFree(c->particle_loss);
                c->particle_loss = nullptr;
                if (c->particles_set) {
                    HIP_OK(hipMalloc((void**)&c->particle_loss, (nbytes / 8) * Pn * sizeof(double)));
                    HIP_OK(hipMemset(c->particle_loss, 0, (nbytes / 8) * Pn * sizeof(double)));
                }
            }
            c->loss_capacity = nbytes / 8 / K;
        } else if (slot >= BEAN_BUF_P_MU_LOC && slot < BEAN_BUF_V_MU_LOC + 16 && nbytes != want * K) {
            return fail("bean_hip_bind: slot " + std::to_string(slot) + " expects " + std::to_string(want * K) +
                        " bytes (" + std::to_string(K) + " member(s)), got " + std::to_string(nbytes));
        } else if (!(slot >= BEAN_BUF_P_MU_LOC && slot < BEAN_BUF_V_MU_LOC + 16) && nbytes != want) {
            return fail("bean_hip_bind: slot " + std::to_string(slot) + " expects " + std::to_string(want) +
                        " bytes, got " + std::to_string(nbytes));
        }
        c->bound_any = true;
    }
    c->slot_ptr[slot] = ptr;
    c->slot_bytes[slot] = ptr ? nbytes : 0;
    sync_devargs(c);
    drop_graph(c);
    if (slot < BEAN_BUF_P_MU_LOC && slot != BEAN_BUF_XCHG_GSUM && slot != BEAN_BUF_XCHG_TGRAD &&
        slot != BEAN_BUF_XCHG_SQ)  // (BEAN_BUF_XCHG_COV lies above the parameter slots)
        c->prepared = false;  // data changed: the data-only precomputation is stale
    return 0;
}

static int require(bean_hip_ctx* c, int slot, const char* what) {
    if (!c->slot_ptr[slot]) return fail(std::string("required buffer not bound: ") + what);
    return 0;
}

static int check_bound(bean_hip_ctx* c, bool need_grads, bool need_moments) {
    const bean_hip_shape& s = c->shape;
#define REQ(slot) if (require(c, slot, #slot)) return -1
    REQ(BEAN_BUF_X); REQ(BEAN_BUF_REPGUIDE); REQ(BEAN_BUF_SIZE_FACTOR); REQ(BEAN_BUF_SAMPLE_MASK);
    REQ(BEAN_BUF_A0); REQ(BEAN_BUF_LOSS_HIST);
    if (is_survival(s)) {
        REQ(BEAN_BUF_TIMEPOINTS);
        if (is_mixture(s)) REQ(BEAN_BUF_CONTROL_TIME);
        if (s.family == BEAN_FAMILY_MIXTURE_NORMAL) REQ(BEAN_BUF_LOG_OBS0);
    } else {
        REQ(BEAN_BUF_Z_HI); REQ(BEAN_BUF_Z_LO);
    }
    if (is_tiling(s)) {
        REQ(BEAN_BUF_A2E_PTR); REQ(BEAN_BUF_E2A_PTR); REQ(BEAN_BUF_ALLELE_MASK);
        if (s.n_a2e_nnz > 0) { REQ(BEAN_BUF_A2E_IDX); REQ(BEAN_BUF_E2A_IDX); }
    } else {
        REQ(BEAN_BUF_TARGET_OFFSETS); REQ(BEAN_BUF_GUIDE_TO_TARGET);
    }
    if (s.flags & BEAN_FLAG_USE_BCMATCH) { REQ(BEAN_BUF_X_BC); REQ(BEAN_BUF_SIZE_FACTOR_BC); REQ(BEAN_BUF_A0_BC); }
    if (is_mixture(s)) { REQ(BEAN_BUF_ALLELE_CTRL); REQ(BEAN_BUF_PI_A0); }
    if (s.flags & BEAN_FLAG_SCALE_BY_ACC) REQ(BEAN_BUF_ACCESSIBILITY);
    if (s.n_sample_covariates > 0) REQ(BEAN_BUF_REP_BY_COV);
    if (is_surv_normal(s) && s.prior_ia_total > 0.0) REQ(BEAN_BUF_PRIOR_IA);
    for (int i = 0; i < 8; ++i) {
        if (expected_bytes(s, BEAN_BUF_P_MU_LOC + i) == 0) continue;
        REQ(BEAN_BUF_P_MU_LOC + i);
        if (need_grads) REQ(BEAN_BUF_G_MU_LOC + i);
        if (need_moments) { REQ(BEAN_BUF_M_MU_LOC + i); REQ(BEAN_BUF_V_MU_LOC + i); }
    }
#undef REQ
    return 0;
}

static DevArgs member_args(const bean_hip_ctx* c, int k, uint64_t seed);
// private copies of everything a step writes: one per ensemble member or per particle (the two exclude each other)
static int n_copies(const bean_hip_ctx* c) { return c->n_members > 1 ? c->n_members : c->n_particles; }
static int alloc_workspace_copies(bean_hip_ctx* c, int n);

extern "C" int bean_hip_prepare(bean_hip_ctx* c, void* stream_) {
    if (!c) return fail("bean_hip_prepare: null handle");
    if (check_bound(c, false, false)) return -1;
    c->resume_ok = false;  // (bean_hip.h: a prepare between two windows forbids a resume, in every family)
    c->alleles_fresh = false;  // (tiling: the allele tables belong to no draw yet)
    hipStream_t stream = (hipStream_t)stream_;
    HIP_OK(hipMemsetAsync(c->d.const_acc, 0, kLossWords * sizeof(long long), stream));
    const long n = (long)c->d.R * c->d.G;
    hipLaunchKernelGGL(k_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, c->d);
    HIP_OK(hipGetLastError());
    if (c->d.kacc) {
        if (!c->d.acc) return fail("bean_hip_prepare: BEAN_FLAG_SCALE_BY_ACC needs BEAN_BUF_ACCESSIBILITY");
        hipLaunchKernelGGL(k_acc_scale, dim3((unsigned)((c->d.G + 255) / 256)), dim3(256), 0, stream, c->d.acc, c->d.G,
                           c->d.kacc);
        HIP_OK(hipGetLastError());
    }
    if (c->wave_guide) {
        // LDS sizing of k_guide_wave: a host read-back (4 bytes, setup only; the other one is the tiling work list below)
        HIP_OK(hipMemsetAsync(c->tile_targets_dev, 0, 2 * sizeof(int), stream));
        const int tiles = c->wave2 ? c->d.n_tiles : (c->d.G + 63) / 64;
        hipLaunchKernelGGL(k_tile_targets, dim3((tiles + 255) / 256), dim3(256), 0, stream, c->d.g2t, c->d.G,
                           c->d.g_sh, c->tile_targets_dev);
        HIP_OK(hipGetLastError());
        // the shape's max_target_len decides the kernels' layouts (scan steps, two slots per target): checked
        hipLaunchKernelGGL(k_max_target_len, dim3((c->d.T + 255) / 256), dim3(256), 0, stream, c->d.toff, c->d.T,
                           c->tile_targets_dev + 1);
        HIP_OK(hipGetLastError());
        int ntl[2] = {0, 0};
        HIP_OK(hipMemcpyAsync(ntl, c->tile_targets_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        const int nt = ntl[0];
        if (nt < 1 || nt > 64) return fail("bean_hip_prepare: guides are not sorted by target (BEAN_BUF_GUIDE_TO_TARGET)");
        if (ntl[1] > c->shape.max_target_len)
            return fail("bean_hip_prepare: bean_hip_shape.max_target_len = " + std::to_string(c->shape.max_target_len) +
                        " but BEAN_BUF_TARGET_OFFSETS holds a target of " + std::to_string(ntl[1]) + " guides");
        if (nt != c->d.tile_targets) drop_graph(c);
        c->d.tile_targets = nt;
        if (c->wave2) {
            // per-target-part sums of d/dmu_t, d/dy_t (k_guide_wave2 -> k_param) and where each target's lie
            // no target longer than a tile (thin mode): two fixed slots per target, no descriptor to read
            c->d.tsum_direct = (!c->d.wide_targets && c->shape.max_target_len >= 1 && c->shape.max_target_len <= 64) ? 1 : 0;
            const size_t n_sum1 = c->d.tsum_direct ? (size_t)2 * c->d.R * 2 * c->d.T : (size_t)2 * c->d.R * c->d.n_tiles * nt;
            c->tsum_stride = n_sum1;
            const size_t n_sum = n_sum1 * (size_t)n_copies(c);  // (an ensemble: one part per member; particles alike)
            if (c->tsum_buf) (void)hipFree(c->tsum_buf);
            c->tsum_buf = nullptr;
            HIP_OK(hipMalloc((void**)&c->tsum_buf, n_sum * sizeof(double)));
            HIP_OK(hipMemsetAsync(c->tsum_buf, 0, n_sum * sizeof(double), stream));
            if (!c->tdesc_buf) HIP_OK(hipMalloc((void**)&c->tdesc_buf, (size_t)c->d.T * sizeof(int2)));
            c->d.tsum = c->tsum_buf;
            c->d.tdesc = c->tdesc_buf;
            hipLaunchKernelGGL(k_tdesc, dim3((c->d.T + 255) / 256), dim3(256), 0, stream, c->d, c->tdesc_buf);
            HIP_OK(hipGetLastError());
            drop_graph(c);
        }
    }
    if (c->d.family == kMultiMixture) {
        // k_allele's work list: the allele slots that hold an allele, in (a1, g) order.  Setup only: the mask
        // and the CSR row pointers come to the host once (G A bytes + (G (A - 1) + 1) ints).
        const DevArgs& d = c->d;
        const long G = d.G, A = d.A, A1 = d.A - 1;
        std::vector<uint8_t> mask((size_t)(G * A));
        std::vector<int> ptr((size_t)(G * A1 + 1));
        HIP_OK(hipMemcpyAsync(mask.data(), d.amask, mask.size(), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipMemcpyAsync(ptr.data(), d.a2e_ptr, ptr.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        std::vector<int> live;
        live.reserve((size_t)(G * A1));
        // in the order the tables are laid out (tab_off): guide-contiguous for the register-resident kernels,
        // allele-contiguous for the allele-parallel ones - consecutive k_allele threads store next to each other
        auto consider = [&](long a1, long g) {
            const long slot = g * A1 + a1;
            if (mask[(size_t)(g * A + a1 + 1)] != 0 || ptr[(size_t)slot + 1] > ptr[(size_t)slot]) live.push_back((int)(a1 * G + g));
        };
        if (d.wide_alleles) {
            for (long g = 0; g < G; ++g)
                for (long a1 = 0; a1 < A1; ++a1) consider(a1, g);
        } else {
            for (long a1 = 0; a1 < A1; ++a1)
                for (long g = 0; g < G; ++g) consider(a1, g);
        }
        if (!c->live_slots) HIP_OK(hipMalloc(&c->live_slots, (size_t)(G * A1) * sizeof(int)));
        if (!live.empty())
            HIP_OK(hipMemcpyAsync(c->live_slots, live.data(), live.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));  // `live` goes out of scope
        // the slots left out hold what k_allele would write there: zeros
        {
            const long n_tab = (long)d.B * A1 * G;
            HIP_OK(hipMemsetAsync((void*)d.tabP, 0, (size_t)n_tab * sizeof(double), stream));
            HIP_OK(hipMemsetAsync((void*)d.tabPmu, 0, (size_t)n_tab * sizeof(double), stream));
            HIP_OK(hipMemsetAsync((void*)d.tabPy, 0, (size_t)n_tab * sizeof(double), stream));
            HIP_OK(hipMemsetAsync((void*)d.mu_a, 0, (size_t)(A1 * G) * sizeof(double), stream));
            if (d.sig_a) HIP_OK(hipMemsetAsync((void*)d.sig_a, 0, (size_t)(A1 * G) * sizeof(double), stream));
            drop_graph(c);
        }
        c->d.live_slots = c->live_slots;
        c->d.n_live_slots = (int)live.size();
    }
    {
        // more than 64 KB of dynamic LDS per workgroup (many conditions): the kernel has to be told
        const DevArgs& d = c->d;
        const bool acc = (d.flags & kAcc) != 0;
        size_t lds = 0;
        const void* fn = nullptr;
        if (c->wave_guide && c->wave2) {
            lds = guide_wave2_lds(d.B, d.tile_targets);
            fn = with_family_acc(d, [](auto fam, auto ac) { return (const void*)k_guide_wave2<fam(), ac()>; });
        } else if (c->tiling_rep || c->tiling_wave) {
            const size_t nt = c->tiling_rep ? 64u * c->tiling_rep_w : 64u;
            lds = guide_tiling_lds(d.B, acc, nt, !c->tiling_rep);
            if (c->tiling_rep)
                fn = with_acc_surv(d, [](auto ac, auto surv) { return (const void*)k_guide_tiling_rep<ac(), surv()>; });
            else
                fn = with_acc_surv(d, [](auto ac, auto surv) { return (const void*)k_guide_tiling_wave<ac(), surv()>; });
        }
        if (lds > kLdsPerWorkgroupMax)
            return fail("bean_hip_prepare: " + std::to_string(d.B) + " conditions x " + std::to_string(d.tile_targets) +
                        " targets per 64-guide tile need " + std::to_string(lds) + " bytes of LDS per workgroup; a compute unit has " +
                        std::to_string(kLdsPerWorkgroupMax));
        if (fn && lds > 65536) HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
#ifdef BEAN_AB_KERNELS
    c->tile_ready = false;
    if (c->tile_svi) {
        // tiles of whole targets with at most kTileThreads / R guides: built on the host from the target
        // offsets (4 (T + 1) bytes read back once, next to the 4 bytes above)
        const int T = c->d.T, G = c->d.G, gb = kTileThreads / c->d.R;
        std::vector<int> toff((size_t)T + 1);
        HIP_OK(hipMemcpyAsync(toff.data(), c->d.toff, sizeof(int) * ((size_t)T + 1), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        std::vector<int> tg0, tt0;
        int ntm = 1, gbm = 1;
        bool ok = toff[0] == 0 && toff[T] == G;
        for (int t = 0; ok && t < T;) {
            int t1 = t, g0 = toff[t];
            while (t1 < T && toff[t1 + 1] - g0 <= gb && toff[t1 + 1] > toff[t1]) ++t1;
            if (t1 == t) {  // an empty target or one longer than a tile: the two-launch path handles it
                ok = false;
                break;
            }
            tg0.push_back(g0);
            tt0.push_back(t);
            if (t1 - t > ntm) ntm = t1 - t;
            if (toff[t1] - g0 > gbm) gbm = toff[t1] - g0;
            t = t1;
        }
        if (ok && !tg0.empty()) {
            tg0.push_back(G);
            tt0.push_back(T);
            const size_t n1 = tg0.size();
            if (c->tile_tab) (void)hipFree(c->tile_tab);
            c->tile_tab = nullptr;
            HIP_OK(hipMalloc((void**)&c->tile_tab, 2 * n1 * sizeof(int)));
            HIP_OK(hipMemcpyAsync(c->tile_tab, tg0.data(), n1 * sizeof(int), hipMemcpyHostToDevice, stream));
            HIP_OK(hipMemcpyAsync(c->tile_tab + n1, tt0.data(), n1 * sizeof(int), hipMemcpyHostToDevice, stream));
            HIP_OK(hipStreamSynchronize(stream));
            c->n_tiles = (int)n1 - 1;
            c->tile_ntm = ntm;
            c->tile_gbm = gbm;
            c->tile_blocks = 0;
            c->tile_ready = true;
        }
    }
#endif
    if (n_copies(c) > 1 || c->particles_set) {
        // every member's (particle's) private workspace starts as a copy of the one just prepared: the data-only parts
        // (the constant, the bin edges, the accessibility factors, the kPNrg row) are then there for all of them
        for (int k = 1; k < n_copies(c); ++k)
            HIP_OK(hipMemcpyAsync(c->member_ws + (size_t)(k - 1) * c->member_ws_stride, c->workspace, c->workspace_bytes,
                                  hipMemcpyDeviceToDevice, stream));
        // (survival members: the single-fit launch raises no dynamic LDS limit, so k_guide_survival_wave_ens gets none
        // either - bean_hip_survival_members_supported refuses the numbers of timepoints that would need one)
        if (!c->d.survival) {
            const size_t lds = guide_wave2_lds(c->d.B, c->d.tile_targets);
            const void* fn = with_family_acc(c->d, [](auto fam, auto ac) { return (const void*)k_guide_wave2_ens<fam(), ac()>; });
            if (lds > 65536) HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        HIP_OK(hipStreamSynchronize(stream));
        drop_graph(c);
    }
    if (c->member_rg || c->member_x) {
        // per-member masks or counts: the constant, the kPNrg row and nobs depend on `rg` and on the counts (the constant
        // holds their log-factorials), so k_prepare's body runs again, once per member, on the member's masks and counts
        // and into its own workspace copy (member 0's is the workspace itself)
        // (the array is uploaded with the seeds known so far - zeros before the first run - and is then current: a
        // bean_hip_svi_run_ensemble with those seeds does not upload it again)
        const int K = c->n_members;
        std::vector<uint64_t> seeds = c->members.seeds;
        if ((int)seeds.size() != K) seeds.assign((size_t)K, 0);
        c->members.dirty = true;  // (this prepare has changed what member_args reads: tsum, tile_targets)
        if (refresh_args(c->members, K, seeds.data(), stream, [&](int k, uint64_t seed) { return member_args(c, k, seed); }))
            return -1;
        for (int k = 0; k < K; ++k)
            HIP_OK(hipMemsetAsync(c->members.host[(size_t)k].const_acc, 0, kLossWords * sizeof(long long), stream));
        hipLaunchKernelGGL(k_prepare_ens, dim3((unsigned)((n + 255) / 256), (unsigned)K), dim3(256), 0, stream,
                           (const DevArgs*)c->members.dev);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(stream));
    }
    c->prepared = true;
    return 0;
}

// ------------------------------------------------------------------ launches
// a profile run that times the guide kernel (mode 1; mode 2 times k_param instead), up to 4096 timed launches
static bool prof_guide(const bean_hip_ctx* c) { return c->profile && !c->profile_param && c->ev.size() < 8192; }

// One kernel launch.  prof: between two events that carry the kernel's own begin / end timestamps
// (hipExtLaunchKernelGGL), i.e. the duration rocprofv3 --kernel-trace reports, without the dispatch gap; the pair goes
// to c->ev.  (A launch that covers several SVI steps adds their number to c->ev_steps itself.)
template <typename... KArgs, typename... Args>
static void launch_timed(bean_hip_ctx* c, bool prof, void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds,
                         hipStream_t stream, Args&&... args) {
    if (!prof) {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<KArgs>(args)...);
        return;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, e0, e1, 0, static_cast<KArgs>(args)...);
    c->ev.push_back(e0);
    c->ev.push_back(e1);
}

// The forms that take several launches (the block forms, the split form's k_lik) and k_guide_tiling_wide are timed from
// the stream instead: what lies between the two records.  span_begin says whether the run is timed.
static bool span_begin(bean_hip_ctx* c, hipStream_t stream) {
    if (!prof_guide(c)) return false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, stream);
    c->ev.push_back(e0);
    c->ev.push_back(e1);
    return true;
}
static void span_end(bean_hip_ctx* c, hipStream_t stream) { (void)hipEventRecord(c->ev.back(), stream); }

static void grid_param(const bean_hip_ctx* c, int& n_target_blocks, int& n_blocks) {
    const DevArgs& d = c->d;
    n_target_blocks = d.wide_targets ? d.T : (int)(((long)d.T * d.lpt + kParamBlock - 1) / kParamBlock);
    int guide_blocks = 0;
    if (d.family == kMultiMixture)  // kAMax lanes per guide, or one wave per guide on the wide path
        guide_blocks = (int)(((long)d.G * (d.wide_alleles ? 64 : kAMax) + kParamBlock - 1) / kParamBlock);
    else if (d.surv_q0lik) guide_blocks = d.n_gamma_blocks;
    else if (d.family == kMixture)  // the alpha_pi blocks + (survival) the q0 blocks
        guide_blocks = (d.G + kParamBlock - 1) / kParamBlock + (d.q0_blocks ? d.n_gamma_blocks : 0);
    n_blocks = n_target_blocks + guide_blocks;
}

// Allele blocks of a PREP launch of k_param on DevArgs d (tgrad as launched): its specialised tiling build (KIND 3), a
// sorting screen, not switched off (BEAN_HIP_ALLELE=split; BEAN_HIP_PARAM_KIND=0 forces the generic kernel, which has none).
static bool param_generic_only() {
    static const bool g = getenv("BEAN_HIP_PARAM_KIND") && !strcmp(getenv("BEAN_HIP_PARAM_KIND"), "0");
    return g;
}
static bool param_kind3(const DevArgs& d) {
    return d.family == kMultiMixture && !d.wide_targets && !d.wide_alleles && !d.n_cov && !d.lpart &&
           d.trow_summed && !d.surv_q0lik && d.lpt == kLanesPerTargetNarrow;
}
static int param_allele_blocks(const bean_hip_ctx* c, const DevArgs& d) {
    if (param_generic_only() || !param_kind3(d) || d.survival || !c->allele_blocks || d.n_live_slots <= 0 || !d.tile_ctr) return 0;
    if (d.T <= 0) return 0;  // (no edit block would ever raise the go flags)
    return (int)(((long)d.n_live_slots + kParamBlock - 1) / kParamBlock);
}
// what a PREP launch leaves (with or without exchanged gradients: the same build of the kernel, the same answer)
static bool param_prep_leaves_alleles_fresh(const bean_hip_ctx* c) {
    return param_allele_blocks(c, c->d) > 0;
}

template <bool FINISH, bool ADAM, bool PREP>
static void launch_param(bean_hip_ctx* c, hipStream_t stream, const double* tgrad = nullptr, bool cov_exchanged = false) {
    int ntb, nb;
    grid_param(c, ntb, nb);
    DevArgs d = c->d;
    d.tgrad = tgrad;
    if (d.n_cov) {  // sample covariates: their own small step runs first (it owns the replicates' shifts)
        // (guide-sharded: the sums were formed by bean_hip_sharded_guide and all-reduced by the caller)
        if (FINISH && !cov_exchanged) hipLaunchKernelGGL(k_cov_sum, dim3(d.R), dim3(1024), 0, stream, d);
        hipLaunchKernelGGL((k_cov_step<FINISH, ADAM, PREP>), dim3(1), dim3(64), 0, stream, d);
    }
    // the specialised build of the kernel (k_param<..., 1>) where its launch conditions hold
    const bool kind1 = !d.survival && d.family != kMultiMixture && !d.wide_targets && !d.tgrad && !d.n_cov && d.wrow &&
                       d.rows_v2 && !d.rrow && !d.surv_q0lik && !d.not_loss_owner && d.lpart &&
                       (d.dgq || d.family != kMixture) && d.tsum;
    const bool kind2 = d.survival && d.family == kMixture && !d.surv_q0lik && d.dgq && !d.tsum && !d.wide_targets && !d.tgrad &&
                       !d.n_cov && d.wrow && d.rows_v2 && !d.rrow && d.lpart && d.lpt == kLanesPerTargetNarrow;
    const bool kind3 = param_kind3(d);
    // BEAN_HIP_PARAM_KIND=0 forces the generic build (the test that the specialised builds change nothing)
    const bool generic_only = param_generic_only();
    const int kind = generic_only ? 0 : (kind1 ? 1 : (kind2 ? 2 : (kind3 ? 3 : 0)));
    const bool prof = c->profile && c->profile_param && FINISH && PREP && c->ev.size() < 8192;
    // allele blocks (k_param<..., 3>, sorting): k_allele's work as the tail of this grid
    const int nab = (PREP && kind == 3) ? param_allele_blocks(c, d) : 0;
    if (PREP) c->alleles_fresh = nab > 0;
    if (nab > 0) {
        // Dispatch order: edit blocks, `ahead` guide blocks, the allele blocks, the other guide blocks (DevArgs::q0_blk0,
        // which the sorting tiling family does not use otherwise).  Measured at BASELINE config 3 (1 792 places for 469 +
        // 1 563 + 753 blocks; us per step): the allele blocks last 146.5; behind the guide blocks that fill the first
        // resident round (1 323) 148.0 (they poll on places the other guide blocks wait for); behind 531 of them 152.2;
        // k_allele as a launch of its own 148.9.  BEAN_HIP_ALLELE_AHEAD: experiments.
        static const int ahead_env = getenv("BEAN_HIP_ALLELE_AHEAD") ? atoi(getenv("BEAN_HIP_ALLELE_AHEAD")) : -1;
        const int ngb = nb - ntb;
        d.q0_blk0 = ahead_env >= 0 && ahead_env < ngb ? ahead_env : ngb;
    }
    const dim3 grid(nb + nab), block(kParamBlock);
    auto go = [&](auto knd) { launch_timed(c, prof, k_param<FINISH, ADAM, PREP, knd()>, grid, block, 0, stream, d, ntb); };
    switch (kind) {
        case 1: go(std::integral_constant<int, 1>{}); break;
        case 2: go(std::integral_constant<int, 2>{}); break;
        case 3: go(std::integral_constant<int, 3>{}); break;
        default: go(std::integral_constant<int, 0>{}); break;
    }
}

#ifdef BEAN_AB_KERNELS  // block forms and the split form: A/B references
template <int B>
static void launch_guide_b(bean_hip_ctx* c, hipStream_t stream, dim3 grid, dim3 block, size_t lds) {
    const DevArgs& d = c->d;
    if (d.survival && d.family != kMultiMixture) {
        with_family_acc(d, [&](auto fam, auto acc) {
            hipLaunchKernelGGL((k_guide_survival<B, fam(), acc()>), grid, block, lds, stream, d);
        });
    } else if (d.family == kMultiMixture) {
#if BEAN_AMAX <= 8
        const size_t tl = ((size_t)kTNumPart * 64 + 16) * sizeof(double);
        with_acc_surv(d, [&](auto acc, auto surv) {
            hipLaunchKernelGGL((k_guide_tiling<B, acc(), surv()>), grid, block, tl, stream, d);
        });
#endif
    }
}

static int waves_per_block(const bean_hip_ctx* c) { return c->d.R < 8 ? c->d.R : 8; }

static void launch_lik(bean_hip_ctx* c, hipStream_t stream, dim3 grid, dim3 block, size_t lds) {
    const DevArgs& d = c->d;
    with_family_acc(d, [&](auto fam, auto acc) {
        hipLaunchKernelGGL((k_lik<fam() == kMixture, acc()>), grid, block, lds, stream, d);
    });
}

// sorting variant families as three launches (see bean_kernels.hpp, "split form")
static void launch_guide_split(bean_hip_ctx* c, hipStream_t stream) {
    const DevArgs& d = c->d;
    const bool mix = d.family == kMixture;
    const int nlik = (d.flags & kUseBc) ? 2 : 1;
    const int rep_waves = d.R < 8 ? d.R : 8;
    const dim3 grid((d.G + 63) / 64);
    if (mix) {
        const long n = (long)d.R * d.G;
        hipLaunchKernelGGL(k_sample_pi, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d);
    }
    const bool prof = span_begin(c, stream);
    launch_lik(c, stream, dim3((d.G + 63) / 64, d.R), dim3(64 * nlik), 0);
    if (prof) span_end(c, stream);
    if (mix) {
        const size_t l3 = ((size_t)rep_waves * 7 * 64 + 16) * sizeof(double);
        hipLaunchKernelGGL(k_pi_terms, grid, dim3(64 * rep_waves), l3, stream, d);
    }
}

#endif  // BEAN_AB_KERNELS

// sorting variant families, one wave per (guide tile, replicate), second form (bean_guide_v2.hpp)
static void launch_guide_wave2(bean_hip_ctx* c, hipStream_t stream) {
    const DevArgs& d = c->d;
    const int tiles = d.n_tiles;
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8) * (unsigned)d.R), block(64);
    // BEAN_HIP_LDS_PAD (bytes; experiments only): a larger LDS request lowers the number of resident waves
    static const size_t lds_pad = getenv("BEAN_HIP_LDS_PAD") ? (size_t)atol(getenv("BEAN_HIP_LDS_PAD")) : 0;
    const size_t lds = guide_wave2_lds(d.B, d.tile_targets) + lds_pad;
    with_family_acc(d, [&](auto fam, auto acc) {
        launch_timed(c, prof_guide(c), k_guide_wave2<fam(), acc()>, grid, block, lds, stream, d);
    });
}

#ifdef BEAN_AB_KERNELS
// sorting variant families, one wave per (guide tile, replicate)
static void launch_guide_wave(bean_hip_ctx* c, hipStream_t stream) {
    const DevArgs& d = c->d;
    const dim3 grid((d.G + 63) / 64, d.R), block(64);
    const size_t lds = ((size_t)3 * d.B * d.tile_targets + (size_t)kWaveMisc * 64) * sizeof(double) +
                       (size_t)2 * d.B * 64 * sizeof(float);
    with_family_acc(d, [&](auto fam, auto acc) {
        launch_timed(c, prof_guide(c), k_guide_wave<fam(), acc()>, grid, block, lds, stream, d);
    });
}

#endif  // BEAN_AB_KERNELS

// tiling families, one wave per (guide tile, replicate), then the sum over replicates
static void launch_guide_tiling_wave(bean_hip_ctx* c, hipStream_t stream) {
    const DevArgs& d = c->d;
    const bool acc = (d.flags & kAcc) != 0;
    const dim3 grid((unsigned)(((d.G + 63) / 64 + 7) / 8 * 8) * (unsigned)d.R), block(64);
    const size_t lds = guide_tiling_lds(d.B, acc, 64, true);
    with_acc_surv(d, [&](auto ac, auto surv) {
        launch_timed(c, prof_guide(c), k_guide_tiling_wave<ac(), surv()>, grid, block, lds, stream, d);
    });
    hipLaunchKernelGGL(k_sum_trow, dim3((d.G + 255) / 256, kTNumPart), dim3(256), 0, stream, d);
}

// tiling families, the replicates of a guide in one wave (bean_tiling_v2.hpp): rows go straight to `part`
static void launch_guide_tiling_rep(bean_hip_ctx* c, hipStream_t stream) {
    const DevArgs& d = c->d;
    const bool acc = (d.flags & kAcc) != 0;
    const int waves = c->tiling_rep_w;
    const int nt = 64 * waves;
    int gw = nt / d.R;  // guides per workgroup (R <= kTilingRepMaxR = 64, so >= 1)
    unsigned n_wg = (unsigned)((d.G + gw - 1) / gw);
    // which guides a workgroup takes: tiling_rep_slice, mode 1 (an XCD's workgroups take contiguous runs of the guide order,
    // one run per quarter of it; BEAN_HIP_TILING_MAP=0: workgroup b takes slice b).  Config 3, same bits: kernel 115.2 ->
    // 113.1 us, step 145.5 -> 144.8.  The grid is padded to a multiple of 32, the mode rides above the argument's low byte.
    static const int map_mode = getenv("BEAN_HIP_TILING_MAP") ? atoi(getenv("BEAN_HIP_TILING_MAP")) : 1;
    if (map_mode) {
        n_wg = (n_wg + 31) / 32 * 32;
        gw |= map_mode << 8;
    }
    // issue priority by progress (k_guide_tiling_rep's phase_prio): bit 16
    static const int prio_mode = getenv("BEAN_HIP_TILING_PRIO") ? atoi(getenv("BEAN_HIP_TILING_PRIO")) : 1;
    if (prio_mode) gw |= 1 << 16;
    const dim3 grid(n_wg), block(nt);
    const size_t lds = guide_tiling_lds(d.B, acc, (size_t)nt, false);
    with_acc_surv(d, [&](auto ac, auto surv) {
        launch_timed(c, prof_guide(c), k_guide_tiling_rep<ac(), surv()>, grid, block, lds, stream, d, gw);
    });
}

#ifdef BEAN_AB_KERNELS
// One SVI step in one launch (bean_step_v2.hpp); `flip` alternates the step-counter buffers.
static void launch_step_wave2(bean_hip_ctx* c, hipStream_t stream, int flip) {
    const DevArgs& d = c->d;
    const int tiles = d.n_tiles;
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8) * (unsigned)d.R), block(64);
    const size_t lds = guide_wave2_lds(d.B, d.tile_targets);
    with_family_acc(d, [&](auto fam, auto acc) {
        launch_timed(c, prof_guide(c), k_step_wave2<fam(), acc()>, grid, block, lds, stream, d, flip);
    });
}

#endif  // BEAN_AB_KERNELS

// survival variant families, one wave per (guide tile, replicate) (bean_survival_v2.hpp)
static void launch_guide_survival_wave(bean_hip_ctx* c, hipStream_t stream) {
    const DevArgs& d = c->d;
    const int tiles = (d.G + 63) / 64;
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8) * (unsigned)d.R), block(64);
    const size_t lds = guide_survival_wave_lds(d.B);
    with_family_acc(d, [&](auto fam, auto acc) {
        launch_timed(c, prof_guide(c), k_guide_survival_wave<fam(), acc()>, grid, block, lds, stream, d);
    });
    if (d.surv_q0lik)  // projection term of the G-dimensional Dirichlet's pathwise gradient
        hipLaunchKernelGGL(k_sum_q, dim3(d.R), dim3(1024), 0, stream, d);
}

static void launch_guide(bean_hip_ctx* c, hipStream_t stream) {
    const DevArgs& d = c->d;
#ifdef BEAN_AB_KERNELS
    if (!c->fused_guide && !d.survival && d.family != kMultiMixture) {
        launch_guide_split(c, stream);
        return;
    }
#endif
    if (c->wave_guide) {
#ifdef BEAN_AB_KERNELS
        if (!c->wave2) {
            launch_guide_wave(c, stream);
            return;
        }
#endif
        launch_guide_wave2(c, stream);
        return;
    }
    if (c->surv_wave) {
        launch_guide_survival_wave(c, stream);
        return;
    }
    if (d.family == kMultiMixture) {  // allele-level tables of this step's draw, unless k_param's allele blocks left them
        const long n = d.n_live_slots;
        if (n > 0 && !c->alleles_fresh) hipLaunchKernelGGL(k_allele, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d);
        c->alleles_fresh = true;
    }
    if (c->tiling_rep) {
        launch_guide_tiling_rep(c, stream);
        return;
    }
    if (c->tiling_wave) {
        launch_guide_tiling_wave(c, stream);
        return;
    }
    if (c->tiling_wide) {
        const dim3 gridw((unsigned)(((long)d.G + 7) / 8 * 8 * d.R)), blockw(64);
        const bool prof = span_begin(c, stream);
        with_acc_surv(d, [&](auto acc, auto surv) {
            hipLaunchKernelGGL((k_guide_tiling_wide<acc(), surv()>), gridw, blockw, 0, stream, d);
        });
        if (prof) span_end(c, stream);
        return;
    }
#ifdef BEAN_AB_KERNELS  // block forms
    const int nw = waves_per_block(c);
    const dim3 grid((d.G + 63) / 64), block(64 * nw);
    const size_t lds = ((size_t)nw * kNumPart * 64 + 16) * sizeof(double);
    const bool prof = span_begin(c, stream);
    switch (d.B) {
        case 1: launch_guide_b<1>(c, stream, grid, block, lds); break;
        case 2: launch_guide_b<2>(c, stream, grid, block, lds); break;
        case 3: launch_guide_b<3>(c, stream, grid, block, lds); break;
        case 4: launch_guide_b<4>(c, stream, grid, block, lds); break;
        case 5: launch_guide_b<5>(c, stream, grid, block, lds); break;
        case 6: launch_guide_b<6>(c, stream, grid, block, lds); break;
        case 7: launch_guide_b<7>(c, stream, grid, block, lds); break;
#if BEAN_BMAX <= 8
        default: launch_guide_b<8>(c, stream, grid, block, lds); break;
#else
        case 8: launch_guide_b<8>(c, stream, grid, block, lds); break;
        case 9: launch_guide_b<9>(c, stream, grid, block, lds); break;
        case 10: launch_guide_b<10>(c, stream, grid, block, lds); break;
        case 11: launch_guide_b<11>(c, stream, grid, block, lds); break;
        case 12: launch_guide_b<12>(c, stream, grid, block, lds); break;
        case 13: launch_guide_b<13>(c, stream, grid, block, lds); break;
        case 14: launch_guide_b<14>(c, stream, grid, block, lds); break;
        case 15: launch_guide_b<15>(c, stream, grid, block, lds); break;
        default: launch_guide_b<16>(c, stream, grid, block, lds); break;
#endif
    }
    if (d.surv_q0lik)  // projection term of the G-dimensional Dirichlet's pathwise gradient
        hipLaunchKernelGGL(k_sum_q, dim3(d.R), dim3(1024), 0, stream, d);
    if (prof) span_end(c, stream);
#endif
}

static void launch_finalize(bean_hip_ctx* c, hipStream_t stream, uint64_t first, uint64_t n, bool cur) {
    const unsigned blocks = (unsigned)((n + 3) / 4);  // one wave per slot
    hipLaunchKernelGGL(k_loss_finalize, dim3(blocks), dim3(n == 1 ? 64 : 256), 0, stream, c->d, (unsigned long long)first,
                       (unsigned long long)n, cur ? 1 : 0);
}

// step counters to (step, slot) and the loss accumulators of n slots from `slot` to zero
static void launch_set_step(bean_hip_ctx* c, hipStream_t stream, uint64_t step, uint64_t slot, uint64_t n) {
    const uint64_t words = n * kLossSub * kLossWords;
    unsigned blocks = (unsigned)((words + 255) / 256);
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_set_step, dim3(blocks), dim3(256), 0, stream, c->d, (unsigned long long)step,
                       (unsigned long long)slot, (unsigned long long)n);
}

extern "C" int bean_hip_elbo_grad(bean_hip_ctx* c, uint64_t seed, uint64_t step, uint64_t loss_index,
                                  void* stream_) {
    if (!c) return fail("bean_hip_elbo_grad: null handle");
    if (!c->prepared) return fail("bean_hip_elbo_grad: call bean_hip_prepare first");
    if (check_bound(c, true, false)) return -1;
    if (loss_index >= c->loss_capacity) return fail("bean_hip_elbo_grad: loss_index beyond loss_hist");
    hipStream_t stream = (hipStream_t)stream_;
    c->d.seed = seed;
    c->resume_ok = false;
    launch_set_step(c, stream, step, loss_index, 1);
    launch_param<false, false, true>(c, stream);
    launch_guide(c, stream);
    launch_param<true, false, false>(c, stream);
    launch_finalize(c, stream, loss_index, 1, false);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bean_hip_adam(bean_hip_ctx* c, uint64_t t, void* stream_) {
    if (!c) return fail("bean_hip_adam: null handle");
    if (check_bound(c, true, true)) return -1;
    if (t < 1) return fail("bean_hip_adam: t is 1-based");
    c->resume_ok = false;
    hipStream_t stream = (hipStream_t)stream_;
    for (int i = 0; i < 8; ++i) {
        const uint64_t bytes = expected_bytes(c->shape, BEAN_BUF_P_MU_LOC + i);
        if (!bytes) continue;
        const long n = (long)(bytes / 4);
        hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, c->d.p[i],
                           (const float*)c->d.g[i], c->d.m[i], c->d.v[i], n, c->d, (unsigned long long)t);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ stepping entry points
// ---- what they share
// The checks every stepping entry point opens with; `who` prefixes the messages.  Returns 1 to go on; otherwise the
// entry point's own return value: -1 (failed, bean_hip_last_error says why) or 0 (no steps asked for).
static int begin_steps(bean_hip_ctx* c, const char* who, uint64_t first_step, uint64_t n_steps) {
    if (!c) return fail(std::string(who) + ": null handle");
    if (!c->prepared) return fail(std::string(who) + ": call bean_hip_prepare first");
    if (check_bound(c, false, true)) return -1;
    if (n_steps == 0) return 0;
    if (first_step + n_steps > c->loss_capacity)
        return fail(std::string(who) + ": loss_hist too small for first_step + n_steps");
    return 1;
}

// the loss window of the call's n_steps steps to zero, then the draw and tables of its first step
static void first_draw(bean_hip_ctx* c, hipStream_t stream, uint64_t first_step, uint64_t n_steps) {
    launch_set_step(c, stream, first_step, first_step, n_steps);
    launch_param<false, false, true>(c, stream);
}

// the call's last launch has drawn step `next` and filled its tables: a bean_hip_svi_resume of that step, with the same
// seed on the same stream, goes on from there
static void mark_resumable(bean_hip_ctx* c, uint64_t seed, uint64_t next, void* stream) {
    c->resume_ok = true;
    c->resume_next = next;
    c->resume_seed = seed;
    c->resume_stream = stream;
}

// Noise injected or dumped at every step: the eps / pi buffers every stepping path asks about.  The sites add what
// else they look at (pi_out, x0_*, eps_u_*, kDumpPi): those sets differ from site to site, which is inherited and not
// reviewed here.
static bool per_step_noise(const DevArgs& d) {
    return d.eps_mu_in || d.eps_sd_in || d.pi_in || d.eps_noise_in || d.eps_mu_out || d.eps_sd_out || d.eps_noise_out;
}
static bool dumps_pi(const DevArgs& d) { return (d.flags & kDumpPi) != 0; }

static void enqueue_pairs(bean_hip_ctx* c, hipStream_t stream, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        launch_param<true, true, true>(c, stream);
        launch_guide(c, stream);
    }
}

// n launches of k_step_wave2 (A/B build), the step-counter buffers alternating from flip0
static void enqueue_fused(bean_hip_ctx* c, hipStream_t stream, uint64_t n, int flip0 = 0) {
#ifdef BEAN_AB_KERNELS
    for (uint64_t i = 0; i < n; ++i) launch_step_wave2(c, stream, (int)((i + flip0) & 1));
#else
    (void)c; (void)stream; (void)n; (void)flip0;
#endif
}

// Capture what enqueue() launches on `stream` into an executable graph; enqueue returns 0 or, having called fail, -1.
// A capture runs nothing, so the allele-table state is saved, set to what a replay will find at the graph's head
// (head_fresh; graphs that begin with a PREP launch of k_param do not care) and restored.  Whatever fails, the stream
// is taken out of capture mode and a partial graph destroyed before returning.
template <typename Enqueue>
static int capture_graph(bean_hip_ctx* c, hipStream_t stream, bool head_fresh, Enqueue&& enqueue, hipGraphExec_t* out) {
    *out = nullptr;
    hipGraph_t graph = nullptr;
    HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const bool fresh_was = c->alleles_fresh;
    c->alleles_fresh = head_fresh;
    const int rc = enqueue();
    c->alleles_fresh = fresh_was;
    hipError_t e = hipStreamEndCapture(stream, &graph);
    if (e != hipSuccess) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
            hipGraph_t junk = nullptr;
            (void)hipStreamEndCapture(stream, &junk);
            if (junk) (void)hipGraphDestroy(junk);
        }
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    }
    int ret = rc;  // (a failed enqueue has said why)
    if (rc == 0 && (e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0)) != hipSuccess) {
        *out = nullptr;
        ret = fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    }
    if (graph) (void)hipGraphDestroy(graph);
    return ret;
}

// A ladder of graphs: rung k replays (base << k) units of what enqueue_n(n) launches.  The top rung is the largest
// k <= cap whose size is within graph_chunk (rung 0 when even the base is larger).
static int top_rung(int32_t graph_chunk, uint64_t base, int cap) {
    int k = 0;
    while ((base << (k + 1)) <= (uint64_t)graph_chunk && k < cap) ++k;
    return k;
}
// All the rungs are instantiated at once (nothing is instantiated inside a later, possibly timed, call).  The step
// counters live on the device, so the graphs do not depend on the step.  On failure the rungs captured so far stay in
// `ladder`: the caller drops them its own way.
template <typename EnqueueN>
static int build_ladder(bean_hip_ctx* c, std::vector<hipGraphExec_t>& ladder, hipStream_t stream, int n_rungs, uint64_t base,
                        bool head_fresh, EnqueueN&& enqueue_n) {
    for (int k = 0; k < n_rungs; ++k) {
        hipGraphExec_t ge = nullptr;
        if (capture_graph(c, stream, head_fresh, [&] { return enqueue_n(base << k); }, &ge)) return -1;
        ladder.push_back(ge);
    }
    return 0;
}

// `pairs` {k_param, guide} pairs as a sum of the rungs of a ladder of base 1 (bean_hip_svi_run and the ensemble).
// Smallest graphs first: the device works on them while the host submits the larger ones (a launch of the 64-pair graph
// costs the host more than the step or two already enqueued); the top rung is repeated.  A graph launch costs ~8.5 us
// of idle device time at its boundary - measured on the kernel timeline of a 20-step call - so one or two pairs are
// launched directly: six eager launches run back to back.
template <typename EnqueueN>
static int replay_pairs(bean_hip_ctx* c, const std::vector<hipGraphExec_t>& ladder, hipStream_t stream, uint64_t pairs,
                        EnqueueN&& enqueue_n) {
    const int kmax = (int)ladder.size() - 1;
    const uint64_t big = pairs >> kmax;           // launches of the largest graph
    const uint64_t rest = pairs - (big << kmax);  // < 2^kmax: one launch per set bit, ascending
    for (int k = 0; k < kmax; ++k)
        if (rest & (1ull << k)) {
            if (k < 2) enqueue_n(1ull << k);
            else {
                HIP_OK(hipGraphLaunch(ladder[k], stream));
                c->alleles_fresh = true;  // (a graph of pairs ends with a guide launch)
            }
        }
    for (uint64_t i = 0; i < big; ++i) {
        HIP_OK(hipGraphLaunch(ladder[kmax], stream));
        c->alleles_fresh = true;
    }
    return 0;
}

// The ladder of an ArgSet, cut like bean_hip_svi_run's pair path: graphs of 1, 2, 4, ... <= graph_chunk units of what
// enqueue_n launches.  A ladder of another size is this set's alone to drop; so is one that could not be built.
template <typename EnqueueN>
static int ensure_ladder(bean_hip_ctx* c, ArgSet& a, hipStream_t stream, int32_t graph_chunk, EnqueueN&& enqueue_n) {
    const int n_rungs = top_rung(graph_chunk, 1, 10) + 1;
    if ((int)a.ladder.size() == n_rungs) return 0;
    destroy_graphs(a.ladder);
    if (build_ladder(c, a.ladder, stream, n_rungs, 1, c->alleles_fresh, enqueue_n)) {
        destroy_graphs(a.ladder);
        return -1;
    }
    return 0;
}

#ifdef BEAN_AB_KERNELS

// ---- one launch per call: bean_tile_svi.hpp
template <int FAM, bool ACC>
static int launch_svi_tile_t(bean_hip_ctx* c, hipStream_t stream, uint64_t step0, uint64_t slot0, uint64_t n_steps,
                             bool prep_last) {
    const DevArgs& d = c->d;
    const size_t lds = svi_tile_lds(d.B, d.R, c->tile_ntm, c->tile_gbm);
    if (c->tile_blocks == 0) {
        int per_cu = 0, dev = 0, n_cu = 0;
        HIP_OK(hipFuncSetAttribute((const void*)k_svi_tile<FAM, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_svi_tile<FAM, ACC>, kTileThreads, lds));
        HIP_OK(hipGetDevice(&dev));
        HIP_OK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        if (per_cu < 1) return fail("k_svi_tile does not fit on a compute unit (LDS " + std::to_string(lds) + " bytes)");
        c->tile_blocks = per_cu * n_cu;
        if (getenv("BEAN_HIP_VERBOSE"))
            fprintf(stderr, "k_svi_tile: %d tiles (<= %d targets, %d guides), LDS %zu B, %d workgroups per CU x %d CUs\n",
                    c->n_tiles, c->tile_ntm, c->tile_gbm, lds, per_cu, n_cu);
    }
    const int blocks = c->n_tiles < c->tile_blocks ? c->n_tiles : c->tile_blocks;
    const int* tg0 = c->tile_tab;
    const int* tt0 = c->tile_tab + (c->n_tiles + 1);
    const bool prof = prof_guide(c);
    launch_timed(c, prof, k_svi_tile<FAM, ACC>, dim3(blocks), dim3(kTileThreads), lds, stream, d, (const DevArgs*)c->dargs_dev,
                 tg0, tt0, c->n_tiles, c->tile_ntm, c->tile_gbm, (unsigned long long)step0, (unsigned long long)slot0,
                 (int)n_steps, prep_last ? 1 : 0, (const float*)c->step_sizes);
    if (prof) c->ev_steps.push_back(n_steps);
    return 0;
}

static int launch_svi_tile(bean_hip_ctx* c, hipStream_t stream, uint64_t step0, uint64_t n_steps) {
    const DevArgs& d = c->d;
    if (n_steps > c->step_sizes_cap) {
        if (c->step_sizes) (void)hipFree(c->step_sizes);
        c->step_sizes = nullptr;
        c->step_sizes_cap = 0;
        const uint64_t cap = n_steps < 256 ? 256 : n_steps;
        HIP_OK(hipMalloc((void**)&c->step_sizes, cap * sizeof(float)));
        c->step_sizes_cap = cap;
    }
    hipLaunchKernelGGL(k_step_sizes, dim3((unsigned)((n_steps + 255) / 256)), dim3(256), 0, stream, d,
                       (unsigned long long)step0, (int)n_steps, c->step_sizes);
    if (!c->dargs_dev) HIP_OK(hipMalloc((void**)&c->dargs_dev, sizeof(DevArgs)));
    // (the kernel-argument copy and this one are the same bytes: c->d as it is now)
    hipLaunchKernelGGL(k_put_args, dim3(1), dim3(64), 0, stream, d, c->dargs_dev);
    return with_family_acc(d, [&](auto fam, auto acc) {
        return launch_svi_tile_t<fam(), acc()>(c, stream, step0, step0, n_steps, false);
    });
}

#endif  // BEAN_AB_KERNELS

// ---- all the steps of a call in one launch: bean_async_v2.hpp
// whether a call of n_steps steps takes the one asynchronous launch (bean_async_v2.hpp; a group's queue counter is an int)
static bool async_candidate(const bean_hip_ctx* c, uint64_t n_steps) {
    const DevArgs& d = c->d;
    const uint64_t per_group = (uint64_t)((d.n_tiles + 7) / 8) * (uint64_t)d.R;
    if (n_steps == 0 || per_group * n_steps > 2000000000ull) return false;
    return c->async_step && !c->profile_param && !per_step_noise(d) && !dumps_pi(d) && d.lpart && d.tile_ctr &&
           (d.family != kMixture || d.dgq);
}

template <int FAM, bool ACC>
static int launch_svi_async_t(bean_hip_ctx* c, hipStream_t stream, const AsyncArgs& a_in, int* roles_out) {
    const DevArgs& d = c->d;
    const size_t lds = guide_wave2_lds(d.B, d.tile_targets);
    if (c->async_blocks == 0) {
        // resident single-wave workgroups: the grid (nothing depends on residency but speed: a block that is
        // dispatched late finds what is left of its group's queue)
        int per_cu = 0, dev = 0, n_cu = 0;
        // (more than 64 KB of dynamic LDS per workgroup - many conditions - has to be asked for)
        if (lds > 65536)
            HIP_OK(hipFuncSetAttribute((const void*)k_svi_async<FAM, ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_svi_async<FAM, ACC>, 64, lds));
        HIP_OK(hipGetDevice(&dev));
        HIP_OK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
        if (per_cu < 1) return fail("k_svi_async does not fit on a compute unit (LDS " + std::to_string(lds) + " bytes)");
        // the same number of waves on every SIMD (four per CU): async_waves_per_simd, within what fits
        int k = async_waves_per_simd((long)d.n_tiles * d.R, 4l * n_cu);
        if (k > per_cu / 4) k = per_cu / 4;
        c->async_blocks = k >= 1 ? k * 4 * n_cu : per_cu * n_cu / 8 * 8;
        // finisher roles: one more wave per SIMD that only finishes tiles, where there is room for it and the item waves
        // have more than ~2 items per step each (async_finisher_roles)
        c->async_fin_blocks = (k >= 1 && k + 1 <= per_cu / 4 && async_finisher_roles(k, (long)d.n_tiles * d.R, 4l * n_cu)) ? 4 * n_cu : 0;
        if (const char* e = getenv("BEAN_HIP_ASYNC_BLOCKS")) {  // experiments
            const int v = atoi(e) / 8 * 8;
            if (v >= 8) c->async_blocks = v;
        }
        if (const char* e = getenv("BEAN_HIP_ASYNC_FIN")) {  // experiments: finisher blocks (0: no roles; -1: roles without finishers)
            const int v = atoi(e);
            c->async_fin_blocks = v < 0 ? -1 : v / 8 * 8;
        }
        if (getenv("BEAN_HIP_VERBOSE"))
            fprintf(stderr, "k_svi_async: %d tiles x %d replicates per step, LDS %zu B, %d workgroups per CU x %d CUs -> grid %d\n",
                    d.n_tiles, d.R, lds, per_cu, n_cu, c->async_blocks);
    }
    // no more waves than one step has items (a small screen would only add pollers)
    const long items = (long)((d.n_tiles + 7) / 8 * 8) * d.R;
    int blocks = c->async_blocks;
    if ((long)blocks > items) blocks = (int)((items + 7) / 8 * 8);
    AsyncArgs a = a_in;
    int fin_blocks = 0;
    // the finish as two ring positions (targets / guides on two finishers at once) while the item waves have few items per
    // step - then a tile's chain is what a step waits for - and as one entry beyond (same box, split / one entry: 50k guides
    // 48.5 / 51.3 us per step, 56k 53.2 / 53.3, 62.5k 59.4 / 58.8, 68.75k 65.5 / 64.4, 125k 97.0 / 95.7)
    a.fin_split = (double)d.n_tiles * d.R / (double)(c->async_blocks > 0 ? c->async_blocks : 1) < 2.15 ? 1 : 0;
    if (const char* e = getenv("BEAN_HIP_ASYNC_SPLIT")) a.fin_split = atoi(e) != 0;  // experiments
    if (c->async_fin_blocks != 0 && a.fring_stride > 0 && d.n_tiles <= 8 * 65535) {
        fin_blocks = c->async_fin_blocks < 0 ? 0 : c->async_fin_blocks;
        const int tiles8 = (d.n_tiles + 7) / 8 * 8;
        if (fin_blocks > tiles8) fin_blocks = tiles8;  // (no more finishers than tiles)
        a.n_guide_blocks = blocks;
        blocks += fin_blocks;
    } else {
        a.n_guide_blocks = 0;
    }
    const bool prof = prof_guide(c);
    launch_timed(c, prof, k_svi_async<FAM, ACC>, dim3(blocks), dim3(64), lds, stream, (const DevArgs*)c->dargs_dev, d.R,
                 d.n_tiles, a);
    if (prof) c->ev_steps.push_back((uint64_t)a.n_steps);
    if (roles_out) *roles_out = a.n_guide_blocks;
    return 0;
}

// n steps from step0 (loss slots from slot0) on the draw and tables already on the device; leaves the draw and tables
// of step0 + n, the step counters as n {guide, k_param} pairs would, and the loss accumulators filled (not finalized)
static int launch_svi_async(bean_hip_ctx* c, hipStream_t stream, uint64_t step0, uint64_t slot0, uint64_t n_steps) {
    const DevArgs& d = c->d;
    if (n_steps > c->step_sizes_cap) {
        if (c->step_sizes) (void)hipFree(c->step_sizes);
        c->step_sizes = nullptr;
        c->step_sizes_cap = 0;
        const uint64_t cap = n_steps < 256 ? 256 : n_steps;
        HIP_OK(hipMalloc((void**)&c->step_sizes, cap * sizeof(float)));
        c->step_sizes_cap = cap;
    }
    // [8 x stride] queue | abort word (a line of its own) | [8 x stride] finish-ring heads | done[2 n_tiles]:
    // zeroed by every call; behind them the finish rings (one or two words per step and tile of the group, by position:
    // async_fin_pos; zeroed by every call)
    const size_t ws_ints = (size_t)17 * kAsyncQueueStride + (size_t)2 * d.n_tiles;
    // (finish rings, and with them finisher roles, only for calls of fewer than 8 000 steps: the rings grow with the call)
    const size_t fring_stride = n_steps < 8000 ? (size_t)2 * ((d.n_tiles + 7) / 8) * n_steps : 0;
    const size_t need_ints = ws_ints + 8 * fring_stride;
    if (need_ints > c->async_ws_ints) {
        if (c->async_ws) (void)hipFree(c->async_ws);
        c->async_ws = nullptr;
        c->async_ws_ints = 0;
        HIP_OK(hipMalloc((void**)&c->async_ws, need_ints * sizeof(int)));
        c->async_ws_ints = need_ints;
    }
    // the out-of-line pieces of the kernel read DevArgs from a copy in global memory (the same bytes: c->d as it is now)
    if (!c->dargs_dev) HIP_OK(hipMalloc((void**)&c->dargs_dev, sizeof(DevArgs)));
    AsyncArgs a;
    a.step0 = step0;
    a.slot0 = slot0;
    a.n_steps = (int)n_steps;
    a.queue = c->async_ws;
    a.abort_flag = c->async_ws + 8 * kAsyncQueueStride;
    a.fhead = c->async_ws + 9 * kAsyncQueueStride;
    a.done = c->async_ws + 17 * kAsyncQueueStride;
    a.fring = c->async_ws + ws_ints;
    a.fring_stride = (long)fring_stride;
    a.n_guide_blocks = 0;  // (set by launch_svi_async_t, where the grid is decided)
    a.fin_split = 0;
    a.early = c->async_early;
    a.step_sizes = c->step_sizes;
    a.stamps = nullptr;
    // queue, abort and completed-step words to zero, step sizes, the DevArgs copy, the step counters the call leaves
    {
        unsigned hb = (unsigned)((8 * fring_stride + 256 * 64 - 1) / (256 * 64));  // ~64 ring words per thread
        if (hb < 1) hb = 1;
        if (hb > 128) hb = 128;
        hipLaunchKernelGGL(k_async_head, dim3(hb), dim3(256), 0, stream, d, a, c->dargs_dev, c->async_ws, (int)ws_ints, c->step_sizes);
    }
#ifdef BEAN_ASYNC_STAMP
    {
        static unsigned long long* g_stamps = nullptr;
        const size_t words = (size_t)2 * kAsyncStampFinOff;  // item rows, then finish-phase rows
        if ((size_t)kAsyncStampSteps * ((d.n_tiles + 7) / 8 * 8) * d.R * 8 > (size_t)kAsyncStampFinOff)
            return fail("BEAN_ASYNC_STAMP: screen too large for the stamp buffer");
        if (!g_stamps) HIP_OK(hipMalloc((void**)&g_stamps, words * 8));
        HIP_OK(hipMemsetAsync(g_stamps, 0, words * 8, stream));
        a.stamps = g_stamps;
        c->async_stamps = g_stamps;
        c->async_stamp_words = words;
    }
#endif
    return with_family_acc(d, [&](auto fam, auto acc) { return launch_svi_async_t<fam(), acc()>(c, stream, a, nullptr); });
}

extern "C" int bean_hip_svi_run(bean_hip_ctx* c, uint64_t seed, uint64_t first_step, uint64_t n_steps,
                                int32_t graph_chunk, void* stream_) {
    const int go = begin_steps(c, "bean_hip_svi_run", first_step, n_steps);
    if (go <= 0) return go;
    hipStream_t stream = (hipStream_t)stream_;
    drop_graph_on_seed_change(c, seed);
    c->d.seed = seed;
    c->resume_ok = false;
    const DevArgs& dd = c->d;
    // one launch for all the steps of the call (bean_tile_svi.hpp) unless per-step noise is injected or
    // dumped, k_param is being timed, or the shape is not eligible
    const bool tile = c->tile_svi && c->tile_ready && !c->profile_param && !per_step_noise(dd) && !dumps_pi(dd);
    const bool use_graph = graph_chunk > 0 && stream != nullptr && !c->profile && !tile;
    // one launch per step unless per-step noise is injected or dumped, or k_param itself is being timed
    // (kDumpPi is not asked about here, unlike `tile` and the asynchronous path: inherited, not reviewed here)
    const bool fused = c->fused_step && !c->profile_param && !per_step_noise(dd);
    auto pairs_n = [&](uint64_t n) {
        enqueue_pairs(c, stream, n);
        return 0;
    };
    if (use_graph) {
        // graphs of 1, 2, 4, ... <= graph_chunk pairs; the one-launch step: of 2, 4, ... <= graph_chunk launches
        const int kmax = top_rung(graph_chunk, 1, 10);
        std::vector<hipGraphExec_t>& ladder = fused ? c->graphs_fused : c->graphs;
        const int n_rungs = fused ? (kmax > 0 ? kmax : 1) : kmax + 1;
        if ((int)ladder.size() != n_rungs) {
            drop_graph(c);
            auto fused_n = [&](uint64_t n) {
                enqueue_fused(c, stream, n);
                return 0;
            };
            const int rc = fused ? build_ladder(c, ladder, stream, n_rungs, 2, c->alleles_fresh, fused_n)
                                 : build_ladder(c, ladder, stream, n_rungs, 1, c->alleles_fresh, pairs_n);
            if (rc) {
                drop_graph(c);
                return -1;
            }
            c->graph_seed = seed;
        }
    }
    first_draw(c, stream, first_step, n_steps);
    if (tile) {
#ifdef BEAN_AB_KERNELS
        if (launch_svi_tile(c, stream, first_step, n_steps)) return -1;
#endif
    } else if (async_candidate(c, n_steps) && stream != nullptr) {
        // one launch for the call: it also draws step first_step + n_steps, which nobody reads
        // (bean_hip_svi_resume takes this path on the null stream too: inherited, not reviewed here)
        if (launch_svi_async(c, stream, first_step, first_step, n_steps)) return -1;
    } else if (fused) {
        // n launches of k_step_wave2 = {guide work, FINISH, PREP of the next step}; graphs hold even
        // numbers of launches (the step counters ping-pong), largest first, an odd remainder is launched last
        uint64_t left = n_steps;
        if (use_graph) {
            for (int k = (int)c->graphs_fused.size() - 1; k >= 0; --k)
                while (left >= (2ull << k)) {
                    HIP_OK(hipGraphLaunch(c->graphs_fused[k], stream));
                    left -= 2ull << k;
                }
        }
        enqueue_fused(c, stream, left);
    } else {
        launch_guide(c, stream);
        if (use_graph) {
            if (replay_pairs(c, c->graphs, stream, n_steps - 1, pairs_n)) return -1;
        } else {
            enqueue_pairs(c, stream, n_steps - 1);
        }
        launch_param<true, true, false>(c, stream);
    }
    launch_finalize(c, stream, first_step, n_steps, false);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- seed ensembles (bean_ensemble.hpp): the pair path with a member axis, gridDim.y = K
static bool ensemble_shape_ok(const bean_hip_ctx* c) {
    const bean_hip_shape& s = c->shape;
    return c->wave_guide && c->wave2 && !is_survival(s) && s.n_sample_covariates == 0 &&
           (s.family == BEAN_FAMILY_NORMAL || s.family == BEAN_FAMILY_MIXTURE_NORMAL) && !c->async_step && !c->fused_step &&
           !c->tile_svi && s.guide_offset == 0 && s.target_offset == 0 &&
           (s.n_guides_total == 0 || s.n_guides_total == s.n_guides) &&
           !(s.flags & (BEAN_FLAG_NOT_LOSS_OWNER | BEAN_FLAG_DUMP_PI));
}

extern "C" int bean_hip_ensemble_supported(const bean_hip_ctx* c) {
    if (!c) return fail("bean_hip_ensemble_supported: null handle");
    return ensemble_shape_ok(c) ? 1 : 0;
}

// ---- survival member fits (bean_survival_ensemble.hpp): the survival variant pair path with the same member axis.
// The wave form only; and a number of timepoints whose dynamic LDS the single-fit launch is made with as it stands:
// launch_guide_survival_wave raises no kernel's dynamic limit, so neither does the member launch, and more than 64 KB
// (59 timepoints and up) is refused here.
static bool survival_members_shape_ok(const bean_hip_ctx* c) {
    const bean_hip_shape& s = c->shape;
    return c->surv_wave && is_survival(s) && !is_tiling(s) &&
           (s.family == BEAN_FAMILY_NORMAL || s.family == BEAN_FAMILY_MIXTURE_NORMAL) && s.n_sample_covariates == 0 &&
           s.guide_offset == 0 && s.target_offset == 0 && (s.n_guides_total == 0 || s.n_guides_total == s.n_guides) &&
           !(s.flags & (BEAN_FLAG_NOT_LOSS_OWNER | BEAN_FLAG_DUMP_PI)) && guide_survival_wave_lds(c->d.B) <= 65536;
}

extern "C" int bean_hip_survival_members_supported(const bean_hip_ctx* c) {
    if (!c) return fail("bean_hip_survival_members_supported: null handle");
    return survival_members_shape_ok(c) ? 1 : 0;
}

// what bean_hip_set_members, the two member binds and bean_hip_svi_run_ensemble admit: either member path.
// (bean_hip_set_particles keeps asking ensemble_shape_ok alone: particles on survival stay on the caller's loop)
static bool members_shape_ok(const bean_hip_ctx* c) { return ensemble_shape_ok(c) || survival_members_shape_ok(c); }

extern "C" int bean_hip_set_members(bean_hip_ctx* c, int32_t n_members) {
    if (!c) return fail("bean_hip_set_members: null handle");
    if (n_members < 1 || n_members > BEAN_HIP_MAX_MEMBERS)
        return fail("bean_hip_set_members: n_members must be in [1, " + std::to_string(BEAN_HIP_MAX_MEMBERS) + "]");
    if (!members_shape_ok(c))
        return fail("bean_hip_set_members: the batched kernels do not take this shape (bean_hip_ensemble_supported): "
                    "fit its seeds one after the other");
    if (c->bound_any) return fail("bean_hip_set_members: call it after bean_hip_create and before any bean_hip_bind");
    if (n_members > 1 && c->n_particles > 1)
        return fail("bean_hip_set_members: this handle steps " + std::to_string(c->n_particles) +
                    " particles (bean_hip_set_particles): particles inside member sets are not batched");
    static_assert(BEAN_HIP_MAX_MEMBERS == kEnsembleMaxMembers, "the header's cap is the kernels'");
    free_args(c->members);
    c->n_members = 1;
    if (c->n_particles == 1 && alloc_workspace_copies(c, n_members)) return -1;
    if (alloc_args(c->members, n_members)) return -1;
    c->n_members = n_members;
    c->members_set = true;
    c->member_rg = nullptr;  // (sized for another K)
    c->member_smask = nullptr;
    c->member_x = nullptr;
    c->member_xbc = nullptr;
    c->prepared = false;
    drop_graph(c);
    return 0;
}

// What members and particles share.  m is a copy of c->d: every pointer into the workspace moves to the k-th private
// copy of it (k >= 1) - every region of workspace_regions whose pointer lies in the workspace: sync_devargs may have put
// a caller's buffer in the place of gsum, sq or cov_sum - and tsum and the loss accumulators, allocations of their own,
// to their k-th part
static void relocate_private(const bean_hip_ctx* c, DevArgs& m, int k) {
    const char* w0 = (const char*)c->workspace;
    const char* w1 = w0 + c->workspace_bytes;
    const ptrdiff_t off = (c->member_ws + (size_t)(k - 1) * c->member_ws_stride) - (char*)c->workspace;
    workspace_regions(c, m, [&](auto& p, uint64_t) {
        const char* q = (const char*)p;
        if (q && q >= w0 && q < w1) p = (std::remove_reference_t<decltype(p)>)(const_cast<char*>(q) + off);
    });
    m.loss_acc += (size_t)k * c->loss_capacity * kLossSub * kLossWords;
    if (m.tsum) m.tsum += (size_t)k * c->tsum_stride;
}

// (n - 1) private copies of the workspace for n members or particles (filled by bean_hip_prepare)
static int alloc_workspace_copies(bean_hip_ctx* c, int n) {
    if (c->member_ws) (void)hipFree(c->member_ws);
    c->member_ws = nullptr;
    c->member_ws_stride = (size_t)((c->workspace_bytes + 255) / 256 * 256);
    if (n > 1) HIP_OK(hipMalloc((void**)&c->member_ws, (size_t)(n - 1) * c->member_ws_stride));
    return 0;
}

// DevArgs of member k: c->d with everything a step writes moved to the member's own part, the two masks at the
// member's slice when per-member masks are bound, and the counts at the member's slice when per-member counts are bound
static DevArgs member_args(const bean_hip_ctx* c, int k, uint64_t seed) {
    DevArgs m = c->d;
    m.seed = seed;
    m.tgrad = nullptr;
    if (c->member_rg) {  // per-member masks (bean_hip_bind_member_masks); member 0 reads its slice too
        m.rg = c->member_rg + (size_t)k * (size_t)c->d.R * (size_t)c->d.G;
        m.smask = c->member_smask + (size_t)k * (size_t)c->d.R * (size_t)c->d.B;
    }
    if (c->member_x) {  // per-member counts (bean_hip_bind_member_counts); member 0 reads its slice too
        const size_t n = (size_t)k * (size_t)c->d.R * (size_t)c->d.B * (size_t)c->d.G;
        m.X = c->member_x + n;
        if (c->member_xbc) m.Xbc = c->member_xbc + n;
    }
    if (k == 0) return m;
    relocate_private(c, m, k);
    for (int i = 0; i < 8; ++i) {
        const size_t n = (size_t)(expected_bytes(c->shape, BEAN_BUF_P_MU_LOC + i) / 4) * (size_t)k;
        if (m.p[i]) m.p[i] += n;
        if (m.g[i]) m.g[i] += n;
        if (m.m[i]) m.m[i] += n;
        if (m.v[i]) m.v[i] += n;
    }
    m.loss_hist += (size_t)k * c->loss_capacity;
    return m;
}

extern "C" int bean_hip_bind_member_masks(bean_hip_ctx* c, const void* repguide, uint64_t repguide_bytes,
                                          const void* sample_mask, uint64_t sample_mask_bytes) {
    if (!c) return fail("bean_hip_bind_member_masks: null handle");
    if (!members_shape_ok(c))
        return fail("bean_hip_bind_member_masks: the batched kernels do not take this shape (bean_hip_ensemble_supported)");
    if (!c->members_set) return fail("bean_hip_bind_member_masks: call bean_hip_set_members first");
    if ((repguide == nullptr) != (sample_mask == nullptr))
        return fail("bean_hip_bind_member_masks: the two masks go together (both, or null for both)");
    if (repguide) {
        const uint64_t K = (uint64_t)c->n_members;
        const uint64_t want_rg = K * (uint64_t)c->d.R * (uint64_t)c->d.G;
        const uint64_t want_sm = K * (uint64_t)c->d.R * (uint64_t)c->d.B * sizeof(double);
        if (repguide_bytes != want_rg)
            return fail("bean_hip_bind_member_masks: repguide expects " + std::to_string(want_rg) + " bytes (" +
                        std::to_string(K) + " member(s)), got " + std::to_string(repguide_bytes));
        if (sample_mask_bytes != want_sm)
            return fail("bean_hip_bind_member_masks: sample_mask expects " + std::to_string(want_sm) + " bytes (" +
                        std::to_string(K) + " member(s)), got " + std::to_string(sample_mask_bytes));
    }
    c->member_rg = (const uint8_t*)repguide;
    c->member_smask = (const double*)sample_mask;
    drop_graph(c);        // (the members' arguments are older than the masks now)
    c->prepared = false;  // the data-only constants are stale: bean_hip_prepare comes next
    return 0;
}

extern "C" int bean_hip_bind_member_counts(bean_hip_ctx* c, const void* x, uint64_t x_bytes, const void* x_bcmatch,
                                           uint64_t x_bcmatch_bytes) {
    if (!c) return fail("bean_hip_bind_member_counts: null handle");
    if (!members_shape_ok(c))
        return fail("bean_hip_bind_member_counts: the batched kernels do not take this shape (bean_hip_ensemble_supported)");
    if (!c->members_set) return fail("bean_hip_bind_member_counts: call bean_hip_set_members first");
    if (!x && x_bcmatch) return fail("bean_hip_bind_member_counts: x_bcmatch without x (both null returns to shared counts)");
    if (x) {
        const bool use_bc = (c->shape.flags & BEAN_FLAG_USE_BCMATCH) != 0;
        if (use_bc && !x_bcmatch)
            return fail("bean_hip_bind_member_counts: this handle uses the barcode-matched counts (BEAN_FLAG_USE_BCMATCH): "
                        "x_bcmatch is required");
        if (!use_bc && x_bcmatch)
            return fail("bean_hip_bind_member_counts: this handle does not use the barcode-matched counts "
                        "(BEAN_FLAG_USE_BCMATCH): x_bcmatch must be null");
        const uint64_t K = (uint64_t)c->n_members;
        const uint64_t want = K * (uint64_t)c->d.R * (uint64_t)c->d.B * (uint64_t)c->d.G * sizeof(float);
        if (x_bytes != want)
            return fail("bean_hip_bind_member_counts: x expects " + std::to_string(want) + " bytes (" + std::to_string(K) +
                        " member(s)), got " + std::to_string(x_bytes));
        if (x_bcmatch && x_bcmatch_bytes != want)
            return fail("bean_hip_bind_member_counts: x_bcmatch expects " + std::to_string(want) + " bytes (" +
                        std::to_string(K) + " member(s)), got " + std::to_string(x_bcmatch_bytes));
    }
    c->member_x = (const float*)x;
    c->member_xbc = (const float*)x_bcmatch;
    drop_graph(c);        // (the members' arguments are older than the counts now)
    c->prepared = false;  // the loss constant holds the counts' log-factorials: bean_hip_prepare comes next
    return 0;
}

static int ens_kind(const bean_hip_ctx* c) {
    const DevArgs& d = c->d;
    const bool kind1 = !d.survival && d.family != kMultiMixture && !d.wide_targets && !d.n_cov && d.wrow && d.rows_v2 &&
                       !d.rrow && !d.surv_q0lik && !d.not_loss_owner && d.lpart && (d.dgq || d.family != kMixture) && d.tsum;
    // (the survival MixtureNormal build, under launch_param's conditions; a member's tgrad is null: member_args)
    const bool kind2 = d.survival && d.family == kMixture && !d.surv_q0lik && d.dgq && !d.tsum && !d.wide_targets &&
                       !d.n_cov && d.wrow && d.rows_v2 && !d.rrow && d.lpart && d.lpt == kLanesPerTargetNarrow;
    if (param_generic_only()) return 0;
    return kind1 ? 1 : (kind2 ? 2 : 0);
}

// (mem, K: the members of an ensemble, or the particles of a fit)
template <bool FINISH, bool ADAM, bool PREP>
static void launch_param_ens(bean_hip_ctx* c, hipStream_t stream, const DevArgs* mem, int K) {
    int ntb, nb;
    grid_param(c, ntb, nb);
    const dim3 grid((unsigned)nb, (unsigned)K), block(kParamBlock);
    switch (ens_kind(c)) {
        case 1: hipLaunchKernelGGL((k_param_ens<FINISH, ADAM, PREP, 1>), grid, block, 0, stream, mem, ntb); break;
        case 2: hipLaunchKernelGGL((k_param_ens<FINISH, ADAM, PREP, 2>), grid, block, 0, stream, mem, ntb); break;
        default: hipLaunchKernelGGL((k_param_ens<FINISH, ADAM, PREP, 0>), grid, block, 0, stream, mem, ntb); break;
    }
}

// survival variant families: launch_guide_survival_wave's grid, times K on y (bean_survival_ensemble.hpp)
static void launch_guide_survival_ens(bean_hip_ctx* c, hipStream_t stream, const DevArgs* mem, int K) {
    const DevArgs& d = c->d;
    const int tiles = (d.G + 63) / 64;
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8) * (unsigned)d.R, (unsigned)K), block(64);
    const size_t lds = guide_survival_wave_lds(d.B);
    with_family_acc(d, [&](auto fam, auto acc) {
        hipLaunchKernelGGL((k_guide_survival_wave_ens<fam(), acc()>), grid, block, lds, stream, mem);
    });
    if (d.surv_q0lik)  // projection term of the G-dimensional Dirichlet's pathwise gradient, per member
        hipLaunchKernelGGL(k_sum_q_ens, dim3((unsigned)d.R, (unsigned)K), dim3(1024), 0, stream, mem);
}

static void launch_guide_ens(bean_hip_ctx* c, hipStream_t stream, const DevArgs* mem, int K) {
    const DevArgs& d = c->d;
    if (d.survival) {
        launch_guide_survival_ens(c, stream, mem, K);
        return;
    }
    const dim3 grid((unsigned)((d.n_tiles + 7) / 8 * 8) * (unsigned)d.R, (unsigned)K), block(64);
    const size_t lds = guide_wave2_lds(d.B, d.tile_targets);
    with_family_acc(d, [&](auto fam, auto acc) {
        hipLaunchKernelGGL((k_guide_wave2_ens<fam(), acc()>), grid, block, lds, stream, mem);
    });
}

static void enqueue_pairs_ens(bean_hip_ctx* c, hipStream_t stream, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        launch_param_ens<true, true, true>(c, stream, c->members.dev, c->n_members);
        launch_guide_ens(c, stream, c->members.dev, c->n_members);
    }
}

// the loss window of the call's n_steps steps of K members (particles) to zero, their step counters to first_step
static void launch_set_step_ens(hipStream_t stream, const DevArgs* mem, int K, uint64_t first_step, uint64_t n_steps) {
    const uint64_t words = n_steps * kLossSub * kLossWords;
    unsigned blocks = (unsigned)((words + 255) / 256);
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_set_step_ens, dim3(blocks, (unsigned)K), dim3(256), 0, stream, mem, (unsigned long long)first_step,
                       (unsigned long long)first_step, (unsigned long long)n_steps);
}
static void launch_finalize_ens(hipStream_t stream, const DevArgs* mem, int K, uint64_t first_step, uint64_t n_steps) {
    hipLaunchKernelGGL(k_loss_finalize_ens, dim3((unsigned)((n_steps + 3) / 4), (unsigned)K), dim3(n_steps == 1 ? 64 : 256), 0,
                       stream, mem, (unsigned long long)first_step, (unsigned long long)n_steps, 0);
}

// The checks bean_hip_svi_run_ensemble and bean_hip_svi_run_particles open with, in the order they have always had;
// `who` prefixes the messages.  Returns as begin_steps does.
static int begin_copies(bean_hip_ctx* c, const char* who_, bool particles, const uint64_t* seeds, int32_t n_seeds,
                        uint64_t first_step, uint64_t n_steps) {
    const std::string who = who_;
    if (!c) return fail(who + ": null handle");
    if (!seeds) return fail(who + ": null seeds");
    if (particles && !c->particles_set) return fail(who + ": call bean_hip_set_particles first");
    const int n = particles ? c->n_particles : c->n_members;
    if (n_seeds != n)
        return fail(who + ": " + std::to_string(n_seeds) + " seeds for " + std::to_string(n) +
                    (particles ? " particle(s) (bean_hip_set_particles)" : " member(s) (bean_hip_set_members)"));
    if (!(particles ? ensemble_shape_ok(c) : members_shape_ok(c)))
        return fail(who + ": the batched kernels do not take this shape (bean_hip_ensemble_supported)");
    // (pi_out without kDumpPi refuses here and nowhere else: inherited, not reviewed here)
    // (survival members: the draws and dumps of the survival sites are one buffer for all members, like the others)
    if (per_step_noise(c->d) || c->d.pi_out ||
        (c->d.survival && (c->d.x0_in || c->d.x0_out || c->d.eps_u_in || c->d.eps_u_out)))
        return fail(who + ": injected or dumped noise belongs to single " + (particles ? "evaluations" : "fits"));
    if (particles && check_bound(c, true, true)) return -1;  // (the mean gradient goes to the bound gradient buffers)
    return begin_steps(c, who_, first_step, n_steps);
}

extern "C" int bean_hip_svi_run_ensemble(bean_hip_ctx* c, const uint64_t* seeds, int32_t n_seeds, uint64_t first_step,
                                         uint64_t n_steps, int32_t graph_chunk, void* stream_) {
    const int go = begin_copies(c, "bean_hip_svi_run_ensemble", false, seeds, n_seeds, first_step, n_steps);
    if (go <= 0) return go;
    hipStream_t stream = (hipStream_t)stream_;
    c->resume_ok = false;
    const int K = c->n_members;
    if (c->d.survival && K > 1) {
        // relocate_private leaves a pointer outside the workspace alone: bound, the members would share these sums
        for (int slot : {BEAN_BUF_XCHG_GSUM, BEAN_BUF_XCHG_SQ})
            if (c->slot_ptr[slot])
                return fail(std::string("bean_hip_svi_run_ensemble: ") +
                            (slot == BEAN_BUF_XCHG_GSUM ? "BEAN_BUF_XCHG_GSUM" : "BEAN_BUF_XCHG_SQ") + " is bound: " +
                            std::to_string(K) + " survival members would share the exchange buffer (unbind it, or fit "
                            "one after the other)");
    }
    ArgSet& a = c->members;
    if (!a.dev && alloc_args(a, K)) return -1;  // (a handle that never heard of members is an ensemble of one)
    if (refresh_args(a, K, seeds, stream, [&](int k, uint64_t seed) { return member_args(c, k, seed); })) return -1;
    const bool use_graph = graph_chunk > 0 && stream != nullptr;
    auto pairs_n = [&](uint64_t n) {
        enqueue_pairs_ens(c, stream, n);
        return 0;
    };
    // the ladder of bean_hip_svi_run's pair path, of {k_param_ens, k_guide_wave2_ens} pairs (survival members:
    // {k_param_ens, k_guide_survival_wave_ens[, k_sum_q_ens]})
    if (use_graph && ensure_ladder(c, a, stream, graph_chunk, pairs_n)) return -1;
    launch_set_step_ens(stream, a.dev, K, first_step, n_steps);
    launch_param_ens<false, false, true>(c, stream, a.dev, K);
    launch_guide_ens(c, stream, a.dev, K);
    if (use_graph) {
        if (replay_pairs(c, a.ladder, stream, n_steps - 1, pairs_n)) return -1;
    } else {
        enqueue_pairs_ens(c, stream, n_steps - 1);
    }
    launch_param_ens<true, true, false>(c, stream, a.dev, K);
    launch_finalize_ens(stream, a.dev, K, first_step, n_steps);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- multi-particle SVI (bean_particles.hpp): P draws per step in the `_ens` launches, one update with their mean
extern "C" int bean_hip_set_particles(bean_hip_ctx* c, int32_t n_particles) {
    if (!c) return fail("bean_hip_set_particles: null handle");
    if (n_particles < 1 || n_particles > BEAN_HIP_MAX_MEMBERS)
        return fail("bean_hip_set_particles: n_particles must be in [1, " + std::to_string(BEAN_HIP_MAX_MEMBERS) + "]");
    if (!ensemble_shape_ok(c))
        return fail("bean_hip_set_particles: the batched kernels do not take this shape (bean_hip_ensemble_supported): "
                    "step its particles one after the other");
    if (c->bound_any) return fail("bean_hip_set_particles: call it after bean_hip_create and before any bean_hip_bind");
    if (c->n_members > 1)
        return fail("bean_hip_set_particles: this handle steps " + std::to_string(c->n_members) +
                    " members (bean_hip_set_members): particles inside member sets are not batched");
    if (c->particle_grad) (void)hipFree(c->particle_grad);
    c->particle_grad = nullptr;
    free_args(c->particles);
    c->n_particles = 1;
    c->particles_set = false;
    if (alloc_workspace_copies(c, n_particles)) return -1;
    uint64_t n_all = 0;
    for (int i = 0; i < 8; ++i) n_all += expected_bytes(c->shape, BEAN_BUF_P_MU_LOC + i) / 4;
    HIP_OK(hipMalloc((void**)&c->particle_grad, (size_t)n_all * (size_t)n_particles * sizeof(float)));
    HIP_OK(hipMemset(c->particle_grad, 0, (size_t)n_all * (size_t)n_particles * sizeof(float)));
    if (alloc_args(c->particles, n_particles)) return -1;
    c->n_particles = n_particles;
    c->particles_set = true;
    c->prepared = false;
    drop_graph(c);
    return 0;
}

// the bound parameter arrays end to end, and where each one's (P, n) scratch block lies in particle_grad
static ParticleArrays particle_arrays(const bean_hip_ctx* c) {
    ParticleArrays a;
    long at = 0;
    for (int i = 0; i < 8; ++i) {
        const long n = (long)(expected_bytes(c->shape, BEAN_BUF_P_MU_LOC + i) / 4);
        a.p[i] = c->d.p[i];
        a.g[i] = c->d.g[i];
        a.m[i] = c->d.m[i];
        a.v[i] = c->d.v[i];
        a.scratch[i] = c->particle_grad + (size_t)at * (size_t)c->n_particles;
        a.start[i] = at;
        at += n;
    }
    a.start[8] = at;
    return a;
}

// DevArgs of particle q: c->d - the shared parameters and moments - with everything a step writes moved to the
// particle's own part: the workspace copy, tsum, the loss accumulators, its scratch rows, its row of losses
static DevArgs particle_args(const bean_hip_ctx* c, int q, uint64_t seed) {
    DevArgs m = c->d;
    m.seed = seed;
    m.tgrad = nullptr;
    if (q > 0) relocate_private(c, m, q);
    const ParticleArrays a = particle_arrays(c);
    for (int i = 0; i < 8; ++i)
        if (m.g[i]) m.g[i] = const_cast<float*>(a.scratch[i]) + (size_t)q * (size_t)(a.start[i + 1] - a.start[i]);
    m.loss_hist = c->particle_loss + (size_t)q * c->loss_capacity;
    return m;
}

// n particle steps, four launches each; every one begins at the step counters the one before has left
static void enqueue_particle_steps(bean_hip_ctx* c, hipStream_t stream, uint64_t n) {
    const DevArgs* mem = c->particles.dev;
    const int P = c->n_particles;
    const ParticleArrays a = particle_arrays(c);
    const unsigned blocks = (unsigned)((a.start[8] + 255) / 256);
    for (uint64_t i = 0; i < n; ++i) {
        launch_param_ens<false, false, true>(c, stream, mem, P);
        launch_guide_ens(c, stream, mem, P);
        launch_param_ens<true, false, false>(c, stream, mem, P);
        hipLaunchKernelGGL(k_particle_adam, dim3(blocks), dim3(256), 0, stream, mem, P, a);
    }
}

extern "C" int bean_hip_svi_run_particles(bean_hip_ctx* c, const uint64_t* seeds, int32_t n_seeds, uint64_t first_step,
                                          uint64_t n_steps, int32_t graph_chunk, void* stream_) {
    const int go = begin_copies(c, "bean_hip_svi_run_particles", true, seeds, n_seeds, first_step, n_steps);
    if (go <= 0) return go;
    hipStream_t stream = (hipStream_t)stream_;
    c->resume_ok = false;
    const int P = c->n_particles;
    ArgSet& a = c->particles;
    if (refresh_args(a, P, seeds, stream, [&](int q, uint64_t seed) { return particle_args(c, q, seed); })) return -1;
    const bool use_graph = graph_chunk > 0 && stream != nullptr;
    auto steps_n = [&](uint64_t n) {
        enqueue_particle_steps(c, stream, n);
        return 0;
    };
    // a ladder of its own, of particle steps
    if (use_graph && ensure_ladder(c, a, stream, graph_chunk, steps_n)) return -1;
    launch_set_step_ens(stream, a.dev, P, first_step, n_steps);
    if (use_graph) {
        if (replay_pairs(c, a.ladder, stream, n_steps, steps_n)) return -1;
    } else {
        enqueue_particle_steps(c, stream, n_steps);
    }
    launch_finalize_ens(stream, a.dev, P, first_step, n_steps);
    hipLaunchKernelGGL(k_particle_loss, dim3((unsigned)((n_steps + 255) / 256)), dim3(256), 0, stream,
                       (const DevArgs*)a.dev, P, c->d.loss_hist, (unsigned long long)first_step,
                       (unsigned long long)n_steps);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- bean_hip_svi_resume: the loop of a fit that is stepped in windows (run_inference: 100 steps at a time)
// n steps and the loss of those n slots (finalized from the device step counter: the group is self-contained,
// so a captured one closes itself and no launch has to follow the last graph of a call)
static void enqueue_resume_pairs(bean_hip_ctx* c, hipStream_t stream, uint64_t n) {
    if (n == 0) return;
    for (uint64_t i = 0; i < n; ++i) {
        launch_guide(c, stream);
        launch_param<true, true, true>(c, stream);
    }
    launch_finalize(c, stream, 0, n, true);
}

// Replay of a resume graph: if it was captured with fresh allele tables at its head and they are not (cannot happen in
// a resume chain - its last launch was a PREP k_param with allele blocks - but nothing else promises it), k_allele runs
// first.  The graph ends with a PREP launch, i.e. in the state it was entered with.
static int launch_resume_graph(bean_hip_ctx* c, hipGraphExec_t ge, hipStream_t stream) {
    const DevArgs& d = c->d;
    if (d.family == kMultiMixture && c->resume_head_fresh && !c->alleles_fresh && d.n_live_slots > 0)
        hipLaunchKernelGGL(k_allele, dim3((unsigned)(((long)d.n_live_slots + 255) / 256)), dim3(256), 0, stream, d);
    HIP_OK(hipGraphLaunch(ge, stream));
    c->alleles_fresh = c->resume_head_fresh;
    return 0;
}

extern "C" int bean_hip_svi_resume(bean_hip_ctx* c, uint64_t seed, uint64_t first_step, uint64_t n_steps,
                                   int32_t graph_chunk, void* stream_) {
    // noise injected or dumped per step, a timed k_param, the opt-in steppers: the plain loop
    // (x0_* / eps_u_* are asked about here and not in bean_hip_svi_run's own path choices: inherited, not reviewed here)
    if (c && c->prepared) {
        const DevArgs& dd = c->d;
        if (per_step_noise(dd) || dd.x0_in || dd.eps_u_in || dd.x0_out || dd.eps_u_out || dumps_pi(dd) || c->profile ||
            c->profile_param || c->fused_step || c->tile_svi || stream_ == nullptr)
            return bean_hip_svi_run(c, seed, first_step, n_steps, graph_chunk, stream_);
    }
    const int go = begin_steps(c, "bean_hip_svi_resume", first_step, n_steps);
    if (go <= 0) return go;
    hipStream_t stream = (hipStream_t)stream_;
    drop_graph_on_seed_change(c, seed);
    const bool resumed = c->resume_ok && c->resume_next == first_step && c->resume_seed == seed &&
                         c->resume_stream == stream_;
    c->resume_ok = false;
    c->d.seed = seed;
    if (async_candidate(c, n_steps)) {
        // the whole window in one launch (bean_async_v2.hpp); windows chain exactly as the pairs do
        if (!resumed) first_draw(c, stream, first_step, n_steps);
        if (launch_svi_async(c, stream, first_step, first_step, n_steps)) return -1;
        launch_finalize(c, stream, first_step, n_steps, false);
        HIP_OK(hipGetLastError());
        mark_resumable(c, seed, first_step + n_steps, stream_);
        return 0;
    }
    int kmax = 0;
    if (graph_chunk > 1) {
        // graphs of 4, 8, ... <= graph_chunk {guide, k_param} pairs, each closed by its own finalize
        kmax = top_rung(graph_chunk, 4, 8);
        if ((int)c->graphs_resume.size() != kmax + 1) {
            drop_graph(c);
            // a graph's first node is a guide launch: it is captured in the state a resume chain enters it with - behind
            // a PREP launch of k_param - and a replay checks that state (launch_resume_graph)
            c->resume_head_fresh = param_prep_leaves_alleles_fresh(c);
            auto resume_n = [&](uint64_t n) {
                enqueue_resume_pairs(c, stream, n);
                return 0;
            };
            if (build_ladder(c, c->graphs_resume, stream, kmax + 1, 4, c->resume_head_fresh, resume_n)) {
                drop_graph(c);
                return -1;
            }
            c->graph_seed = seed;
        }
    }
    if (!resumed) first_draw(c, stream, first_step, n_steps);
    uint64_t left = n_steps;
    if (graph_chunk > 1 && !c->graphs_resume.empty()) {
        // one to four pairs directly - the device starts on an eager launch some 15 us sooner than on a graph
        // launch, and works on them while the host submits the graphs - then graphs, smallest first
        const uint64_t head = left % 4 ? left % 4 : (left >= 4 ? 4 : 0);
        enqueue_resume_pairs(c, stream, head);
        left -= head;
        const uint64_t big = left >> (kmax + 2);
        const uint64_t rest = left - (big << (kmax + 2));
        for (int k = 0; k < kmax; ++k)
            if (rest & (4ull << k))
                if (launch_resume_graph(c, c->graphs_resume[k], stream)) return -1;
        for (uint64_t i = 0; i < big; ++i)
            if (launch_resume_graph(c, c->graphs_resume[kmax], stream)) return -1;
        left = 0;
    }
    enqueue_resume_pairs(c, stream, left);
    HIP_OK(hipGetLastError());
    mark_resumable(c, seed, first_step + n_steps, stream_);  // (the last k_param was a PREP launch)
    return 0;
}

// ------------------------------------------------------------------ sharded / communicator
// ---- guide-sharded stepping with exchange points (see bean_hip.h)
extern "C" int bean_hip_sharded_begin(bean_hip_ctx* c, uint64_t seed, uint64_t first_step, uint64_t n_steps,
                                      void* stream_) {
    // (begin_steps' checks without its early return: an empty window is checked and prepares a draw like any other)
    if (!c) return fail("bean_hip_sharded_begin: null handle");
    if (!c->prepared) return fail("bean_hip_sharded_begin: call bean_hip_prepare first");
    if (check_bound(c, false, true)) return -1;
    if (first_step + n_steps > c->loss_capacity)
        return fail("bean_hip_sharded_begin: loss_hist too small for first_step + n_steps");
    if (is_survival(c->shape) && c->shape.family == BEAN_FAMILY_MIXTURE_NORMAL && !c->slot_ptr[BEAN_BUF_XCHG_GSUM])
        return fail("bean_hip_sharded_begin: bind BEAN_BUF_XCHG_GSUM for a sharded survival MixtureNormal fit");
    if (is_surv_normal(c->shape) && (!c->slot_ptr[BEAN_BUF_XCHG_GSUM] || !c->slot_ptr[BEAN_BUF_XCHG_SQ]))
        return fail("bean_hip_sharded_begin: bind BEAN_BUF_XCHG_GSUM and BEAN_BUF_XCHG_SQ for a sharded survival "
                    "NormalModel fit");
    if ((c->shape.family == BEAN_FAMILY_CONTROL_NORMAL || is_tiling(c->shape)) && !c->slot_ptr[BEAN_BUF_XCHG_TGRAD])
        return fail("bean_hip_sharded_begin: bind BEAN_BUF_XCHG_TGRAD for a sharded ControlNormal / tiling fit");
    hipStream_t stream = (hipStream_t)stream_;
    c->d.seed = seed;
    c->resume_ok = false;
    first_draw(c, stream, first_step, n_steps);
    c->sharded_steps = 0;
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bean_hip_sharded_sums(bean_hip_ctx* c, void* stream_) {
    if (!c) return fail("bean_hip_sharded_sums: null handle");
    // the normalisers of the survival families' Dirichlet-over-all-guides draw are formed at the tail of
    // the k_param launch that prepares the step (bean_hip_sharded_begin / _update): this rank's part is
    // already in BEAN_BUF_XCHG_GSUM when this returns.  Kept as the exchange point of the protocol.
    (void)stream_;
    return 0;
}

extern "C" int bean_hip_sharded_guide(bean_hip_ctx* c, void* stream_) {
    if (!c) return fail("bean_hip_sharded_guide: null handle");
    hipStream_t stream = (hipStream_t)stream_;
    launch_guide(c, stream);
    if (c->slot_ptr[BEAN_BUF_XCHG_TGRAD]) {
        int ntb, nb;
        grid_param(c, ntb, nb);
        hipLaunchKernelGGL(k_target_reduce, dim3(ntb), dim3(kParamBlock), 0, stream, c->d,
                           (double*)c->slot_ptr[BEAN_BUF_XCHG_TGRAD]);
    }
    if (c->d.n_cov && c->slot_ptr[BEAN_BUF_XCHG_COV])
        hipLaunchKernelGGL(k_cov_sum, dim3(c->d.R), dim3(1024), 0, stream, c->d);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bean_hip_sharded_update(bean_hip_ctx* c, int32_t last, void* stream_) {
    if (!c) return fail("bean_hip_sharded_update: null handle");
    hipStream_t stream = (hipStream_t)stream_;
    const double* tg = (const double*)c->slot_ptr[BEAN_BUF_XCHG_TGRAD];
    const bool covx = c->d.n_cov && c->slot_ptr[BEAN_BUF_XCHG_COV];
    if (last)
        launch_param<true, true, false>(c, stream, tg, covx);
    else
        launch_param<true, true, true>(c, stream, tg, covx);
    // the loss slots of the run's steps are finalized ONCE, by its last update (a launch per step cost every
    // exchanged step 4.7 us of device time - a twentieth of a 1/8-size tiling step, a tenth of a survival one)
    ++c->sharded_steps;
    if (last) {
        launch_finalize(c, stream, 0, c->sharded_steps, true);  // the slots that end with the step just finished
        c->sharded_steps = 0;
    }
    HIP_OK(hipGetLastError());
    return 0;
}


// ---- RCCL owned by the library (see bean_hip.h): resolved at run time from the shared object the
// caller names (the copy PyTorch has loaded), so libbean_hip.so has no link-time dependency on it
struct RcclApi {
    void* handle;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*);
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*GroupStart)();
    ncclResult_t (*GroupEnd)();
    const char* (*GetErrorString)(ncclResult_t);
};
static RcclApi g_rccl = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

static int rccl_load(const char* path) {
    if (g_rccl.handle) return 0;
    void* h = nullptr;
    if (path && path[0]) h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(std::string("RCCL not found (") + (path ? path : "") + "): " + (dlerror() ? dlerror() : ""));
    RcclApi a;
    a.handle = h;
#define BEAN_RCCL_SYM(field, name)                                               \
    a.field = (decltype(a.field))dlsym(h, name);                                 \
    if (!a.field) return fail(std::string("RCCL symbol missing: ") + name)
    BEAN_RCCL_SYM(GetUniqueId, "ncclGetUniqueId");
    BEAN_RCCL_SYM(CommInitRank, "ncclCommInitRank");
    BEAN_RCCL_SYM(CommDestroy, "ncclCommDestroy");
    BEAN_RCCL_SYM(AllReduce, "ncclAllReduce");
    BEAN_RCCL_SYM(GroupStart, "ncclGroupStart");
    BEAN_RCCL_SYM(GroupEnd, "ncclGroupEnd");
    BEAN_RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef BEAN_RCCL_SYM
    g_rccl = a;
    return 0;
}
#define RCCL_OK(expr)                                                                        \
    do {                                                                                     \
        ncclResult_t r_ = (expr);                                                            \
        if (r_ != ncclSuccess)                                                               \
            return fail(std::string(#expr) + ": " + g_rccl.GetErrorString(r_));              \
    } while (0)

extern "C" int bean_hip_comm_unique_id(const char* rccl_path, uint8_t* id) {
    if (!id) return fail("bean_hip_comm_unique_id: null id");
    if (rccl_load(rccl_path)) return -1;
    static_assert(sizeof(ncclUniqueId) == BEAN_HIP_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    ncclUniqueId u;
    RCCL_OK(g_rccl.GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return 0;
}

extern "C" int bean_hip_comm_init(bean_hip_ctx* c, const char* rccl_path, const uint8_t* id, int32_t rank,
                                  int32_t world) {
    if (!c || !id) return fail("bean_hip_comm_init: null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail("bean_hip_comm_init: rank / world out of range");
    if (c->comm) return fail("bean_hip_comm_init: communicator already initialised");
    if (rccl_load(rccl_path)) return -1;
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t comm = nullptr;
    RCCL_OK(g_rccl.CommInitRank(&comm, world, u, rank));
    c->comm = comm;
    c->comm_world = world;
    drop_graph(c);
    return 0;
}

extern "C" int bean_hip_comm_all_reduce(bean_hip_ctx* c, double* buf, uint64_t n, void* stream_) {
    if (!c || !buf) return fail("bean_hip_comm_all_reduce: null argument");
    if (!c->comm) return fail("bean_hip_comm_all_reduce: no communicator (bean_hip_comm_init)");
    RCCL_OK(g_rccl.AllReduce(buf, buf, (size_t)n, ncclFloat64, ncclSum, c->comm, (hipStream_t)stream_));
    return 0;
}

extern "C" int bean_hip_comm_destroy(bean_hip_ctx* c) {
    if (!c || !c->comm) return 0;
    drop_graph(c);
    ncclComm_t comm = c->comm;
    c->comm = nullptr;
    c->comm_world = 0;
    RCCL_OK(g_rccl.CommDestroy(comm));
    return 0;
}

// one exchanged step on `stream`: [all-reduce gsum] guide [all-reduce tgrad (+ sq)] update
// (fin_n > 0: this step closes the run - the loss slots of its fin_n steps are finalized behind it)
static int enqueue_exchanged_step(bean_hip_ctx* c, hipStream_t stream, bool last, uint64_t fin_n = 0) {
    const bean_hip_shape& s = c->shape;
    double* gsum = (double*)c->slot_ptr[BEAN_BUF_XCHG_GSUM];
    double* tg = (double*)c->slot_ptr[BEAN_BUF_XCHG_TGRAD];
    double* sq = (double*)c->slot_ptr[BEAN_BUF_XCHG_SQ];
    if (gsum) RCCL_OK(g_rccl.AllReduce(gsum, gsum, (size_t)s.n_reps + 1, ncclFloat64, ncclSum, c->comm, stream));
    launch_guide(c, stream);
    if (tg) {
        int ntb, nb;
        grid_param(c, ntb, nb);
        hipLaunchKernelGGL(k_target_reduce, dim3(ntb), dim3(kParamBlock), 0, stream, c->d, tg);
    }
    double* cov = c->d.n_cov ? (double*)c->slot_ptr[BEAN_BUF_XCHG_COV] : nullptr;
    if (cov) hipLaunchKernelGGL(k_cov_sum, dim3(c->d.R), dim3(1024), 0, stream, c->d);
    const int n_coll = (tg ? 1 : 0) + (sq ? 1 : 0) + (cov ? 1 : 0);
    {
        // a group that has been opened is ALWAYS closed, whatever fails inside it: a rank that returned between
        // GroupStart and GroupEnd would leave its peers inside the collective (and a capturing stream half-captured)
        const bool grouped = n_coll > 1;
        ncclResult_t r = ncclSuccess, rg = ncclSuccess;
        const char* what = "";
        if (grouped) {
            r = g_rccl.GroupStart();
            what = "ncclGroupStart";
        }
        const bool opened = grouped && r == ncclSuccess;
        if (r == ncclSuccess && tg) {
            r = g_rccl.AllReduce(tg, tg, (size_t)2 * s.n_targets, ncclFloat64, ncclSum, c->comm, stream);
            what = "ncclAllReduce(tgrad)";
        }
        if (r == ncclSuccess && sq) {
            r = g_rccl.AllReduce(sq, sq, (size_t)s.n_reps, ncclFloat64, ncclSum, c->comm, stream);
            what = "ncclAllReduce(sq)";
        }
        if (r == ncclSuccess && cov) {
            r = g_rccl.AllReduce(cov, cov, (size_t)s.n_reps, ncclFloat64, ncclSum, c->comm, stream);
            what = "ncclAllReduce(cov)";
        }
        if (opened) rg = g_rccl.GroupEnd();
        if (r != ncclSuccess) return fail(std::string(what) + ": " + g_rccl.GetErrorString(r));
        if (rg != ncclSuccess) return fail(std::string("ncclGroupEnd: ") + g_rccl.GetErrorString(rg));
    }
    if (last) launch_param<true, true, false>(c, stream, tg, cov != nullptr);
    else launch_param<true, true, true>(c, stream, tg, cov != nullptr);
    if (fin_n) launch_finalize(c, stream, 0, fin_n, true);  // the slots that end with the step just finished
    return 0;
}

extern "C" int bean_hip_svi_run_exchanged(bean_hip_ctx* c, uint64_t seed, uint64_t first_step, uint64_t n_steps,
                                          int32_t graph_chunk, void* stream_) {
    if (!c) return fail("bean_hip_svi_run_exchanged: null handle");
    if (!c->comm) return fail("bean_hip_svi_run_exchanged: call bean_hip_comm_init first");
    if (n_steps == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    drop_graph_on_seed_change(c, seed);
    if (bean_hip_sharded_begin(c, seed, first_step, n_steps, stream_)) return -1;  // checks, loss window, draw of step 0
    uint64_t left = n_steps;
    // hipGraphs of 2, 4, ... <= graph_chunk exchanged steps (never holding a run's last step, whose update
    // prepares no further draw); the remainder is enqueued directly
    if (graph_chunk > 1 && stream != nullptr && !c->profile) {
        if (c->graphs_xchg.empty()) {
            // (tiling: a graph's first node is a guide launch; it is captured in the state every replay enters it with -
            // behind a PREP launch of k_param, bean_hip_sharded_begin's or an exchanged update's - and a replay checks
            // that state, as launch_resume_graph does)
            c->resume_head_fresh = param_prep_leaves_alleles_fresh(c);
            // the capture is ended whether or not a step failed inside it (enqueue_exchanged_step closes its RCCL
            // group on every path, capture_graph destroys the partial graph)
            auto steps_n = [&](uint64_t n) {
                int rc = 0;
                for (uint64_t i = 0; rc == 0 && i < n; ++i) rc = enqueue_exchanged_step(c, stream, false);
                return rc;
            };
            if (build_ladder(c, c->graphs_xchg, stream, top_rung(graph_chunk, 2, 9) + 1, 2, c->resume_head_fresh, steps_n)) {
                // RCCL (or HIP) refused the capture: forget graphs, keep going eagerly
                (void)hipGetLastError();
                drop_graph(c);
                g_err = "bean_hip_svi_run_exchanged: the exchanged step could not be captured into a hipGraph; "
                        "running it with eager launches";
            }
            c->graph_seed = seed;
        }
        for (int k = (int)c->graphs_xchg.size() - 1; k >= 0; --k)
            while (left > (2ull << k)) {  // strictly more: the last step stays outside the graphs
                if (launch_resume_graph(c, c->graphs_xchg[k], stream)) return -1;  // (ends with an exchanged PREP update)
                left -= 2ull << k;
            }
    }
    for (; left > 0; --left)
        if (enqueue_exchanged_step(c, stream, left == 1, left == 1 ? n_steps : 0)) return -1;
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ introspection
extern "C" uint64_t bean_hip_step_bytes(const bean_hip_ctx* c) {
    if (!c) return 0;
    const bean_hip_shape& s = c->shape;
    const uint64_t R = s.n_reps, B = s.n_condits, G = s.n_guides, T = s.n_targets, A = s.n_max_alleles;
    const bool bc = s.flags & BEAN_FLAG_USE_BCMATCH;
    // counts (f32) once per likelihood, repguide mask, per-guide a0 / a0_bc / g2t
    uint64_t bytes = G * (4 * R * B * (bc ? 2 : 1) + R + 8 * (bc ? 2 : 1) + 4);
    if (is_mixture(s)) bytes += G * (4 * R * s.n_ctrl * A + 8 /*pi_a0*/ + 3 * 4 * A * 2 /*alpha_pi, m, v r+w*/);
    if (is_tiling(s)) bytes += G * A /*allele_mask*/ + 4 * (G * (A - 1) + 1) + 2 * 4 * (uint64_t)s.n_a2e_nnz + 4 * (T + 1);
    if (s.flags & BEAN_FLAG_SCALE_BY_ACC) bytes += G * (8 + ((s.flags & BEAN_FLAG_FIT_NOISE) ? 2 * 3 * 4 * 2 : 0));
    bytes += T * ((is_survival(s) ? 2 : 4) * 3 * 4 * 2);  // per-target params with moments, read + written
    if (is_survival(s) && s.family == BEAN_FAMILY_MIXTURE_NORMAL) bytes += G * (3 * 4 * 2 /*q0*/ + 8 * R /*log_obs0*/);
    return bytes;
}

extern "C" const char* bean_hip_dominant_kernel(const bean_hip_ctx* c) {
    if (c && c->d.family == kMultiMixture)
        return c->tiling_wide ? "k_guide_tiling_wide"
                              : (c->tiling_rep ? "k_guide_tiling_rep" : (c->tiling_wave ? "k_guide_tiling_wave" : "k_guide_tiling"));
    if (c && c->d.survival) return c->surv_wave ? "k_guide_survival_wave" : "k_guide_survival";
    if (c && c->wave_guide && c->tile_svi && c->tile_ready) return "k_svi_tile";
    if (c && c->wave_guide && c->wave2 && c->async_step) return "k_svi_async";
    if (c && c->wave_guide) return c->wave2 ? (c->fused_step ? "k_step_wave2" : "k_guide_wave2") : "k_guide_wave";
    return "k_lik";
}

extern "C" const char* bean_hip_dominant_kernel_variant(const bean_hip_ctx* c) {
    static thread_local std::string name;
    if (!c) return "";
    const DevArgs& d = c->d;
    const char* acc = (d.flags & kAcc) ? "true" : "false";
    const char* surv = d.survival ? "true" : "false";
    const std::string base = bean_hip_dominant_kernel(c);
    if (d.family == kMultiMixture) name = base + "<" + acc + ", " + surv + ">";
    else if (base == "k_guide_wave2" || base == "k_guide_survival_wave" || base == "k_step_wave2" || base == "k_svi_tile" ||
             base == "k_guide_wave" || base == "k_svi_async")
        name = base + "<" + (d.family == kMixture ? "2" : "0") + ", " + (d.family == kMixture ? acc : "false") + ">";
    else name = base;
    return name.c_str();
}

extern "C" uint64_t bean_hip_dominant_lds_bytes(const bean_hip_ctx* c) {
    if (!c) return 0;
    const DevArgs& d = c->d;
    const bool acc = (d.flags & kAcc) != 0;
    if (d.family == kMultiMixture) {
        if (c->tiling_wide) return 0;
        const uint64_t nt = c->tiling_rep ? 64ull * c->tiling_rep_w : 64ull;
        return guide_tiling_lds(d.B, acc, (size_t)nt, !c->tiling_rep);
    }
    if (d.survival) return c->surv_wave ? guide_survival_wave_lds(d.B) : 0;
    if (c->wave_guide && c->wave2) return guide_wave2_lds(d.B, d.tile_targets);
    return 0;
}

extern "C" int bean_hip_set_profile(bean_hip_ctx* c, int32_t enable) {
    if (!c) return fail("bean_hip_set_profile: null handle");
    c->profile = enable != 0;
    c->profile_param = enable == 2;
    if (c->profile) drop_graph(c);
    return 0;
}

extern "C" int bean_hip_get_profile(bean_hip_ctx* c, double* avg_ms, uint64_t* launches) {
    if (!c || !avg_ms || !launches) return fail("bean_hip_get_profile: null argument");
    double total = 0.0;
    uint64_t n = 0;
    for (size_t i = 0; i + 1 < c->ev.size(); i += 2) {
        HIP_OK(hipEventSynchronize(c->ev[i + 1]));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        total += ms;
        // a launch of k_svi_tile covers all the steps of its call: the average is per SVI step
        n += (c->ev_steps.size() * 2 == c->ev.size()) ? c->ev_steps[i / 2] : 1;
    }
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    c->ev.clear();
    c->ev_steps.clear();
    *avg_ms = n ? total / (double)n : 0.0;
    *launches = n;
    return 0;
}

#ifdef BEAN_ASYNC_STAMP
// diagnostic builds only: the item timeline of the last k_svi_async call (bean_async_v2.hpp)
extern "C" int64_t bean_hip_async_stamps(bean_hip_ctx* c, unsigned long long* host, uint64_t n_words) {
    HIP_OK(hipDeviceSynchronize());
    if (!c->async_stamps) return 0;
    const uint64_t n = n_words < c->async_stamp_words ? n_words : c->async_stamp_words;
    HIP_OK(hipMemcpy(host, c->async_stamps, n * 8, hipMemcpyDeviceToHost));
    return (int64_t)c->async_stamp_words;
}
#endif

#ifdef BEAN_STAMP
// diagnostic builds only: copy the per-wave cycle stamps of the last k_lik launch to the host
extern "C" int bean_hip_debug_stamps(bean_hip_ctx* c, unsigned long long* host, uint64_t n_words) {
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(host, c->d.dbg, n_words * 8, hipMemcpyDeviceToHost));
    return 0;
}
#endif

extern "C" int bean_hip_test_special(int32_t op, uint64_t n, const double* a, const double* x,
                                     const double* b, double* out0, double* out1, void* stream_) {
    if (op < 0 || op > 25) return fail("bean_hip_test_special: unknown op");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_test_special, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_,
                       (int)op, (long)n, a, x, b, out0, out1);
    HIP_OK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ posterior predictive replicate counts
// (bean_predictive.hpp, bean_survival_predictive.hpp)
static bool predictive_shape_ok(const bean_hip_ctx* c) {
    const bean_hip_shape& s = c->shape;
    return c->wave_guide && c->wave2 && c->fused_guide && !is_survival(s) && s.n_sample_covariates == 0 &&
           (s.family == BEAN_FAMILY_NORMAL || s.family == BEAN_FAMILY_MIXTURE_NORMAL) && s.guide_offset == 0 &&
           s.target_offset == 0 && (s.n_guides_total == 0 || s.n_guides_total == s.n_guides) &&
           !(s.flags & BEAN_FLAG_NOT_LOSS_OWNER) && c->n_members == 1 && c->n_particles == 1;
}

extern "C" int bean_hip_predictive_supported(const bean_hip_ctx* c) {
    if (!c) return fail("bean_hip_predictive_supported: null handle");
    return predictive_shape_ok(c) ? 1 : 0;
}

// ... and of survival screens.  Such a handle has no k_guide_wave2 (wave2 is false), so bean_hip_create leaves it
// g_sh == 0 and n_tiles == (G + 63) / 64: pair_grid() below is the grid of k_guide_survival_wave.
static bool survival_predictive_shape_ok(const bean_hip_ctx* c) {
    const bean_hip_shape& s = c->shape;
    return is_survival(s) && !is_tiling(s) && s.n_sample_covariates == 0 &&
           (s.family == BEAN_FAMILY_NORMAL || s.family == BEAN_FAMILY_MIXTURE_NORMAL) && s.guide_offset == 0 &&
           s.target_offset == 0 && (s.n_guides_total == 0 || s.n_guides_total == s.n_guides) &&
           !(s.flags & BEAN_FLAG_NOT_LOSS_OWNER) && c->n_members == 1 && c->n_particles == 1;
}

extern "C" int bean_hip_survival_predictive_supported(const bean_hip_ctx* c) {
    if (!c) return fail("bean_hip_survival_predictive_supported: null handle");
    return survival_predictive_shape_ok(c) ? 1 : 0;
}

// ---- what the post-fit entry points share.  Each composes these in its own order: a call that is wrong twice is
// refused for the first reason the entry point tests.
// A null handle, a handle `ok` does not take, an unprepared one; `stem` is the entry point's own sentence ("the count
// simulator does not take this handle") and `takes` names the probe of `ok` and the handles it admits.
static const char* const kSortingHandles = " (bean_hip_predictive_supported): sorting variant Normal / MixtureNormal, "
                                           "unsharded, no sample covariates, one member, one particle";
static const char* const kSurvivalHandles = " (bean_hip_survival_predictive_supported): survival variant Normal / "
                                            "MixtureNormal, unsharded, no sample covariates, one member, one particle";
static int postfit_admit(const bean_hip_ctx* c, const std::string& name, const char* stem,
                         bool (*ok)(const bean_hip_ctx*) = predictive_shape_ok, const char* takes = kSortingHandles) {
    if (!c) return fail(name + ": null handle");
    if (!ok(c)) return fail(name + ": " + stem + takes);
    if (!c->prepared) return fail(name + ": call bean_hip_prepare first");
    return 0;
}
// ... and, for the grid posterior, a handle with accessibility
static int grid_admit(const bean_hip_ctx* c, const std::string& name) {
    if (postfit_admit(c, name, "the grid posterior does not take this handle")) return -1;
    if (c->shape.flags & BEAN_FLAG_SCALE_BY_ACC)
        return fail(name + ": a handle with accessibility (BEAN_FLAG_SCALE_BY_ACC) is refused: the guide "
                    "noise is a further latent per guide, so the posterior of a target is not 2-D");
    return 0;
}

// A caller's buffer `what` of the given shape: there, with exactly n bytes ...
static int buf_exact(const std::string& name, const char* what, const std::string& shape, const void* p, uint64_t bytes,
                     uint64_t n) {
    if (!p || bytes != n) return fail(name + ": " + what + " must hold " + shape + ", " + std::to_string(n) + " bytes");
    return 0;
}
// ... or null with 0 bytes
static int buf_optional(const std::string& name, const char* what, const std::string& shape, const void* p,
                        uint64_t bytes, uint64_t n) {
    if (p ? bytes != n : bytes != 0)
        return fail(name + ": " + what + " must be null or hold " + shape + ", " + std::to_string(n) + " bytes");
    return 0;
}
// the simulators' counts: `planes` x (R, B, G) float32 in x_out, and in xbc_out exactly where the handle uses them
static int sim_buffers(const bean_hip_ctx* c, const std::string& name, const std::string& shape, uint64_t planes,
                       const void* x_out, uint64_t x_bytes, const void* xbc_out, uint64_t xbc_bytes) {
    const DevArgs& d = c->d;
    const uint64_t n = 4 * planes * d.R * d.B * d.G;
    if (buf_exact(name, "x_out", shape, x_out, x_bytes, n)) return -1;
    if (d.flags & kUseBc)
        return buf_exact(name, "this handle uses the barcode-matched counts: xbc_out", shape, xbc_out, xbc_bytes, n);
    if (xbc_out || xbc_bytes) return fail(name + ": xbc_out on a handle without BEAN_FLAG_USE_BCMATCH");
    return 0;
}
// the importance weights' outputs: (n_draws, T) float64 in logw_out, mu_out and - optional - y_out, (n_draws, R, G) in
// pair_out
static int logw_buffers(const bean_hip_ctx* c, const std::string& name, int32_t n_draws, const void* logw_out,
                        uint64_t logw_bytes, const void* mu_out, uint64_t mu_bytes, const void* y_out, uint64_t y_bytes,
                        const void* pair_out, uint64_t pair_bytes) {
    const DevArgs& d = c->d;
    const uint64_t nt = 8 * (uint64_t)n_draws * d.T, np = 8 * (uint64_t)n_draws * d.R * d.G;
    const std::string of = " float64 with n_draws = " + std::to_string(n_draws);
    if (buf_exact(name, "logw_out", "(n_draws, T)" + of, logw_out, logw_bytes, nt)) return -1;
    if (buf_exact(name, "mu_out", "(n_draws, T)" + of, mu_out, mu_bytes, nt)) return -1;
    if (buf_optional(name, "y_out", "(n_draws, T)" + of, y_out, y_bytes, nt)) return -1;
    return buf_exact(name, "pair_out (caller-owned scratch)", "(n_draws, R, G)" + of, pair_out, pair_bytes, np);
}

// launch geometry: kLogwBlock lanes per block over n items ...
static dim3 logw_blocks(uint64_t n) { return dim3((unsigned)((n + kLogwBlock - 1) / kLogwBlock)); }
// ... and one wave per (tile, replicate), the tiles rounded up to a multiple of 8, times `planes` in grid.y
static dim3 pair_grid(const DevArgs& d, unsigned planes = 1) {
    return dim3((unsigned)((d.n_tiles + 7) / 8 * 8) * (unsigned)d.R, planes);
}

// A kernel launched with more than 64 KB of dynamic LDS has its limit raised first
static int raise_lds_limit(const void* fn, size_t lds) {
    if (lds > 65536) HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return 0;
}

// What every simulator does once its arguments are checked: the seed, draw `draw` as bean_hip_elbo_grad(seed, step =
// draw) prepares it (no loss slot is cleared: n = 0), then one launch of `planes` member planes with `lds` bytes of
// dynamic LDS per wave.  `launch(fam, acc, grid, lds, sa)` names the kernel and its further argument struct.
template <typename Launch>
static int simulate_run(bean_hip_ctx* c, uint64_t seed, uint64_t draw, unsigned planes, void* x_out, void* xbc_out,
                        void* alpha_out, hipStream_t stream, size_t lds, Launch&& launch) {
    c->d.seed = seed;
    c->resume_ok = false;  // the workspace now holds this draw and its tables
    launch_set_step(c, stream, draw, 0, 0);
    launch_param<false, false, true>(c, stream);
    const DevArgs& d = c->d;
    SimArgs sa;
    sa.x_out = (float*)x_out;
    sa.xbc_out = (float*)xbc_out;
    sa.alpha_out = (double*)alpha_out;
    const dim3 grid = pair_grid(d, planes);
    with_family_acc(d, [&](auto fam, auto acc) { launch(fam, acc, grid, lds, sa); });
    HIP_OK(hipGetLastError());
    return 0;
}

// The D values of a study (`what`: "depths" / "effects") with n_draws screens each: D x K members at most, every value
// passing `ok` (`bad` ends the refusal of one that does not).  They are copied into the 64 slots of the launch's
// argument struct, the rest set to `pad`: the caller's array is not read after the call returns.
static int study_values(const std::string& name, const std::string& what, bool (*ok)(double), const char* bad,
                        const double* v, int32_t n_v, int32_t n_draws, double pad, double* slots) {
    if (!v) return fail(name + ": " + what + " is null");
    if (n_v < 1 || n_draws < 1 || (int64_t)n_v * n_draws > BEAN_HIP_MAX_MEMBERS)
        return fail(name + ": n_" + what + " >= 1, n_draws >= 1 and n_" + what + " * n_draws <= " +
                    std::to_string(BEAN_HIP_MAX_MEMBERS) + ", got " + std::to_string(n_v) + " x " +
                    std::to_string(n_draws) + " = " + std::to_string((int64_t)n_v * n_draws));
    for (int i = 0; i < n_v; ++i)
        if (!ok(v[i])) return fail(name + ": " + what + "[" + std::to_string(i) + "] = " + std::to_string(v[i]) + bad);
    for (int i = 0; i < kEnsembleMaxMembers; ++i) slots[i] = i < n_v ? v[i] : pad;
    return 0;
}

static const char* const kSimStem = "the count simulator does not take this handle";

extern "C" int bean_hip_simulate(bean_hip_ctx* c, uint64_t seed, uint64_t draw, void* x_out, uint64_t x_bytes,
                                 void* xbc_out, uint64_t xbc_bytes, void* alpha_out, uint64_t alpha_bytes,
                                 void* stream_) {
    const std::string name = "bean_hip_simulate";
    if (postfit_admit(c, name, kSimStem)) return -1;
    if (check_bound(c, false, false)) return -1;
    if (sim_buffers(c, name, "(R, B, G) float32", 1, x_out, x_bytes, xbc_out, xbc_bytes)) return -1;
    if (buf_optional(name, "alpha_out", "(2, R, B, G) float64", alpha_out, alpha_bytes,
                     16 * (uint64_t)c->d.R * c->d.B * c->d.G))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    return simulate_run(c, seed, draw, 1, x_out, xbc_out, alpha_out, stream, simulate_wave2_lds(c->d.B),
                        [&](auto fam, auto acc, dim3 grid, size_t lds, const SimArgs& sa) {
                            hipLaunchKernelGGL((k_simulate_wave2<fam(), acc()>), grid, dim3(64), lds, stream, c->d, sa);
                        });
}

// K replicate screens in one launch (k_simulate_members: a parametric bootstrap's screens, member-major - what
// bean_hip_bind_member_counts binds).  The target / guide sites are those of draw first_draw, member k's pi, Dirichlet
// and categorical draws those of draw first_draw + k.
extern "C" int bean_hip_simulate_members(bean_hip_ctx* c, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                         void* x_out, uint64_t x_bytes, void* xbc_out, uint64_t xbc_bytes,
                                         void* stream_) {
    const std::string name = "bean_hip_simulate_members";
    if (postfit_admit(c, name, kSimStem)) return -1;
    if (n_draws < 1 || n_draws > BEAN_HIP_MAX_MEMBERS)
        return fail(name + ": n_draws must be in [1, " + std::to_string(BEAN_HIP_MAX_MEMBERS) + "], got " +
                    std::to_string(n_draws));
    if (check_bound(c, false, false)) return -1;
    if (sim_buffers(c, name, "(K, R, B, G) float32 with K = " + std::to_string(n_draws), (uint64_t)n_draws, x_out,
                    x_bytes, xbc_out, xbc_bytes))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    return simulate_run(c, seed, first_draw, (unsigned)n_draws, x_out, xbc_out, nullptr, stream, simulate_wave2_lds(c->d.B),
                        [&](auto fam, auto acc, dim3 grid, size_t lds, const SimArgs& sa) {
                            hipLaunchKernelGGL((k_simulate_members<fam(), acc()>), grid, dim3(64), lds, stream, c->d, sa);
                        });
}

// K replicate screens at each of D read depths in one launch (k_simulate_design: a depth study's screens, (D, K)
// member-major - D * K members of bean_hip_bind_member_counts).  Everything of member (i, j) but its totals is member j
// of bean_hip_simulate_members(seed, first_draw, K); its pairs draw floor(depths[i] * n_obs + 0.5) reads.
extern "C" int bean_hip_simulate_design(bean_hip_ctx* c, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                        const double* depths, int32_t n_depths, void* x_out, uint64_t x_bytes,
                                        void* xbc_out, uint64_t xbc_bytes, void* stream_) {
    const std::string name = "bean_hip_simulate_design";
    if (postfit_admit(c, name, kSimStem)) return -1;
    DesignArgs dz;
    dz.K = n_draws;
    dz.D = n_depths;
    if (study_values(name, "depths", [](double v) { return v > 0.0 && v <= 1.7976931348623157e308; },
                     " is not a finite factor > 0", depths, n_depths, n_draws, 1.0, dz.depth))
        return -1;
    if (check_bound(c, false, false)) return -1;
    const uint64_t planes = (uint64_t)n_depths * n_draws;
    if (sim_buffers(c, name, "(D, K, R, B, G) float32 with D = " + std::to_string(n_depths) + ", K = " +
                    std::to_string(n_draws), planes, x_out, x_bytes, xbc_out, xbc_bytes))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    return simulate_run(c, seed, first_draw, (unsigned)planes, x_out, xbc_out, nullptr, stream, simulate_wave2_lds(c->d.B),
                        [&](auto fam, auto acc, dim3 grid, size_t lds, const SimArgs& sa) {
                            hipLaunchKernelGGL((k_simulate_design<fam(), acc()>), grid, dim3(64), lds, stream, c->d, sa,
                                               dz);
                        });
}

// K replicate screens at each of D planted effects in one launch (k_simulate_power: a power study's screens, (D, K)
// member-major - D * K members of bean_hip_bind_member_counts).  Everything of member (i, j) is member j of
// bean_hip_simulate_members(seed, first_draw, K) but the table entries of the planted targets, which its lanes form at
// mu = effects[i].  `plant` is the caller's device array and is read by the kernel.
extern "C" int bean_hip_simulate_power(bean_hip_ctx* c, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                       const double* effects, int32_t n_effects, const void* plant, void* x_out,
                                       uint64_t x_bytes, void* xbc_out, uint64_t xbc_bytes, void* stream_) {
    const std::string name = "bean_hip_simulate_power";
    if (postfit_admit(c, name, kSimStem)) return -1;
    PowerArgs pw;
    pw.K = n_draws;
    pw.D = n_effects;
    pw.plant = (const uint8_t*)plant;
    if (study_values(name, "effects", [](double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; },
                     " is not a finite number", effects, n_effects, n_draws, 0.0, pw.effect))
        return -1;
    if (check_bound(c, false, false)) return -1;
    const uint64_t planes = (uint64_t)n_effects * n_draws;
    if (sim_buffers(c, name, "(D, K, R, B, G) float32 with D = " + std::to_string(n_effects) + ", K = " +
                    std::to_string(n_draws), planes, x_out, x_bytes, xbc_out, xbc_bytes))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    return simulate_run(c, seed, first_draw, (unsigned)planes, x_out, xbc_out, nullptr, stream, simulate_wave2_lds(c->d.B),
                        [&](auto fam, auto acc, dim3 grid, size_t lds, const SimArgs& sa) {
                            hipLaunchKernelGGL((k_simulate_power<fam(), acc()>), grid, dim3(64), lds, stream, c->d, sa,
                                               pw);
                        });
}

static const char* const kSurvSimStem = "the survival count simulator does not take this handle";

// One replicate screen of a survival fit (k_simulate_survival): the signature and buffer rules of bean_hip_simulate,
// simulate_run's launches over the (tile, replicate) waves of k_guide_survival_wave's grid.
extern "C" int bean_hip_simulate_survival(bean_hip_ctx* c, uint64_t seed, uint64_t draw, void* x_out, uint64_t x_bytes,
                                          void* xbc_out, uint64_t xbc_bytes, void* alpha_out, uint64_t alpha_bytes,
                                          void* stream_) {
    const std::string name = "bean_hip_simulate_survival";
    if (postfit_admit(c, name, kSurvSimStem, survival_predictive_shape_ok, kSurvivalHandles)) return -1;
    if (check_bound(c, false, false)) return -1;
    if (sim_buffers(c, name, "(R, B, G) float32", 1, x_out, x_bytes, xbc_out, xbc_bytes)) return -1;
    if (buf_optional(name, "alpha_out", "(2, R, B, G) float64", alpha_out, alpha_bytes,
                     16 * (uint64_t)c->d.R * c->d.B * c->d.G))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t lds = simulate_survival_lds(c->d.B);  // beyond 35 timepoints: more than 64 KB
    if (raise_lds_limit(with_family_acc(c->d, [](auto fam, auto acc) { return (const void*)k_simulate_survival<fam(), acc()>; }),
                        lds))
        return -1;
    return simulate_run(c, seed, draw, 1, x_out, xbc_out, alpha_out, stream, lds,
                        [&](auto fam, auto acc, dim3 grid, size_t lds, const SimArgs& sa) {
                            hipLaunchKernelGGL((k_simulate_survival<fam(), acc()>), grid, dim3(64), lds, stream, c->d, sa);
                        });
}

// K replicate screens of a survival fit in one launch (k_simulate_survival_members: the screens of a survival screen's
// parametric bootstrap, (K, R, B, G) member-major).  The buffer rules and error contract of bean_hip_simulate_members,
// the admission of bean_hip_simulate_survival.  mu_t, lpn and gam / gsum are those of draw first_draw (or injected) for
// every member; member k's baseline u_g (unless eps_u is injected), pi, Dirichlet and categorical draws are those of
// draw first_draw + k.  No graph; no parameter, moment, gradient, loss_hist entry or loss accumulator is written, and
// the resume is cleared.
extern "C" int bean_hip_simulate_survival_members(bean_hip_ctx* c, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                                  void* x_out, uint64_t x_bytes, void* xbc_out, uint64_t xbc_bytes,
                                                  void* stream_) {
    const std::string name = "bean_hip_simulate_survival_members";
    if (postfit_admit(c, name, kSurvSimStem, survival_predictive_shape_ok, kSurvivalHandles)) return -1;
    if (n_draws < 1 || n_draws > BEAN_HIP_MAX_MEMBERS)
        return fail(name + ": n_draws must be in [1, " + std::to_string(BEAN_HIP_MAX_MEMBERS) + "], got " +
                    std::to_string(n_draws));
    if (check_bound(c, false, false)) return -1;
    if (sim_buffers(c, name, "(K, R, B, G) float32 with K = " + std::to_string(n_draws), (uint64_t)n_draws, x_out,
                    x_bytes, xbc_out, xbc_bytes))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t lds = simulate_survival_lds(c->d.B);
    if (raise_lds_limit(with_family_acc(c->d, [](auto fam, auto acc) { return (const void*)k_simulate_survival_members<fam(), acc()>; }),
                        lds))
        return -1;
    return simulate_run(c, seed, first_draw, (unsigned)n_draws, x_out, xbc_out, nullptr, stream, lds,
                        [&](auto fam, auto acc, dim3 grid, size_t lds, const SimArgs& sa) {
                            hipLaunchKernelGGL((k_simulate_survival_members<fam(), acc()>), grid, dim3(64), lds, stream,
                                               c->d, sa);
                        });
}

// ------------------------------------------------------------------ per-target log importance weights
// (bean_importance.hpp)
// log p(x, z) - log q(z) of draws first_draw .. first_draw + n_draws - 1 of the fitted guide, per target: draw d is the
// draw bean_hip_elbo_grad(seed, step = d) evaluates, formed by the lanes themselves - three launches per call whatever
// n_draws (the pairs' data-only constants, the pairs, the targets), no k_set_step, no PREP launch, nothing of the
// workspace written.
//
// ... with pi integrated out of the model (`marginal`, bean_importance_marg.hpp): logw_marg of the same draws, the
// weight of (mu_t, sd_t) alone.  MixtureNormal: four launches per call whatever n_draws (the pairs' constants, the
// unresolved pairs per target, the pairs' integrals, the targets); Normal has no pi: exactly the launches of
// bean_hip_log_weights and unresolved_out zeroed.
static LogwArgs logw_args(uint64_t first_draw, int n_draws, void* logw_out, void* mu_out, void* y_out, void* pair_out) {
    LogwArgs la;
    la.first_draw = first_draw;
    la.n_draws = n_draws;
    la.logw_out = (double*)logw_out;
    la.mu_out = (double*)mu_out;
    la.y_out = (double*)y_out;
    la.pair_out = (double*)pair_out;
    return la;
}

static MargArgs marg_args(int32_t n_nodes, void* unresolved_out) {
    MargArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.n_nodes = n_nodes;
    ma.unresolved_out = (int*)unresolved_out;
    gauss_hermite_half(n_nodes, ma.x, ma.lw);
    return ma;
}

// ... and with `tail` (bean_hip_log_weights_marginal_tail, bean_importance_tail.hpp) the pairs the predicate leaves out
// get bean_jacobi.hpp's Gauss-Jacobi rule per draw.  MixtureNormal: the unresolved count comes first, with its scan and
// - one host synchronisation per call - the number of tail pairs; with tail pairs k_tail_list and k_tail_nodes follow;
// then k_logw_consts and k_logw_pairs_marg as they are, k_logw_pairs_marg_tail over the tail pairs' slots,
// k_logw_targets_marg as it is, and k_grid_targets_tail with N = n_draws.  With no tail pair, and for Normal, the
// launches are those of bean_hip_log_weights_marginal and tail_err_out is zeroed.  (The tail helpers are defined with
// the grid posterior below.)
static int tail_reserve(bean_hip_ctx* c, uint64_t bytes);
static int tail_count(bean_hip_ctx* c, int* unresolved, TailArgs& ta, hipStream_t stream);
static void tail_nodes_launch(const DevArgs& d, const TailArgs& ta, hipStream_t stream);

static int logw_run(bean_hip_ctx* c, const std::string& name, bool marginal, bool tail, uint64_t seed,
                    uint64_t first_draw, int32_t n_draws, int32_t n_nodes, void* logw_out, uint64_t logw_bytes,
                    void* mu_out, uint64_t mu_bytes, void* y_out, uint64_t y_bytes, void* pair_out, uint64_t pair_bytes,
                    void* unresolved_out, uint64_t unresolved_bytes, void* tail_err_out, uint64_t tail_err_bytes,
                    void* stream_) {
    if (postfit_admit(c, name, "the importance weights do not take this handle")) return -1;
    if (n_draws < 1 || n_draws > BEAN_HIP_MAX_LOGW_DRAWS)
        return fail(name + ": n_draws must be in [1, " + std::to_string(BEAN_HIP_MAX_LOGW_DRAWS) + "], got " +
                    std::to_string(n_draws));
    if (marginal && n_nodes != 16 && n_nodes != 32 && n_nodes != 64)
        return fail(name + ": n_nodes must be 16, 32 or 64, got " + std::to_string(n_nodes));
    if (check_bound(c, false, false)) return -1;
    if (logw_buffers(c, name, n_draws, logw_out, logw_bytes, mu_out, mu_bytes, y_out, y_bytes, pair_out, pair_bytes))
        return -1;
    if (marginal && buf_exact(name, "unresolved_out", "(T) int32", unresolved_out, unresolved_bytes, 4 * (uint64_t)c->d.T))
        return -1;
    if (tail && buf_exact(name, "tail_err_out", "(n_draws, T) float64 with n_draws = " + std::to_string(n_draws),
                          tail_err_out, tail_err_bytes, 8 * (uint64_t)n_draws * c->d.T))
        return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const bool integrate = marginal && c->d.family == kMixture;
    TailArgs ta;
    memset(&ta, 0, sizeof(ta));
    if (tail && integrate) {
        if (tail_count(c, (int*)unresolved_out, ta, stream)) return -1;
        if (ta.n_tail > 0) {
            const uint64_t n = (uint64_t)ta.n_tail, need = n * (kTailPairBytes + 8 * (uint64_t)n_draws);
            if (need > kTailMaxBytes)
                return fail(name + ": " + std::to_string(ta.n_tail) + " tail pairs at n_draws = " +
                            std::to_string(n_draws) + " need a workspace of " + std::to_string(need) + " bytes (" +
                            std::to_string(kTailPairBytes) + " + 8 n_draws per pair), above the cap of " +
                            std::to_string(kTailMaxBytes) + "; send fewer draws per call");
            if (logw_tail_lds(c->d.R, c->d.B) > 65536)
                return fail(name + ": " + std::to_string(ta.n_tail) + " tail pairs, and k_logw_pairs_marg_tail needs " +
                            std::to_string(logw_tail_lds(c->d.R, c->d.B)) + " bytes of LDS at R = " +
                            std::to_string(c->d.R) + ", B = " + std::to_string(c->d.B) + ", above 65536");
            if (tail_reserve(c, need)) return -1;
            ta.N = n_draws;
            ta.z = (double*)c->tail_ws;
            ta.lw = ta.z + n * kTailAll;
            ta.pair_err = ta.lw + n * kTailAll;
            ta.pair = (int*)(ta.pair_err + n * (uint64_t)n_draws);
            ta.side = ta.pair + n;
            ta.tail_err_out = (double*)tail_err_out;
            HIP_OK(hipMemsetAsync(ta.pair, 0, 2 * n * sizeof(int), stream));  // (an entry never names a pair out of range)
            tail_nodes_launch(c->d, ta, stream);
        }
    }
    // no pi to integrate out: the joint weights are the marginal ones, and no pair is unresolved
    if (marginal && !integrate) HIP_OK(hipMemsetAsync(unresolved_out, 0, unresolved_bytes, stream));
    c->d.seed = seed;
    c->resume_ok = false;  // (the seed of the handle has changed)
    const DevArgs& d = c->d;
    const LogwArgs la = logw_args(first_draw, n_draws, logw_out, mu_out, y_out, pair_out);
    const dim3 grid = pair_grid(d, (unsigned)n_draws), block(64);
    const uint64_t nt = (uint64_t)n_draws * d.T;
    hipLaunchKernelGGL(k_logw_consts, logw_blocks((uint64_t)d.R * d.G), dim3(kLogwBlock), 0, stream, d, la);
    if (!integrate) {
        const size_t lds = simulate_wave2_lds(d.B);
        with_family_acc(d, [&](auto fam, auto acc) {
            hipLaunchKernelGGL((k_logw_pairs<fam(), acc()>), grid, block, lds, stream, d, la);
        });
        hipLaunchKernelGGL(k_logw_targets, logw_blocks(nt), dim3(kLogwBlock), 0, stream, d, la);
    } else {
        const MargArgs ma = marg_args(n_nodes, unresolved_out);
        const size_t lds = logw_marg_lds(d.B);
        // (with `tail` the count is tail_count's, already in unresolved_out)
        if (!tail) hipLaunchKernelGGL(k_logw_unresolved, logw_blocks(d.T), dim3(kLogwBlock), 0, stream, d, ma);
        if (d.flags & kAcc) hipLaunchKernelGGL(k_logw_pairs_marg<true>, grid, block, lds, stream, d, la, ma);
        else hipLaunchKernelGGL(k_logw_pairs_marg<false>, grid, block, lds, stream, d, la, ma);
        if (ta.n_tail > 0) {
            const dim3 tgrid((unsigned)(((uint64_t)ta.n_tail * n_draws + 63) / 64));
            const size_t tlds = logw_tail_lds(d.R, d.B);
            if (d.flags & kAcc) hipLaunchKernelGGL(k_logw_pairs_marg_tail<true>, tgrid, block, tlds, stream, d, la, ta);
            else hipLaunchKernelGGL(k_logw_pairs_marg_tail<false>, tgrid, block, tlds, stream, d, la, ta);
        }
        hipLaunchKernelGGL(k_logw_targets_marg, logw_blocks(nt), dim3(kLogwBlock), 0, stream, d, la);
    }
    if (tail) {
        if (ta.n_tail > 0) hipLaunchKernelGGL(k_grid_targets_tail, logw_blocks(nt), dim3(kLogwBlock), 0, stream, d, ta);
        else HIP_OK(hipMemsetAsync(tail_err_out, 0, tail_err_bytes, stream));
    }
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bean_hip_log_weights(bean_hip_ctx* c, uint64_t seed, uint64_t first_draw, int32_t n_draws, void* logw_out,
                                    uint64_t logw_bytes, void* mu_out, uint64_t mu_bytes, void* y_out, uint64_t y_bytes,
                                    void* pair_out, uint64_t pair_bytes, void* stream_) {
    return logw_run(c, "bean_hip_log_weights", false, false, seed, first_draw, n_draws, 0, logw_out, logw_bytes, mu_out,
                    mu_bytes, y_out, y_bytes, pair_out, pair_bytes, nullptr, 0, nullptr, 0, stream_);
}

extern "C" int bean_hip_log_weights_marginal(bean_hip_ctx* c, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                             int32_t n_nodes, void* logw_out, uint64_t logw_bytes, void* mu_out,
                                             uint64_t mu_bytes, void* y_out, uint64_t y_bytes, void* pair_out,
                                             uint64_t pair_bytes, void* unresolved_out, uint64_t unresolved_bytes,
                                             void* stream_) {
    return logw_run(c, "bean_hip_log_weights_marginal", true, false, seed, first_draw, n_draws, n_nodes, logw_out,
                    logw_bytes, mu_out, mu_bytes, y_out, y_bytes, pair_out, pair_bytes, unresolved_out, unresolved_bytes,
                    nullptr, 0, stream_);
}

extern "C" int bean_hip_log_weights_marginal_tail(bean_hip_ctx* c, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                                  int32_t n_nodes, void* logw_out, uint64_t logw_bytes, void* mu_out,
                                                  uint64_t mu_bytes, void* y_out, uint64_t y_bytes, void* pair_out,
                                                  uint64_t pair_bytes, void* unresolved_out, uint64_t unresolved_bytes,
                                                  void* tail_err_out, uint64_t tail_err_bytes, void* stream_) {
    return logw_run(c, "bean_hip_log_weights_marginal_tail", true, true, seed, first_draw, n_draws, n_nodes, logw_out,
                    logw_bytes, mu_out, mu_bytes, y_out, y_bytes, pair_out, pair_bytes, unresolved_out, unresolved_bytes,
                    tail_err_out, tail_err_bytes, stream_);
}

// ------------------------------------------------------------------ the log joint on a grid of (mu, y) per target
// (bean_grid.hpp) lj of n_mu * n_y given nodes per target, pi integrated out: four launches per call whatever the grid
// (the pairs' constants, the unresolved pairs per target, the pairs' terms, the targets).  No seed, no draw, no term of
// q; nothing of the handle is written.
//
// With tail_err_out (bean_hip_marginal_grid_tail, bean_jacobi.hpp) the pairs the predicate leaves out get a Gauss-Jacobi
// rule: the unresolved count comes first, its scan gives the compact list's offsets and - one host synchronisation per
// call - the number of tail pairs; with none, the launches are those of bean_hip_marginal_grid and tail_err_out is
// zeroed; otherwise k_tail_list and k_tail_nodes follow, then k_logw_consts and k_grid_pairs as they are,
// k_grid_pairs_tail over the tail pairs' slots, k_grid_targets as it is, and k_grid_targets_tail.
static int tail_reserve(bean_hip_ctx* c, uint64_t bytes) {
    if (!c->tail_off) HIP_OK(hipMalloc((void**)&c->tail_off, sizeof(int) * (2 * (size_t)c->d.T + 1)));
    if (bytes > c->tail_ws_bytes) {
        if (c->tail_ws) (void)hipFree(c->tail_ws);
        c->tail_ws = nullptr;
        c->tail_ws_bytes = 0;
        HIP_OK(hipMalloc(&c->tail_ws, bytes));
        c->tail_ws_bytes = bytes;
    }
    return 0;
}

// the unresolved count (into `unresolved`, (T) int32 on the device; null: the T slots the handle keeps behind its
// offsets), its scan, and the number of tail pairs on the host
static int tail_count(bean_hip_ctx* c, int* unresolved, TailArgs& ta, hipStream_t stream) {
    const DevArgs& d = c->d;
    if (tail_reserve(c, 0)) return -1;
    if (!unresolved) unresolved = c->tail_off + d.T + 1;  // (there only once tail_reserve has run)
    MargArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.unresolved_out = unresolved;
    hipLaunchKernelGGL(k_logw_unresolved, logw_blocks(d.T), dim3(kLogwBlock), 0, stream, d, ma);
    memset(&ta, 0, sizeof(ta));
    ta.unresolved = unresolved;
    ta.toff = c->tail_off;
    hipLaunchKernelGGL(k_tail_offsets, dim3(1), dim3(kTailScanBlock), 0, stream, d.T, ta);
    int n = 0;
    HIP_OK(hipMemcpyAsync(&n, c->tail_off + d.T, sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    ta.n_tail = n;
    return 0;
}

// the compact list and the 64 + 48 nodes and log weights of every tail pair, into ta's arrays
static void tail_nodes_launch(const DevArgs& d, const TailArgs& ta, hipStream_t stream) {
    hipLaunchKernelGGL(k_tail_list, logw_blocks(d.T), dim3(kLogwBlock), 0, stream, d, ta);
    hipLaunchKernelGGL(k_tail_nodes, logw_blocks((uint64_t)ta.n_tail * kTailAll), dim3(kLogwBlock), 0, stream, d, ta);
}

static int grid_run(bean_hip_ctx* c, const std::string& name, bool tail, int32_t n_nodes, int32_t n_mu, int32_t n_y,
                    const void* centre_mu, const void* centre_y, const void* step_mu, const void* step_y, void* lj_out,
                    uint64_t lj_bytes, void* pair_out, uint64_t pair_bytes, void* unresolved_out,
                    uint64_t unresolved_bytes, void* tail_err_out, uint64_t tail_err_bytes, void* stream_) {
    if (grid_admit(c, name)) return -1;
    if (n_nodes != 16 && n_nodes != 32 && n_nodes != 64)
        return fail(name + ": n_nodes must be 16, 32 or 64, got " + std::to_string(n_nodes));
    if (n_mu < 1 || n_y < 1 || (int64_t)n_mu * n_y > BEAN_HIP_MAX_LOGW_DRAWS)
        return fail(name + ": n_mu >= 1, n_y >= 1 and n_mu * n_y <= " +
                    std::to_string(BEAN_HIP_MAX_LOGW_DRAWS) + ", got " + std::to_string(n_mu) + " x " +
                    std::to_string(n_y) + " = " + std::to_string((int64_t)n_mu * n_y));
    if (check_bound(c, false, false)) return -1;
    const DevArgs& d = c->d;
    const int N = n_mu * n_y;
    const uint64_t nt = (uint64_t)N * d.T, np = (uint64_t)N * d.R * d.G;
    if (!centre_mu || !centre_y || !step_mu || !step_y)
        return fail(name + ": centre_mu, centre_y, step_mu and step_y must each hold (T) float64 on the "
                    "device; one of them is null");
    const std::string of = " float64 with N = n_mu * n_y = " + std::to_string(N);
    if (buf_exact(name, "lj_out", "(N, T)" + of, lj_out, lj_bytes, 8 * nt)) return -1;
    if (buf_exact(name, "pair_out (caller-owned scratch)", "(N, R, G)" + of, pair_out, pair_bytes, 8 * np)) return -1;
    if (buf_exact(name, "unresolved_out", "(T) int32 (N = " + std::to_string(N) + ")", unresolved_out, unresolved_bytes,
                  4 * (uint64_t)d.T))
        return -1;
    if (tail && buf_exact(name, "tail_err_out", "(N, T)" + of, tail_err_out, tail_err_bytes, 8 * nt)) return -1;
    hipStream_t stream = (hipStream_t)stream_;
    const LogwArgs la = logw_args(0, N, nullptr, nullptr, nullptr, pair_out);
    GridArgs ga;
    ga.n_mu = n_mu;
    ga.n_y = n_y;
    ga.centre_mu = (const double*)centre_mu;
    ga.centre_y = (const double*)centre_y;
    ga.step_mu = (const double*)step_mu;
    ga.step_y = (const double*)step_y;
    ga.lj_out = (double*)lj_out;
    ga.pair_out = (double*)pair_out;
    const MargArgs ma = marg_args(n_nodes, unresolved_out);
    const dim3 grid = pair_grid(d, (unsigned)((N + kGridChunk - 1) / kGridChunk)), block(64);
    const size_t lds = logw_marg_lds(d.B);
    TailArgs ta;
    memset(&ta, 0, sizeof(ta));
    if (tail && d.family == kMixture) {
        if (tail_count(c, (int*)unresolved_out, ta, stream)) return -1;
        if (ta.n_tail > 0) {
            const uint64_t n = (uint64_t)ta.n_tail, need = n * (kTailPairBytes + 8 * (uint64_t)N);
            if (need > kTailMaxBytes)
                return fail(name + ": " + std::to_string(ta.n_tail) + " tail pairs at N = " + std::to_string(N) +
                            " grid nodes need a workspace of " + std::to_string(need) + " bytes (" +
                            std::to_string(kTailPairBytes) + " + 8 N per pair), above the cap of " +
                            std::to_string(kTailMaxBytes) + "; send fewer nodes per call");
            if (logw_tail_lds(d.R, d.B) > 65536)
                return fail(name + ": " + std::to_string(ta.n_tail) + " tail pairs, and k_grid_pairs_tail needs " +
                            std::to_string(logw_tail_lds(d.R, d.B)) + " bytes of LDS at R = " + std::to_string(d.R) +
                            ", B = " + std::to_string(d.B) + ", above 65536");
            if (tail_reserve(c, need)) return -1;
            ta.N = N;
            ta.z = (double*)c->tail_ws;
            ta.lw = ta.z + n * kTailAll;
            ta.pair_err = ta.lw + n * kTailAll;
            ta.pair = (int*)(ta.pair_err + n * (uint64_t)N);
            ta.side = ta.pair + n;
            ta.tail_err_out = (double*)tail_err_out;
            HIP_OK(hipMemsetAsync(ta.pair, 0, 2 * n * sizeof(int), stream));  // (an entry never names a pair out of range)
            tail_nodes_launch(d, ta, stream);
        }
    }
    hipLaunchKernelGGL(k_logw_consts, logw_blocks((uint64_t)d.R * d.G), dim3(kLogwBlock), 0, stream, d, la);
    if (d.family == kMixture) {
        if (!tail) hipLaunchKernelGGL(k_logw_unresolved, logw_blocks(d.T), dim3(kLogwBlock), 0, stream, d, ma);
        hipLaunchKernelGGL(k_grid_pairs<kMixture>, grid, block, lds, stream, d, ga, ma);
        if (ta.n_tail > 0)
            hipLaunchKernelGGL(k_grid_pairs_tail, dim3((unsigned)((ta.n_tail + 63) / 64),
                                                       (unsigned)((N + kTailChunk - 1) / kTailChunk)),
                               block, logw_tail_lds(d.R, d.B), stream, d, ga, ta);
    } else {
        // no pi to integrate out, and no pair is unresolved
        HIP_OK(hipMemsetAsync(unresolved_out, 0, unresolved_bytes, stream));
        hipLaunchKernelGGL(k_grid_pairs<kNormal>, grid, block, lds, stream, d, ga, ma);
    }
    hipLaunchKernelGGL(k_grid_targets, logw_blocks(nt), dim3(kLogwBlock), 0, stream, d, ga);
    if (tail) {
        if (ta.n_tail > 0) hipLaunchKernelGGL(k_grid_targets_tail, logw_blocks(nt), dim3(kLogwBlock), 0, stream, d, ta);
        else HIP_OK(hipMemsetAsync(tail_err_out, 0, tail_err_bytes, stream));
    }
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int bean_hip_marginal_grid(bean_hip_ctx* c, int32_t n_nodes, int32_t n_mu, int32_t n_y, const void* centre_mu,
                                      const void* centre_y, const void* step_mu, const void* step_y, void* lj_out,
                                      uint64_t lj_bytes, void* pair_out, uint64_t pair_bytes, void* unresolved_out,
                                      uint64_t unresolved_bytes, void* stream_) {
    return grid_run(c, "bean_hip_marginal_grid", false, n_nodes, n_mu, n_y, centre_mu, centre_y, step_mu, step_y, lj_out,
                    lj_bytes, pair_out, pair_bytes, unresolved_out, unresolved_bytes, nullptr, 0, stream_);
}

extern "C" int bean_hip_marginal_grid_tail(bean_hip_ctx* c, int32_t n_nodes, int32_t n_mu, int32_t n_y,
                                           const void* centre_mu, const void* centre_y, const void* step_mu,
                                           const void* step_y, void* lj_out, uint64_t lj_bytes, void* pair_out,
                                           uint64_t pair_bytes, void* unresolved_out, uint64_t unresolved_bytes,
                                           void* tail_err_out, uint64_t tail_err_bytes, void* stream_) {
    return grid_run(c, "bean_hip_marginal_grid_tail", true, n_nodes, n_mu, n_y, centre_mu, centre_y, step_mu, step_y,
                    lj_out, lj_bytes, pair_out, pair_bytes, unresolved_out, unresolved_bytes, tail_err_out, tail_err_bytes,
                    stream_);
}

// the compact list of tail pairs with its nodes, for the tests: *n_tail_out (host) is the number of tail pairs; with
// capacity = 0 nothing else is written (the count query); otherwise capacity >= that number and the first n_tail
// entries of pair_index_out (int32, r * G + g in the handle's guide order), z_out and lw_out ((capacity, 112) float64:
// the 64 nodes ascending, then the 48) and side_out (int32) are written
extern "C" int bean_hip_marginal_tail_nodes(bean_hip_ctx* c, int32_t capacity, void* pair_index_out, void* z_out,
                                            void* lw_out, void* side_out, int32_t* n_tail_out, void* stream_) {
    const std::string name = "bean_hip_marginal_tail_nodes";
    if (grid_admit(c, name)) return -1;
    if (!n_tail_out) return fail(name + ": n_tail_out is null");
    if (capacity < 0) return fail(name + ": capacity must not be negative, got " + std::to_string(capacity));
    if (capacity > 0 && (!pair_index_out || !z_out || !lw_out || !side_out))
        return fail(name + ": with capacity > 0, pair_index_out, z_out, lw_out and side_out must not be null");
    if (check_bound(c, false, false)) return -1;
    const DevArgs& d = c->d;
    *n_tail_out = 0;
    if (d.family != kMixture) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    TailArgs ta;
    if (tail_count(c, nullptr, ta, stream)) return -1;
    *n_tail_out = ta.n_tail;
    if (capacity == 0 || ta.n_tail == 0) return 0;
    if (capacity < ta.n_tail)
        return fail(name + ": capacity " + std::to_string(capacity) + " is below the " + std::to_string(ta.n_tail) +
                    " tail pairs of the handle");
    ta.pair = (int*)pair_index_out;
    ta.side = (int*)side_out;
    ta.z = (double*)z_out;
    ta.lw = (double*)lw_out;
    HIP_OK(hipMemsetAsync(ta.pair, 0, (size_t)ta.n_tail * sizeof(int), stream));
    tail_nodes_launch(d, ta, stream);
    HIP_OK(hipGetLastError());
    return 0;
}
