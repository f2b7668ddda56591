/*
 * bean_hip.h - C ABI of the MI355X-native BEAN SVI step (libbean_hip.so).
 *
 * The reference has no FFI boundary for this path: the seam is the Python call
 *   run_inference(model, guide, data, initial_lr, gamma, num_steps)
 *       (bean/model/run.py:347-396)
 * which drives pyro.infer.SVI over the model/guide pairs of
 * bean/model/model.py and bean/model/survival_model.py.  This header is the
 * C-ABI a maintainer would bind (ctypes) to replace the body
 * of that loop.  Entry points and what they replace:
 *
 *   bean_hip_elbo_grad   one Trace_ELBO.loss_and_grads evaluation
 *                        (svi.step minus the optimiser; run.py:377)
 *   bean_hip_adam        pyro.optim.ClippedAdam update (run.py:371)
 *   bean_hip_svi_run     the whole "for t in range(num_steps): svi.step(data)"
 *                        loop (run.py:376-380) with the loss history kept on
 *                        the device
 *
 * Conventions
 *   - plain C: opaque handle, int status codes (0 = ok, < 0 = error; the message
 *     is available from bean_hip_last_error()); nothing throws across the ABI.
 *   - every data / parameter / optimiser-state / gradient buffer is a
 *     caller-owned DEVICE pointer bound to a slot with bean_hip_bind(); the
 *     library never frees or retains them beyond the handle's lifetime.  The
 *     handle owns only scratch workspace.
 *   - all launches go to the hipStream_t passed in (void* here so that the
 *     header needs no HIP include); no call synchronises the host unless noted.
 *   - one handle per (device, stream); calls on one handle are serialised by
 *     the caller.
 *   - random draws come from a counter-based generator keyed by
 *     (seed, site, element, step): results do not depend on grid shape or on
 *     how guides are sharded across GPUs.
 *
 * Tensor layouts (R reps, B conditions, G guides, T targets, A alleles,
 * C control conditions) follow the reference's ScreenData contract
 * (bean/preprocessing/data_class.py): counts are
 * (R, B, G) float32 with G contiguous.
 */
#ifndef BEAN_HIP_H
#define BEAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bean_hip_ctx bean_hip_ctx;

/* model families: bean/model/run.py:399-474 (identify_model_guide) */
enum bean_hip_family {
    BEAN_FAMILY_NORMAL = 0,          /* NormalModel/NormalGuide            model.py:19,754  */
    BEAN_FAMILY_CONTROL_NORMAL = 1,  /* ControlNormalModel/Guide           model.py:168,861 */
    BEAN_FAMILY_MIXTURE_NORMAL = 2,  /* MixtureNormalModel/Guide           model.py:378,785 */
    BEAN_FAMILY_MULTI_MIXTURE = 3    /* MultiMixtureNormalModel/Guide      model.py:550,878 */
};

enum bean_hip_selection { BEAN_SELECTION_SORTING = 0, BEAN_SELECTION_SURVIVAL = 1 };

enum bean_hip_flags {
    BEAN_FLAG_USE_BCMATCH = 1,     /* second DirMult site on X_bcmatch (model.py:536-547) */
    BEAN_FLAG_SCALE_BY_ACC = 2,    /* scale_pi_by_accessibility (utils.py:106-178)         */
    BEAN_FLAG_FIT_NOISE = 4,       /* guide learns noise_loc/noise_scale (utils.py:144-155) */
    BEAN_FLAG_PRIOR_NORMAL_MU = 8, /* --prior-params: Normal instead of Laplace (model.py:408-420) */
    BEAN_FLAG_DUMP_PI = 16,        /* write the Dirichlet draws to BEAN_BUF_PI_OUT (tests)  */
    BEAN_FLAG_NOT_LOSS_OWNER = 32  /* guide-sharded fit of a family with replicated per-target
                                      parameters: another rank counts their prior/entropy terms */
};

typedef struct bean_hip_shape {
    int32_t family;        /* enum bean_hip_family */
    int32_t selection;     /* enum bean_hip_selection */
    int32_t flags;         /* OR of enum bean_hip_flags */
    int32_t n_reps;        /* R */
    int32_t n_condits;     /* B: sort bins incl. the control pseudo-bin, or timepoints (<= 8 in libbean_hip.so,
                              <= 64 in libbean_hip_a16.so / _a32.so) */
    int32_t n_guides;      /* G */
    int32_t n_targets;     /* T (variant); = n_edits for tiling: the per-target parameters are per edit */
    int32_t n_max_alleles; /* A (2 in variant mode) */
    int32_t n_edits;       /* E (tiling) */
    int32_t n_ctrl;        /* C: control conditions in allele_counts_control */
    int32_t mask_thres;    /* guides with sum_b x <= mask_thres are masked (10) */
    int32_t max_target_len;/* longest target (guides); very long targets get one block each */
    /* position of this shard inside the whole screen: the random streams are
     * keyed by GLOBAL guide / target indices, so a guide-sharded multi-GPU fit
     * reproduces the single-GPU fit bit for bit */
    int32_t guide_offset;  /* index of this shard's first guide in the whole screen */
    int32_t target_offset; /* index of this shard's first target */
    int32_t n_guides_total;/* guides in the whole screen (0 = n_guides) */
    int32_t n_a2e_nnz;     /* tiling: total number of (allele, edit) pairs */
    double sd_prior_scale; /* LogNormal prior scale of sd_targets (0.01; 1.0 for ControlNormal) */
    double initial_lr;     /* ClippedAdam lr (0.01) */
    double lrd;            /* per-step lr decay gamma ** (1 / num_steps) */
    double clip_norm;      /* 10 */
    /* survival MixtureNormal: prior of the per-guide baseline growth mu_negctrl
     * (survival_model.py:225,271-274); fed from the neg-ctrl fit by bean run */
    double negctrl_loc;    /* 0.0 */
    double negctrl_scale;  /* 0.1 */
    /* sorting NormalModel with sample covariates (bean/model/model.py:73-91, 771-783): number of
     * covariates (0 = none).  The mu_cov_loc / mu_cov_scale parameters (n_sample_covariates each) use
     * the NOISE_LOC / NOISE_SCALE parameter slots and the eps draws the EPS_NOISE_IN / _OUT slots,
     * which this family does not otherwise use. */
    int32_t n_sample_covariates;
    int32_t reserved_;
    /* survival NormalModel with prior_params["initial_abundance"] (survival_model.py:38-49): sum of that
     * per-guide prior concentration over the WHOLE screen (0 = the default prior ones / G); the per-guide
     * values of this shard go in BEAN_BUF_PRIOR_IA */
    double prior_ia_total;
} bean_hip_shape;

/* Buffer slots.  dtype / shape in brackets; "opt" = only for some families. */
enum bean_hip_buf {
    /* ---- data (read-only) */
    BEAN_BUF_X = 0,           /* f32 (R,B,G)   X_masked                               */
    BEAN_BUF_X_BC,            /* f32 (R,B,G)   X_bcmatch_masked                  opt  */
    BEAN_BUF_ALLELE_CTRL,     /* f32 (R,C,G,A) allele_counts_control             opt  */
    BEAN_BUF_REPGUIDE,        /* u8  (R,G)     repguide_mask                          */
    BEAN_BUF_SIZE_FACTOR,     /* f64 (R,B)                                            */
    BEAN_BUF_SIZE_FACTOR_BC,  /* f64 (R,B)                                       opt  */
    BEAN_BUF_SAMPLE_MASK,     /* f64 (R,B)     0/1                                    */
    BEAN_BUF_A0,              /* f64 (G)                                              */
    BEAN_BUF_A0_BC,           /* f64 (G)                                         opt  */
    BEAN_BUF_PI_A0,           /* f64 (G)                                         opt  */
    BEAN_BUF_Z_HI,            /* f64 (B)  Phi^-1(upper quantile), +inf where it is 1  */
    BEAN_BUF_Z_LO,            /* f64 (B)  Phi^-1(lower quantile), -inf where it is 0  */
    BEAN_BUF_TARGET_OFFSETS,  /* i32 (T+1) exclusive prefix sum of target_lengths     */
    BEAN_BUF_GUIDE_TO_TARGET, /* i32 (G)                                              */
    BEAN_BUF_ACCESSIBILITY,   /* f64 (G)                                         opt  */
    BEAN_BUF_PRIOR_MU_LOC,    /* f64 (T)  --prior-params                         opt  */
    BEAN_BUF_PRIOR_MU_SCALE,  /* f64 (T)                                         opt  */
    BEAN_BUF_PRIOR_SD_LOC,    /* f64 (T)                                         opt  */
    BEAN_BUF_PRIOR_SD_SCALE,  /* f64 (T)                                         opt  */
    /* tiling: allele slot s = g*(A-1) + (a-1) -> its edits (CSR), and the transpose */
    BEAN_BUF_A2E_PTR,         /* i32 (G*(A-1)+1)                                 opt  */
    BEAN_BUF_A2E_IDX,         /* i32 (nnz)  edit ids                             opt  */
    BEAN_BUF_E2A_PTR,         /* i32 (E+1)                                       opt  */
    BEAN_BUF_E2A_IDX,         /* i32 (nnz)  allele slots containing the edit     opt  */
    BEAN_BUF_ALLELE_MASK,     /* u8  (G,A)  allele_mask                          opt  */
    /* survival: timepoints divided by the last one (data_class.py:1034-1053) */
    BEAN_BUF_TIMEPOINTS,      /* f64 (B)                                         opt  */
    BEAN_BUF_CONTROL_TIME,    /* f64 (C)   timepoint(s) of the control condition opt  */
    BEAN_BUF_LOG_OBS0,        /* f64 (R,G) log((X[:,0,:]+1)/sum): observed initial abundance opt */
    BEAN_BUF_NEGCTRL_MASK,    /* u8  (G)   survival NormalModel: 1 where the guide is a negative control
                                 (mu forced to 0, survival_model.py:59-60)                   opt  */
    /* exchange buffers of guide-sharded fits (bean_hip_sharded_*): the library writes this rank's
       sums, the caller all-reduces them over the ranks, the library reads the totals */
    BEAN_BUF_XCHG_GSUM,       /* f64 (R+1) survival MixtureNormal: sum_g of the Dirichlet(q0) site's gamma
                                 draws per replicate, sum_g q0                               opt  */
    BEAN_BUF_XCHG_TGRAD,      /* f64 (2,T) ControlNormal / tiling: per-target likelihood gradient opt  */
    BEAN_BUF_XCHG_SQ,         /* f64 (R)   survival NormalModel: sum_g q_0[r,g] * d loss / d q_0[r,g], the
                                 projection term of the Dirichlet-over-guides pathwise gradient opt  */
    /* ---- sorting NormalModel with sample covariates */
    BEAN_BUF_REP_BY_COV = 31, /* f64 (R, n_sample_covariates) design matrix rep_by_cov (data_class.py:83-90) opt */
    /* ---- parameters: unconstrained values as Pyro's param store keeps them */
    BEAN_BUF_P_MU_LOC = 32,   /* f32 (T)                                              */
    BEAN_BUF_P_MU_SCALE,      /* f32 (T)   log mu_scale                               */
    BEAN_BUF_P_SD_LOC,        /* f32 (T)                                              */
    BEAN_BUF_P_SD_SCALE,      /* f32 (T)   log sd_scale                               */
    BEAN_BUF_P_ALPHA_PI,      /* f32 (G,A) log alpha_pi                          opt  */
    BEAN_BUF_P_NOISE_LOC,     /* f32 (G)                                         opt  */
    BEAN_BUF_P_NOISE_SCALE,   /* f32 (G)   log noise_scale                       opt  */
    BEAN_BUF_P_Q0,            /* f32 (G)   log q0 (survival MixtureNormal)       opt  */
    /* ---- gradients w.r.t. the unconstrained parameters (bean_hip_elbo_grad) */
    BEAN_BUF_G_MU_LOC = 48,
    BEAN_BUF_G_MU_SCALE,
    BEAN_BUF_G_SD_LOC,
    BEAN_BUF_G_SD_SCALE,
    BEAN_BUF_G_ALPHA_PI,
    BEAN_BUF_G_NOISE_LOC,
    BEAN_BUF_G_NOISE_SCALE,
    BEAN_BUF_G_Q0,
    /* ---- ClippedAdam first / second moments, same shapes as the parameters */
    BEAN_BUF_M_MU_LOC = 64,
    BEAN_BUF_M_MU_SCALE,
    BEAN_BUF_M_SD_LOC,
    BEAN_BUF_M_SD_SCALE,
    BEAN_BUF_M_ALPHA_PI,
    BEAN_BUF_M_NOISE_LOC,
    BEAN_BUF_M_NOISE_SCALE,
    BEAN_BUF_M_Q0,
    BEAN_BUF_V_MU_LOC = 80,
    BEAN_BUF_V_MU_SCALE,
    BEAN_BUF_V_SD_LOC,
    BEAN_BUF_V_SD_SCALE,
    BEAN_BUF_V_ALPHA_PI,
    BEAN_BUF_V_NOISE_LOC,
    BEAN_BUF_V_NOISE_SCALE,
    BEAN_BUF_V_Q0,
    /* ---- injected / exported noise (parity tests) */
    BEAN_BUF_EPS_MU_IN = 96,  /* f64 (T)   standard-normal draws for mu_targets  opt  */
    BEAN_BUF_EPS_SD_IN,       /* f64 (T)                                         opt  */
    BEAN_BUF_PI_IN,           /* f64 (R,G,A) Dirichlet draws                     opt  */
    BEAN_BUF_EPS_NOISE_IN,    /* f64 (G)                                         opt  */
    BEAN_BUF_EPS_MU_OUT,      /* f64 (T)   draws actually used                   opt  */
    BEAN_BUF_EPS_SD_OUT,      /* f64 (T)                                         opt  */
    BEAN_BUF_PI_OUT,          /* f64 (R,G,A)                                     opt  */
    BEAN_BUF_EPS_NOISE_OUT,   /* f64 (G)                                         opt  */
    BEAN_BUF_X0_IN,           /* f64 (R,G) survival: Dirichlet(q0) draws         opt  */
    BEAN_BUF_EPS_U_IN,        /* f64 (G)   survival: mu_negctrl standard normals opt  */
    BEAN_BUF_X0_OUT,          /* f64 (R,G)                                       opt  */
    BEAN_BUF_EPS_U_OUT,       /* f64 (G)                                         opt  */
    BEAN_BUF_PRIOR_IA,        /* f64 (G)   survival NormalModel: prior concentration of the Dirichlet-over-guides
                                 site, prior_params["initial_abundance"]                      opt  */
    BEAN_BUF_XCHG_COV,        /* f64 (R)   guide-sharded sorting NormalModel with sample covariates: sum over this
                                 rank's guides of each replicate's d nll / d mu row (the likelihood gradient of
                                 the shared mu_cov site), all-reduced by the caller between
                                 bean_hip_sharded_guide and bean_hip_sharded_update                opt  */
    BEAN_BUF_GUIDE_IDS,       /* i32 (G)   tiling: each guide's index in the caller's whole screen.  The per-guide
                                 random streams (pi draws, accessibility noise) are keyed by it instead of
                                 guide_offset + position, so a caller may hand the guides over in ANOTHER ORDER
                                 - crispr-bean_amd orders them by their number of alleles, which makes the lanes
                                 of a wave take the same branches - and still draw what the screen order draws  opt  */
    /* ---- loss */
    BEAN_BUF_LOSS_HIST = 112, /* f64 (capacity) one entry per SVI step                */
    BEAN_BUF_COUNT = 128
};

const char* bean_hip_version(void);
const char* bean_hip_last_error(void);

/* Create / destroy a handle for one screen shape on the current HIP device.
 * Allocates the scratch workspace (O(G + B*T) doubles). */
int bean_hip_create(const bean_hip_shape* shape, bean_hip_ctx** out);
int bean_hip_destroy(bean_hip_ctx* ctx);

/* Bind a caller-owned device buffer to a slot; nbytes is checked against the
 * size the shape implies (a mismatch is an error, nothing is launched). */
int bean_hip_bind(bean_hip_ctx* ctx, int slot, void* device_ptr, uint64_t nbytes);

/* Validate that every slot the family needs is bound, and run the one-off
 * data-only precomputation (masks, log-factorial constants of the likelihoods;
 * tiling: the list of allele slots that hold an allele, for which the allele
 * mask and the CSR row pointers are read back to the host once).  Synchronises
 * the stream.  Must be called after the data slots are bound and before any step. */
int bean_hip_prepare(bean_hip_ctx* ctx, void* stream);

/* One ELBO evaluation with gradients: draws the step's noise (or reads the
 * *_IN slots when bound), writes d loss / d param to the BEAN_BUF_G_* slots and
 * the loss to loss_hist[loss_index].  Parameters are not modified. */
int bean_hip_elbo_grad(bean_hip_ctx* ctx, uint64_t seed, uint64_t step,
                       uint64_t loss_index, void* stream);

/* ClippedAdam update of every bound parameter from the BEAN_BUF_G_* slots;
 * t is the 1-based update count (lr_t = initial_lr * lrd ** t). */
int bean_hip_adam(bean_hip_ctx* ctx, uint64_t t, void* stream);

/* Fused SVI loop: n_steps x {draw, ELBO, gradient, ClippedAdam}, steps
 * first_step .. first_step + n_steps - 1, loss of step s written to
 * loss_hist[s].  Kernels are enqueued through a captured hipGraph of
 * graph_chunk steps when graph_chunk > 0 (eager launches when 0). */
int bean_hip_svi_run(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_step,
                     uint64_t n_steps, int32_t graph_chunk, void* stream);

/* Seed ensembles: K independent fits of the SAME screen, stepped by the same launches (the grids get a member
 * axis; the data is bound once and read by all members).  Member k is, bit for bit, the fit that
 * bean_hip_svi_run(seed = seeds[k]) produces on a handle of its own.
 *
 *   bean_hip_ensemble_supported   1 if the batched kernels take this handle's shape, 0 if not: the sorting variant
 *                                 families on the two-launches-per-step path (Normal without sample covariates,
 *                                 MixtureNormal with or without accessibility scaling / fit_noise / X_bcmatch /
 *                                 --prior-params), unsharded.  Not: tiling, survival, ControlNormal, sample
 *                                 covariates, screens large enough for the one-launch stepper, BEAN_FLAG_DUMP_PI.
 *                                 Callers fit the seeds of such a shape one after the other.  (It also governs
 *                                 bean_hip_set_particles, and stays 0 for every survival handle.)
 *   bean_hip_survival_members_supported
 *                                 1 if the survival member kernels take this handle's shape, 0
 *                                 if not: survival selection on the wave-form variant path (not
 *                                 BEAN_HIP_SURVIVAL=block), family Normal or MixtureNormal (with or without
 *                                 accessibility scaling / X_bcmatch), no sample covariates, unsharded (no guide or
 *                                 target offset, n_guides_total 0 or n_guides), neither BEAN_FLAG_NOT_LOSS_OWNER nor
 *                                 BEAN_FLAG_DUMP_PI, and at most 58 timepoints (the dynamic LDS of the single-fit launch
 *                                 as it is made: 64 KB).  bean_hip_set_members, the two member binds and
 *                                 bean_hip_svi_run_ensemble admit a handle where EITHER predicate is 1, and everything
 *                                 said below holds for such a survival handle: member k is, bit for bit,
 *                                 bean_hip_svi_run(seed = seeds[k]) on a handle of its own with member k's counts and
 *                                 masks.  bean_hip_svi_run_ensemble on a survival handle with more than one member
 *                                 refuses while BEAN_BUF_XCHG_GSUM or BEAN_BUF_XCHG_SQ is bound (the members would share
 *                                 the buffer; the message names it), and the survival draws and dumps (BEAN_BUF_X0_IN /
 *                                 _OUT, EPS_U_IN / _OUT) count as injected / dumped noise.  bean_hip_set_particles and
 *                                 bean_hip_simulate_survival* stay refused there (the latter with n_members > 1).
 *   bean_hip_set_members          after bean_hip_create, before ANY bean_hip_bind; 1 <= n_members <=
 *                                 BEAN_HIP_MAX_MEMBERS.  From then on the slots BEAN_BUF_P_*, G_*, M_*, V_* expect
 *                                 n_members times their single-fit size, member-major ((K, T), (K, G, A), ...), and
 *                                 BEAN_BUF_LOSS_HIST holds (K, capacity) doubles; bean_hip_bind checks these sizes.
 *                                 The handle allocates a private workspace per member.  The single-fit entry points
 *                                 (bean_hip_elbo_grad, bean_hip_svi_run, ...) keep working and address member 0.
 *   bean_hip_svi_run_ensemble     the loop of bean_hip_svi_run for all members: `seeds` is a HOST array of n_seeds ==
 *                                 n_members values; loss of member k, step s in loss_hist[k * capacity + s].  A call
 *                                 with first_step = the previous call's first_step + n_steps continues the fits
 *                                 (windows give the bits of one call).  Injected / dumped noise is refused.
 *
 *   bean_hip_bind_member_masks    per-member masks: the members may also differ in the two mask arrays (a replicate
 *                                 jackknife: member j is the screen with one replicate masked).  `repguide` is
 *                                 (K, R, G) uint8 and `sample_mask` (K, R, B) float64, member-major like the
 *                                 parameters, device memory the caller keeps alive; member k reads its slice where a
 *                                 single fit reads BEAN_BUF_REPGUIDE / BEAN_BUF_SAMPLE_MASK.  Those two slots stay
 *                                 bound and the single-fit entry points (which address member 0) keep reading THEM,
 *                                 while the data-only words in member 0's workspace are then those of member 0's
 *                                 slice: on a handle with member masks the single-fit entry points are only
 *                                 meaningful if member 0's slice equals the shared masks (the jackknife binds it so;
 *                                 the library does not compare the arrays).  Allowed after bean_hip_set_members and before
 *                                 bean_hip_prepare: a call marks the handle unprepared, and the following
 *                                 bean_hip_prepare computes the data-only words that depend on the repguide mask (the
 *                                 loss constant, the number of unmasked replicates per guide) once per member.
 *                                 Member k is then, bit for bit, bean_hip_svi_run on a handle of its own whose
 *                                 BEAN_BUF_REPGUIDE / BEAN_BUF_SAMPLE_MASK are member k's slices (counts, size
 *                                 factors and every other buffer as bound here).  Null for both returns the handle
 *                                 to shared masks (prepare again).  The byte counts are checked against K.
 *
 *   bean_hip_bind_member_counts   per-member counts: the members may also differ in their data (a sample jackknife:
 *                                 member j is the screen with one sorted sample masked, whose counts the reference
 *                                 zeroes - the guide kernel reads every bin's count whatever the sample mask says, so a
 *                                 masked sample is not a mask change alone; a parametric bootstrap or a downsampling
 *                                 run would bind their draws the same way).  `x` is (K, R, B, G) float32, member-major
 *                                 like the parameters, device memory the caller keeps alive; `x_bcmatch` has the same
 *                                 shape, is required exactly when the handle was created with BEAN_FLAG_USE_BCMATCH and
 *                                 must be null otherwise.  Member k reads its slice where a single fit reads BEAN_BUF_X /
 *                                 BEAN_BUF_X_BC; member 0 reads its slice too.  Those two slots stay bound and the
 *                                 single-fit entry points (which address member 0) keep reading THEM, while the
 *                                 data-only words in member 0's workspace are then those of member 0's slice: as with
 *                                 member masks, on a handle with member counts the single-fit entry points are only
 *                                 meaningful if member 0's slice equals the shared buffer (the sample jackknife binds it
 *                                 so; the library does not compare the arrays).  Allowed after bean_hip_set_members and
 *                                 before bean_hip_prepare, with or without bean_hip_bind_member_masks (either may be
 *                                 bound, or both): a call marks the handle unprepared and drops the ensemble graphs,
 *                                 and the following bean_hip_prepare computes the data-only words (the loss constant
 *                                 holds the log-factorials of the counts; the observed totals per (replicate, guide))
 *                                 once per member - it does so whenever member masks OR member counts are bound.
 *                                 Member k is then, bit for bit, bean_hip_svi_run on a handle of its own whose
 *                                 BEAN_BUF_X, BEAN_BUF_X_BC, BEAN_BUF_REPGUIDE and BEAN_BUF_SAMPLE_MASK are member k's
 *                                 slices (size factors, a0 and every other buffer as bound here).  Null for both
 *                                 returns the handle to shared counts (prepare again).  The byte counts are checked
 *                                 against K.  The members' counts cost 4 K R B G bytes each; every other input stays
 *                                 shared.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched): a null handle; set_members on a shape that
 * is not supported, after a bind, with n_members outside [1, BEAN_HIP_MAX_MEMBERS]; run_ensemble with n_seeds !=
 * n_members or null seeds; bind_member_masks on a shape that is not supported, before set_members, with one mask null
 * and the other not, or with byte counts other than K R G and 8 K R B (the message states K); bind_member_counts on a
 * shape that is not supported, before set_members, with byte counts other than 4 K R B G (the message states K), with
 * x_bcmatch on a handle without BEAN_FLAG_USE_BCMATCH or without it on a handle with the flag, or with x null and
 * x_bcmatch not.  The handle stays usable after every one of them. */
#define BEAN_HIP_MAX_MEMBERS 64
int bean_hip_ensemble_supported(const bean_hip_ctx* ctx);
int bean_hip_survival_members_supported(const bean_hip_ctx* ctx);
int bean_hip_set_members(bean_hip_ctx* ctx, int32_t n_members);
int bean_hip_bind_member_masks(bean_hip_ctx* ctx, const void* repguide, uint64_t repguide_bytes,
                               const void* sample_mask, uint64_t sample_mask_bytes);
int bean_hip_bind_member_counts(bean_hip_ctx* ctx, const void* x, uint64_t x_bytes,
                                const void* x_bcmatch, uint64_t x_bcmatch_bytes);
int bean_hip_svi_run_ensemble(bean_hip_ctx* ctx, const uint64_t* seeds, int32_t n_seeds, uint64_t first_step,
                              uint64_t n_steps, int32_t graph_chunk, void* stream);

/* Multi-particle SVI: every step draws every latent site P times and applies ONE ClippedAdam update with the mean of
 * the P gradients (Pyro's Trace_ELBO(num_particles = P)).  With particle seeds s_0 ... s_{P-1}, step s is:
 *   1. for every particle p, bean_hip_elbo_grad(seed = s_p, step = s) at the current, shared parameters: the loss L_p
 *      and the float32 gradients g_p, bit for bit;
 *   2. per element, acc = (double)g_0, then + (double)g_1, + (double)g_2, ... in particle order, and the mean gradient
 *      is (float)(acc * (1.0 / P)): one float64 multiply, one rounding, no contraction;
 *   3. bean_hip_adam(t = s + 1) with that mean (it is clamped as a single gradient is; a NaN in any g_p stays);
 *   4. loss_hist[s] = (L_0 + L_1 + ... in particle order, float64) * (1.0 / P).
 * The P evaluations run in the same launches (the member axis of the ensemble kernels); P = 1 is bean_hip_svi_run.
 *
 *   bean_hip_set_particles        after bean_hip_create, before ANY bean_hip_bind; 1 <= n_particles <=
 *                                 BEAN_HIP_MAX_MEMBERS; only where bean_hip_ensemble_supported is 1.  Every buffer of
 *                                 the caller keeps its single-fit size: parameters, moments, gradients, loss_hist.  The
 *                                 handle owns what is per particle: a workspace copy, the loss accumulators, a (P, n)
 *                                 float32 gradient scratch per parameter array and (P, capacity) loss values.  It does
 *                                 not combine with bean_hip_set_members(K > 1): whichever of the two comes second is
 *                                 refused.  The single-fit entry points keep working.
 *   bean_hip_svi_run_particles    n_steps such steps from first_step: `seeds` is a HOST array of n_seeds == n_particles
 *                                 values.  The gradient buffers must be bound: behind the call they hold the mean
 *                                 gradient of its last step, and loss_hist[first_step .. first_step + n_steps) the mean
 *                                 losses; no other slot of loss_hist is written.  Windows give the bits of one call.
 *                                 Graphs of up to graph_chunk steps when graph_chunk > 0 (eager launches when 0).
 *                                 Injected / dumped noise is refused.  A following bean_hip_svi_resume does not
 *                                 continue it.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched): a null handle; set_particles on a shape that
 * is not supported, after a bind, with n_particles outside [1, BEAN_HIP_MAX_MEMBERS], or on a handle of more than one
 * member (and set_members(K > 1) on a handle of more than one particle); run_particles before set_particles, with
 * n_seeds != n_particles, null seeds, or noise buffers bound.  The handle stays usable after every one of them. */
int bean_hip_set_particles(bean_hip_ctx* ctx, int32_t n_particles);
int bean_hip_svi_run_particles(bean_hip_ctx* ctx, const uint64_t* seeds, int32_t n_seeds, uint64_t first_step,
                               uint64_t n_steps, int32_t graph_chunk, void* stream);

/* Posterior predictive check: replicate counts drawn on the device from the handle's current parameters.
 *
 *   bean_hip_predictive_supported 1 if the count simulator takes this handle, 0 if not: the sorting variant families
 *                                 k_guide_wave2 serves (Normal, MixtureNormal with or without accessibility scaling /
 *                                 fit_noise / X_bcmatch / --prior-params), unsharded, no sample covariates, on a
 *                                 single-fit handle (n_members == 1 and n_particles == 1), whichever stepping path the
 *                                 handle's size selects.  Not: tiling, survival, ControlNormal.
 *   bean_hip_simulate             draws the latent sites of "draw `draw`" - bit for bit the draws of
 *                                 bean_hip_elbo_grad(seed, step = draw), injected noise (*_IN slots) honoured the same
 *                                 way - forms the Dirichlet-Multinomial concentrations of every (replicate, guide) as
 *                                 the ELBO does, and draws p ~ Dirichlet(alpha), x_rep ~ Multinomial(n_obs, p) with
 *                                 n_obs the pair's observed total; masked pairs are simulated like any other.
 *                                 x_out: (R, B, G) float32, the layout of BEAN_BUF_X (and of one member of
 *                                 bean_hip_bind_member_counts); xbc_out: the same for X_bcmatch, required exactly when the
 *                                 handle was created with BEAN_FLAG_USE_BCMATCH and null (0 bytes) otherwise; alpha_out:
 *                                 null (0 bytes) or (2, R, B, G) float64, the floored concentrations of both
 *                                 likelihoods (plane 1 is written only with BEAN_FLAG_USE_BCMATCH).  All three are device
 *                                 memory of the caller.  The same (seed, draw) gives the same bits.  The call writes
 *                                 no parameter, moment, gradient, loss_hist entry or loss accumulator; it overwrites
 *                                 the workspace's draws and tables, so a following bean_hip_svi_resume does not
 *                                 continue an earlier window and bean_hip_svi_run starts from its own first draw, as
 *                                 after bean_hip_elbo_grad.  No graph is built or replayed.  The time is proportional
 *                                 to the largest n_obs of each 64-guide tile.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched): a null handle; a handle that is not
 * supported or not prepared; byte counts other than 4 R B G (x_out, xbc_out) and 16 R B G (alpha_out); xbc_out on a
 * handle without BEAN_FLAG_USE_BCMATCH or without it on a handle with the flag.  The handle stays usable. */
int bean_hip_predictive_supported(const bean_hip_ctx* ctx);
int bean_hip_simulate(bean_hip_ctx* ctx, uint64_t seed, uint64_t draw, void* x_out, uint64_t x_bytes, void* xbc_out,
                      uint64_t xbc_bytes, void* alpha_out, uint64_t alpha_bytes, void* stream);

/* K replicate screens of the handle's current parameters in ONE launch: the screens of a parametric bootstrap.
 *
 *   bean_hip_simulate_members     takes the handles bean_hip_predictive_supported takes, any size, and 1 <= n_draws <=
 *                                 BEAN_HIP_MAX_MEMBERS.  x_out: (K, R, B, G) float32, K = n_draws, member-major - exactly
 *                                 what bean_hip_bind_member_counts binds; xbc_out: the same shape, required exactly when
 *                                 the handle has BEAN_FLAG_USE_BCMATCH and null (0 bytes) otherwise.  No alpha_out.
 *                                 Launches: one k_set_step(first_draw, slot 0, n = 0), one PREP k_param, one
 *                                 k_simulate_members with the member on blockIdx.y.
 *                                 Which draw is whose: the per-target and per-guide Normal sites (mu, sd, the noise
 *                                 site, the tables) are those of the one PREP launch - draw first_draw, or the
 *                                 injected *_IN values - and are shared by all K members; the per-(replicate, guide)
 *                                 sites of member k - the pi draw, p ~ Dirichlet(alpha) and the categorical draws - use
 *                                 draw index first_draw + k wherever bean_hip_simulate uses `draw`.  So plane 0 is
 *                                 bean_hip_simulate(seed, first_draw) bit for bit, and with every Normal site injected
 *                                 plane k is bean_hip_simulate(seed, first_draw + k).  BEAN_BUF_PI_IN is honoured
 *                                 identically for every member; with BEAN_FLAG_DUMP_PI member 0 alone writes PI_OUT.
 *                                 State: as bean_hip_simulate - no parameter, moment, gradient, loss_hist entry or loss
 *                                 accumulator is written, and a following bean_hip_svi_resume does not continue an
 *                                 earlier window.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched, the handle stays usable): a null handle; a
 * handle that is not supported (the message names bean_hip_predictive_supported) or not prepared; n_draws outside
 * [1, BEAN_HIP_MAX_MEMBERS] (the message states the range); byte counts other than 4 K R B G (the message states K);
 * xbc_out on a handle without BEAN_FLAG_USE_BCMATCH or without it on a handle with the flag. */
int bean_hip_simulate_members(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws, void* x_out,
                              uint64_t x_bytes, void* xbc_out, uint64_t xbc_bytes, void* stream);

/* K replicate screens at each of D read depths in ONE launch: the screens of a depth study ("would sequencing deeper
 * tighten the hits?").
 *
 *   bean_hip_simulate_design      takes the handles bean_hip_predictive_supported takes, any size, n_depths = D >= 1,
 *                                 n_draws = K >= 1 and D * K <= BEAN_HIP_MAX_MEMBERS.  depths: D factors in HOST memory,
 *                                 each finite and > 0; they are copied into the launch's arguments before the call
 *                                 returns (no device pointer of the caller, no host synchronisation).  x_out:
 *                                 (D, K, R, B, G) float32, member-major with member m = i * K + j depth i, draw j -
 *                                 D * K members of bean_hip_bind_member_counts; xbc_out: the same shape, required
 *                                 exactly when the handle has BEAN_FLAG_USE_BCMATCH and null (0 bytes) otherwise.
 *                                 Launches: those of bean_hip_simulate_members - one k_set_step(first_draw, slot 0,
 *                                 n = 0), one PREP k_param - then one k_simulate_design with the member on blockIdx.y.
 *                                 Which draw is whose: member (i, j) is member j of bean_hip_simulate_members(seed,
 *                                 first_draw, K) - the shared Normal sites of draw first_draw (or the injected *_IN
 *                                 values), draw index first_draw + j for its pi, Dirichlet and categorical sites AT
 *                                 EVERY DEPTH (common random numbers across depths), BEAN_BUF_PI_IN and
 *                                 BEAN_FLAG_DUMP_PI as there - except that every (replicate, guide) draws
 *                                     n_i = floor(depths[i] * n_obs + 0.5)   (float64)
 *                                 reads instead of its observed total n_obs.  Concentrations, a0, masks and size
 *                                 factors are the observed ones: nothing else of the draw depends on the depth.  So
 *                                   (a) with depths[i] == 1 plane (i, j) is bit for bit plane j of
 *                                       bean_hip_simulate_members(seed, first_draw, K);
 *                                   (b) for depths[a] <= depths[b], plane (a, j) <= plane (b, j) elementwise: read t of
 *                                       a pair is word t of its stream and p does not depend on n;
 *                                   (c) every (replicate, guide) of plane (i, j) sums to n_i exactly.
 *                                 n_i is clamped to 2^24 - 1: the words a (likelihood, draw) owns in the categorical
 *                                 stream, and the limit of exact float32 integers.  Callers keep max(depths) * max n_obs
 *                                 below 2^24 (HipSVI.simulate_design refuses otherwise).  Cost: the time follows the
 *                                 LARGEST n_i of each 64-guide tile, so a depth-4 member takes four times its depth-1
 *                                 twin.  State: as bean_hip_simulate_members - nothing of the fit is written, and a
 *                                 following bean_hip_svi_resume does not continue an earlier window.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched, the handle stays usable): a null handle; a
 * handle that is not supported (the message names bean_hip_predictive_supported) or not prepared; null depths; D < 1,
 * K < 1 or D * K > BEAN_HIP_MAX_MEMBERS (the message states the product and the limit); a depth that is not finite or
 * not > 0 (the message states its index and value); byte counts other than 4 D K R B G (the message states D and K);
 * xbc_out on a handle without BEAN_FLAG_USE_BCMATCH or without it on a handle with the flag. */
int bean_hip_simulate_design(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws, const double* depths,
                             int32_t n_depths, void* x_out, uint64_t x_bytes, void* xbc_out, uint64_t xbc_bytes,
                             void* stream);

/* K replicate screens at each of D PLANTED EFFECTS in ONE launch: the screens of a power study ("how large must a
 * variant's effect be for this screen to have called it, and how often does a null variant cross the threshold?").
 *
 *   bean_hip_simulate_power       takes the handles bean_hip_predictive_supported takes, any size, n_effects = D >= 1,
 *                                 n_draws = K >= 1 and D * K <= BEAN_HIP_MAX_MEMBERS.  effects: D finite values in HOST
 *                                 memory, copied into the launch's arguments before the call returns.  plant: a
 *                                 DEVICE array of T bytes (non-zero: the target is planted), read by the kernel on
 *                                 `stream`, or null: every target is planted.  x_out: (D, K, R, B, G) float32,
 *                                 member-major with member m = i * K + j effect i, draw j - D * K members of
 *                                 bean_hip_bind_member_counts; xbc_out: the same shape, required exactly when the
 *                                 handle has BEAN_FLAG_USE_BCMATCH and null (0 bytes) otherwise.
 *                                 Launches: those of bean_hip_simulate_members - one k_set_step(first_draw, slot 0,
 *                                 n = 0), one PREP k_param - then one k_simulate_power with the member on blockIdx.y.
 *                                 Which draw is whose: member (i, j) is member j of bean_hip_simulate_members(seed,
 *                                 first_draw, K) - the shared Normal sites of draw first_draw (or the injected *_IN
 *                                 values), draw index first_draw + j for its pi, Dirichlet and categorical sites AT
 *                                 EVERY EFFECT (common random numbers across effects), BEAN_BUF_PI_IN and
 *                                 BEAN_FLAG_DUMP_PI as there - except that a (replicate, guide) of a planted target
 *                                 takes, wherever the table P[b, t] is read,
 *                                     Phi((z_hi[b] - e) / sigma_t) - Phi((z_lo[b] - e) / sigma_t),   e = effects[i],
 *                                 with sigma_t from the target's drawn y_t as the PREP launch forms it: mu_t = e, the
 *                                 value itself and not a shift of the fitted mean.  The operations are those of the
 *                                 PREP launch's table, so
 *                                   (a) with nothing planted (an all-zero plant) plane (i, j) is bit for bit plane j of
 *                                       bean_hip_simulate_members(seed, first_draw, K);
 *                                   (b) plane (i, j) is bit for bit plane j of bean_hip_simulate_members on a twin
 *                                       handle that is equal in everything but mu_loc = float32(e) and eps_mu = 0 on
 *                                       the planted targets (for an e that float32 holds exactly);
 *                                   (c) every (replicate, guide) of every plane sums to n_obs exactly;
 *                                   (d) the (replicate, guide) pairs of unplanted targets are those of
 *                                       bean_hip_simulate_members in every plane.
 *                                 The variant families share no parameter between targets, so all targets may be
 *                                 planted at once.  Cost: that of D * K members of bean_hip_simulate_members plus 2 B
 *                                 normal CDFs per (planted pair, likelihood).  State: as bean_hip_simulate_members -
 *                                 nothing of the fit is written, and a following bean_hip_svi_resume does not continue
 *                                 an earlier window.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched, the handle stays usable): a null handle; a
 * handle that is not supported (the message names bean_hip_predictive_supported) or not prepared; null effects; D < 1,
 * K < 1 or D * K > BEAN_HIP_MAX_MEMBERS (the message states the product and the limit); an effect that is not finite
 * (the message states its index and value); byte counts other than 4 D K R B G (the message states D and K); xbc_out on
 * a handle without BEAN_FLAG_USE_BCMATCH or without it on a handle with the flag. */
int bean_hip_simulate_power(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws, const double* effects,
                            int32_t n_effects, const void* plant, void* x_out, uint64_t x_bytes, void* xbc_out,
                            uint64_t xbc_bytes, void* stream);

/* Per-target log importance weights of S draws from the fitted guide: the device side of the importance-sampling check
 * of the mean-field posterior (PSIS k-hat, importance-corrected mu and mu_sd per target).
 *
 *   bean_hip_log_weights          takes the handles bean_hip_predictive_supported takes, any size, n_draws in
 *                                 [1, BEAN_HIP_MAX_LOGW_DRAWS].  For j < n_draws, draw d = first_draw + j is the draw
 *                                 bean_hip_elbo_grad(seed, step = d) evaluates - same sites, counters, operands and bits,
 *                                 the injected BEAN_BUF_*_IN values honoured (every draw of the call is then the same
 *                                 draw) - and
 *                                     logw_out[j, t] = log p(x_t, z_t) - log q(z_t)
 *                                 of target t: its mu and sd sites, its guides' pi (and, with accessibility, noise)
 *                                 sites, and the likelihood terms of its (replicate, guide) pairs, data-only constants
 *                                 included, so that  - sum_t logw_out[j, t]  is the loss bean_hip_elbo_grad reports for
 *                                 that draw.  mu_out[j, t] / y_out[j, t]: the drawn mu_t and y_t = log sd_t (y_out may
 *                                 be null with 0 bytes).  pair_out: caller-owned scratch of (n_draws, R, G) float64,
 *                                 required; after the call it holds the terms of every (draw, replicate, guide) pair -
 *                                 the two Dirichlet-Multinomial log-probabilities (under the repguide mask and
 *                                 n > mask_thres), the control-allele Multinomial, log p(pi) under the repguide mask and
 *                                 - log q(pi), without the per-guide Dirichlet normalisers.  Guides in the handle's
 *                                 order.  All four arrays are DEVICE memory, float64, draw-major.
 *                                 Launches: one k_logw_consts (the pairs' data-only constants, once per call), one
 *                                 k_logw_pairs (grid of k_simulate_members, the draw on blockIdx.y) and one
 *                                 k_logw_targets, whatever n_draws; no k_set_step, no k_param.
 *                                 State: parameters, moments, gradients, loss_hist and the workspace are not written;
 *                                 the handle's seed is, so a following bean_hip_svi_resume does not continue an earlier
 *                                 window.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched, the handle stays usable): a null handle; a
 * handle that is not supported (the message names bean_hip_predictive_supported) or not prepared; n_draws outside
 * [1, BEAN_HIP_MAX_LOGW_DRAWS] (the message states the range); a null logw_out, mu_out or pair_out; byte counts other
 * than 8 n_draws T (logw_out, mu_out, a non-null y_out), 0 (a null y_out) and 8 n_draws R G (pair_out) - the message
 * states n_draws and the bytes expected. */
#define BEAN_HIP_MAX_LOGW_DRAWS 4096
int bean_hip_log_weights(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws, void* logw_out,
                         uint64_t logw_bytes, void* mu_out, uint64_t mu_bytes, void* y_out, uint64_t y_bytes,
                         void* pair_out, uint64_t pair_bytes, void* stream);

/* The same weights with pi integrated out of the model: the importance weight of (mu_t, sd_t) alone (DESIGN.md section
 * 21).  MixtureNormal's joint weight covers the 2 R n_guides pi coordinates of a target, for which the product Dirichlet
 * guide is a poor proposal whatever the quality of q(mu_t); this one is a 2-D importance-sampling problem per target.
 *
 *   bean_hip_log_weights_marginal takes the handles, draws and arrays of bean_hip_log_weights with the same size
 *                                 checks, and
 *                                     logw_out[j, t] = log p(x_t, mu_t, sd_t[, noise]) - log q(mu_t, sd_t[, noise]),
 *                                 the pi site of every (replicate, guide) integrated out of the model: one 1-D integral
 *                                 per (draw, replicate, guide) in u = logit(pi_1), by n_nodes-point Gauss-Hermite
 *                                 centred at the mode of the log integrand and scaled by its curvature there (a fixed
 *                                 number of clamped Newton steps from the Beta factor's centre).  n_nodes is 16, 32 or
 *                                 64.  No term of q(pi) appears.  mu_out / y_out are bean_hip_log_weights', bit for bit;
 *                                 injected eps_mu / eps_sd / eps_noise are honoured, an injected pi is ignored.
 *                                 pair_out[j, r, g] afterwards: the pair's data-only constants plus, under the repguide
 *                                 mask, the log of its integral.
 *                                 unresolved_out[t] (DEVICE int32, T of them): the pairs of target t under the repguide
 *                                 mask at which the rule is not valid - min over the two alleles of (c_p + control
 *                                 allele counts) below 2; a draw-independent count.  The weights of a target with such a
 *                                 pair are computed all the same and are not to be used.
 *                                 BEAN_FAMILY_NORMAL has no pi: exactly the launches of bean_hip_log_weights (logw_out
 *                                 bit for bit) and unresolved_out zeroed.
 *                                 Launches (MixtureNormal): k_logw_consts, k_logw_unresolved, k_logw_pairs_marg,
 *                                 k_logw_targets_marg, whatever n_draws.  State: as bean_hip_log_weights.
 *
 * Errors: those of bean_hip_log_weights under this function's name; n_nodes other than 16, 32, 64 (the message names
 * n_nodes); a null unresolved_out or unresolved_bytes other than 4 T. */
int bean_hip_log_weights_marginal(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws, int32_t n_nodes,
                                  void* logw_out, uint64_t logw_bytes, void* mu_out, uint64_t mu_bytes, void* y_out,
                                  uint64_t y_bytes, void* pair_out, uint64_t pair_bytes, void* unresolved_out,
                                  uint64_t unresolved_bytes, void* stream);

/* The log joint of every target on a grid of GIVEN (mu_t, y_t = log sd_t), pi integrated out of the model: the device
 * side of the grid posterior of (mu, sd) per target (posterior mean and sd of mu without a mean-field assumption,
 * P(mu > 0 | x), log evidence).  In the sorting variant families the targets share no parameter,
 * so with pi integrated out the posterior of a target is a function of two numbers.
 *
 *   bean_hip_marginal_grid        takes the handles bean_hip_predictive_supported takes, without accessibility.
 *                                 N = n_mu * n_y nodes per target; node n = i * n_y + k of target t is
 *                                     mu = centre_mu[t] + (i - (n_mu - 1) / 2) * step_mu[t]
 *                                     y  = centre_y[t]  + (k - (n_y - 1) / 2) * step_y[t]
 *                                 formed in float64: every target has its own affine grid.  centre_mu, centre_y, step_mu
 *                                 and step_y are DEVICE float64 arrays of T.  No seed, no draw, no term of q.
 *                                     lj_out[n, t] = log p(mu) + log p(sd) + y
 *                                                  + sum_g nrg_g (lgamma(c_p0 + c_p1) - lgamma(c_p0) - lgamma(c_p1))
 *                                                  + sum_r sum_g ( const[r, g] + [rg] log int f(pi) dpi ),
 *                                 the log joint of the target as a density in (mu, y): the priors are those of the fit
 *                                 (BEAN_BUF_PRIOR_* included), const, f, the n_nodes-point rule (16, 32 or 64) and its
 *                                 validity predicate those of bean_hip_log_weights_marginal.  BEAN_FAMILY_NORMAL has no
 *                                 pi: a pair's term is its likelihood term, and unresolved_out is zeroed.
 *                                 pair_out: caller-owned scratch of (N, R, G) float64, required; afterwards
 *                                 pair_out[n, r, g] holds the pair's data-only constants plus, under the repguide mask,
 *                                 its term at node n.  unresolved_out: as bean_hip_log_weights_marginal's.
 *                                 Launches: k_logw_consts, k_logw_unresolved (MixtureNormal), k_grid_pairs,
 *                                 k_grid_targets, whatever N.
 *                                 State: nothing of the handle is written - no parameters, moments, gradients,
 *                                 loss_hist, workspace or seed; a following bean_hip_svi_resume continues its window.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched, the handle stays usable): a null handle; a
 * handle that is not supported (the message names bean_hip_predictive_supported), not prepared, or has accessibility
 * (the message says so: with it the guide noise is a further latent per guide and the posterior is not 2-D); n_nodes
 * other than 16, 32, 64; n_mu or n_y below 1 or n_mu * n_y above BEAN_HIP_MAX_LOGW_DRAWS (the message states both and
 * the limit); a null array; byte counts other than 8 N T (lj_out), 8 N R G (pair_out) and 4 T (unresolved_out) - the
 * message states N and the bytes expected. */
int bean_hip_marginal_grid(bean_hip_ctx* ctx, int32_t n_nodes, int32_t n_mu, int32_t n_y, const void* centre_mu,
                           const void* centre_y, const void* step_mu, const void* step_y, void* lj_out, uint64_t lj_bytes,
                           void* pair_out, uint64_t pair_bytes, void* unresolved_out, uint64_t unresolved_bytes,
                           void* stream);

/* bean_hip_marginal_grid with a Gauss-Jacobi rule for the pairs its predicate leaves out.
 *
 *   bean_hip_marginal_grid_tail   bean_hip_marginal_grid's arguments, refusals and state contract, plus tail_err_out,
 *                                 (N, T) float64.  A tail pair is a pair under the repguide mask that fails the
 *                                 predicate min(a0', a1') >= 2; unresolved_out keeps its meaning and is now also the
 *                                 number of tail pairs of the target.  A tail pair's log integral is
 *                                     lbeta(a0', a1') + logsumexp_i(lw_i + lg(z_i))
 *                                 over the 64 Gauss-Jacobi nodes of the weight z^(min a' - 1) (1 - z)^(max a' - 1), z the
 *                                 share of the smaller exponent's side; its slot of pair_out holds the pair's constant
 *                                 plus that.  The 48-node rule gives a second value: tail_err_out[n, t] is the sum over
 *                                 the target's tail pairs of |J64 - J48| at node n.  Slots of resolved pairs are bit for
 *                                 bit those of bean_hip_marginal_grid; with no tail pair so are lj_out and pair_out, and
 *                                 tail_err_out is zero (BEAN_FAMILY_NORMAL: always).
 *                                 Launches (MixtureNormal): k_logw_unresolved, k_tail_offsets, one host synchronisation
 *                                 of the stream (the number of tail pairs), with tail pairs k_tail_list and k_tail_nodes,
 *                                 k_logw_consts, k_grid_pairs, with tail pairs k_grid_pairs_tail, k_grid_targets, with
 *                                 tail pairs k_grid_targets_tail.
 *                                 Workspace, owned by the handle and read by nothing else: 1 800 + 8 N bytes per tail
 *                                 pair.  A call that would need more than 256 MiB is refused after the count (only
 *                                 unresolved_out has been written); the message names the number of tail pairs.
 *   bean_hip_marginal_tail_nodes  the compact list of tail pairs - ordered by target, guide, replicate - and its nodes.
 *                                 *n_tail_out (HOST int32) receives the number of tail pairs; with capacity = 0 nothing
 *                                 else is written.  Otherwise capacity must be at least that number, and the first
 *                                 n_tail entries are written of pair_index_out (capacity) int32, r * G + g in the
 *                                 handle's guide order; z_out and lw_out (capacity, 112) float64, the 64 nodes
 *                                 ascending and then the 48, log weights normalised to sum 1; side_out (capacity) int32,
 *                                 1 where the smaller exponent is pi_1's (ties included), 0 where it is pi_0's.  Device
 *                                 arrays.  BEAN_FAMILY_NORMAL: 0 pairs.  Same handles, same state contract. */
int bean_hip_marginal_grid_tail(bean_hip_ctx* ctx, int32_t n_nodes, int32_t n_mu, int32_t n_y, const void* centre_mu,
                                const void* centre_y, const void* step_mu, const void* step_y, void* lj_out,
                                uint64_t lj_bytes, void* pair_out, uint64_t pair_bytes, void* unresolved_out,
                                uint64_t unresolved_bytes, void* tail_err_out, uint64_t tail_err_bytes, void* stream);
int bean_hip_marginal_tail_nodes(bean_hip_ctx* ctx, int32_t capacity, void* pair_index_out, void* z_out, void* lw_out,
                                 void* side_out, int32_t* n_tail_out, void* stream);

/* bean_hip_log_weights_marginal with that Gauss-Jacobi rule for the pairs its predicate leaves out (DESIGN.md section
 * 25).  Accessibility is admitted, as for the importance weights: the noise stays a drawn site.
 *
 *   bean_hip_log_weights_marginal_tail
 *                                 bean_hip_log_weights_marginal's arguments, refusals and state contract, plus
 *                                 tail_err_out, (n_draws, T) float64 on the device.  The tail pairs, their order and
 *                                 their 64 + 48 nodes are those of bean_hip_marginal_grid_tail; the integrand of draw j
 *                                 is taken at the drawn (mu_t, y_t) of the pair's target and, with accessibility, at
 *                                 the guide's drawn noise.  A tail pair's slot of pair_out holds its constant plus
 *                                 lbeta(a0', a1') + the 64-node log-sum-exp; tail_err_out[j, t] is the sum over the
 *                                 target's tail pairs of |J64 - J48| at draw j.  mu_out, y_out, unresolved_out, the
 *                                 slots of resolved pairs and logw_out of targets without tail pairs are bit for bit
 *                                 those of bean_hip_log_weights_marginal; with no tail pair so is everything, and
 *                                 tail_err_out is zero (BEAN_FAMILY_NORMAL: always).  Draw first_draw + j has the
 *                                 same bits whatever n_draws and however the draws are split over calls.
 *                                 Launches (MixtureNormal): k_logw_unresolved, k_tail_offsets, one host synchronisation
 *                                 of the stream (the number of tail pairs), with tail pairs k_tail_list and k_tail_nodes,
 *                                 k_logw_consts, k_logw_pairs_marg, with tail pairs k_logw_pairs_marg_tail (one lane
 *                                 per (tail pair, draw)), k_logw_targets_marg, with tail pairs k_grid_targets_tail.
 *                                 Workspace: the handle's, 1 800 + 8 n_draws bytes per tail pair.  A call that would
 *                                 need more than 256 MiB is refused after the count (only unresolved_out has been
 *                                 written); the message names the number of tail pairs.
 *
 * Errors: those of bean_hip_log_weights_marginal under this function's name; a null tail_err_out or tail_err_bytes
 * other than 8 n_draws T. */
int bean_hip_log_weights_marginal_tail(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                       int32_t n_nodes, void* logw_out, uint64_t logw_bytes, void* mu_out,
                                       uint64_t mu_bytes, void* y_out, uint64_t y_bytes, void* pair_out,
                                       uint64_t pair_bytes, void* unresolved_out, uint64_t unresolved_bytes,
                                       void* tail_err_out, uint64_t tail_err_bytes, void* stream);

/* Posterior predictive check of a SURVIVAL screen: replicate counts over the timepoints, drawn on the device from the
 * handle's current parameters (k_simulate_survival).
 *
 *   bean_hip_survival_predictive_supported
 *                                 1 if the survival count simulator takes this handle, 0 if not: survival selection,
 *                                 family Normal or MixtureNormal (with or without accessibility scaling / X_bcmatch),
 *                                 unsharded, no sample covariates, the loss owner, n_members == 1 and n_particles == 1.
 *                                 Not: sorting screens (bean_hip_simulate serves them), tiling, ControlNormal.
 *   bean_hip_simulate_survival    the signature, buffer rules and state contract of bean_hip_simulate.  Draws the latent
 *                                 sites of "draw `draw`" - bit for bit the draws of bean_hip_elbo_grad(seed, step =
 *                                 draw): the Normal sites, the baseline u_g, pi, the Dirichlet-over-all-guides site;
 *                                 injected noise (*_IN slots) is honoured the same way, and the *_OUT slots that are bound
 *                                 hold the draw afterwards - forms the Dirichlet-Multinomial concentrations of every
 *                                 (replicate, guide) over the timepoints as k_guide_survival_wave does, and draws
 *                                 p ~ Dirichlet(alpha), x_rep ~ Multinomial(n_obs, p) from the sites and counters
 *                                 bean_hip_simulate uses.  Masked pairs are simulated like any other.  x_out, xbc_out:
 *                                 (R, B, G) float32; alpha_out: null (0 bytes) or (2, R, B, G) float64.  The same (seed,
 *                                 draw) gives the same bits.  The call writes no parameter, moment, gradient, loss_hist
 *                                 entry or loss accumulator; a following bean_hip_svi_resume does not continue an earlier
 *                                 window.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched): a null handle; a handle that is not
 * supported (the message names bean_hip_survival_predictive_supported and what it takes) or not prepared; byte counts
 * other than 4 R B G (x_out, xbc_out) and 16 R B G (alpha_out); xbc_out on a handle without BEAN_FLAG_USE_BCMATCH or
 * without it on a handle with the flag.  The handle stays usable. */
int bean_hip_survival_predictive_supported(const bean_hip_ctx* ctx);
int bean_hip_simulate_survival(bean_hip_ctx* ctx, uint64_t seed, uint64_t draw, void* x_out, uint64_t x_bytes,
                               void* xbc_out, uint64_t xbc_bytes, void* alpha_out, uint64_t alpha_bytes, void* stream);

/* K replicate screens of a SURVIVAL handle's current parameters in ONE launch: the screens of a survival screen's
 * parametric bootstrap (k_simulate_survival_members).
 *
 *   bean_hip_simulate_survival_members
 *                                 takes the handles bean_hip_survival_predictive_supported takes, any size, and 1 <=
 *                                 n_draws <= BEAN_HIP_MAX_MEMBERS.  x_out: (K, R, B, G) float32, K = n_draws,
 *                                 member-major; xbc_out: the same shape, required exactly when the handle has
 *                                 BEAN_FLAG_USE_BCMATCH and null (0 bytes) otherwise.  No alpha_out.
 *                                 Launches: one k_set_step(first_draw, slot 0, n = 0), the one PREP k_param of
 *                                 bean_hip_simulate_survival, one k_simulate_survival_members with the member on
 *                                 blockIdx.y.  No graph.
 *                                 Which draw is whose: mu_t, lpn (the per-target and per-guide Normal sites) and gam /
 *                                 gsum (the Dirichlet-over-all-guides site) are those of the one PREP launch - draw
 *                                 first_draw, or the injected *_IN values - and are shared by all K members.  The
 *                                 baseline u_g (MixtureNormal): with BEAN_BUF_EPS_U_IN that value for every member;
 *                                 otherwise member k redraws it in the kernel for draw first_draw + k with PREP's own
 *                                 expression (member 0: the value PREP left).  Member k's pi draw, p ~ Dirichlet(alpha)
 *                                 and the categorical draws use draw index first_draw + k wherever
 *                                 bean_hip_simulate_survival uses `draw`.  So plane 0 is bean_hip_simulate_survival(seed,
 *                                 first_draw) bit for bit, and with the shared sites injected plane k is
 *                                 bean_hip_simulate_survival(seed, first_draw + k).  BEAN_BUF_PI_IN and BEAN_BUF_X0_IN
 *                                 are honoured identically for every member; member 0 alone writes PI_OUT (with
 *                                 BEAN_FLAG_DUMP_PI) and X0_OUT; the kernel writes no u_g, eps_u or EPS_U_OUT (they hold
 *                                 draw first_draw, from PREP).
 *                                 State: as bean_hip_simulate_survival - no parameter, moment, gradient, loss_hist entry
 *                                 or loss accumulator is written, and a following bean_hip_svi_resume does not continue
 *                                 an earlier window.
 *
 * Errors (status < 0, message in bean_hip_last_error(), nothing launched, the handle stays usable): a null handle; a
 * handle that is not supported (the message names bean_hip_survival_predictive_supported) or not prepared; n_draws
 * outside [1, BEAN_HIP_MAX_MEMBERS] (the message states the range); byte counts other than 4 K R B G (the message
 * states K); xbc_out on a handle without BEAN_FLAG_USE_BCMATCH or without it on a handle with the flag. */
int bean_hip_simulate_survival_members(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws,
                                       void* x_out, uint64_t x_bytes, void* xbc_out, uint64_t xbc_bytes, void* stream);

/* The same loop for a fit that is stepped in windows (run_inference reports every 100 steps,
 * bean/model/run.py:378): results are those of bean_hip_svi_run, bit for bit, but the call ends with the
 * draw and the tables of step first_step + n_steps already on the device, and a call that continues exactly
 * there - same seed, same stream, first_step = the previous call's first_step + n_steps, nothing bound,
 * prepared or stepped through another entry point in between - starts stepping at once instead of with the
 * two preparing launches.  The caller asserts that it has not written the bound parameter / moment buffers
 * since the previous call returned (the library cannot see such writes; use bean_hip_svi_run after one).
 * Falls back to bean_hip_svi_run when per-step noise is injected or dumped. */
int bean_hip_svi_resume(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_step,
                        uint64_t n_steps, int32_t graph_chunk, void* stream);

/* The same loop for guide-sharded fits of families in which something is shared across the
 * shards (the reference is single-process, so there is no interface to
 * mirror).  The step is cut at its exchange points; after each call that names a buffer the
 * caller all-reduces (sum) that caller-owned buffer over the ranks, on the same stream:
 *
 *   bean_hip_sharded_begin(first_step, n_steps)     once per run: zero the loss window, draw step 0
 *   per step:
 *     bean_hip_sharded_sums      -> BEAN_BUF_XCHG_GSUM   (survival MixtureNormal / NormalModel: normalisers
 *                                                         of the Dirichlet-over-guides draw; no-op otherwise)
 *     bean_hip_sharded_guide     -> BEAN_BUF_XCHG_TGRAD  (ControlNormal, tiling: per-target likelihood
 *                                                         gradients; not written when the slot is unbound)
 *                                -> BEAN_BUF_XCHG_SQ     (survival NormalModel: projection sums)
 *                                -> BEAN_BUF_XCHG_COV    (sorting NormalModel with sample covariates: the
 *                                                         replicates' gradient sums of the shared mu_cov site)
 *     bean_hip_sharded_update(last)                       gradients, ClippedAdam, draws of the next step;
 *                                                         last != 0 on the run's final step: no further draw, and
 *                                                         loss_hist of ALL the run's steps is written (once, here)
 *
 * Families whose parameters are all per-target or per-guide with target-aligned shards (sorting
 * Normal / MixtureNormal) need none of this: bean_hip_svi_run on every rank is the sharded fit. */
int bean_hip_sharded_begin(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_step, uint64_t n_steps, void* stream);
int bean_hip_sharded_sums(bean_hip_ctx* ctx, void* stream);
int bean_hip_sharded_guide(bean_hip_ctx* ctx, void* stream);
int bean_hip_sharded_update(bean_hip_ctx* ctx, int32_t last, void* stream);

/* The same per-step exchange without the host in the loop: the library owns an RCCL communicator (one
 * process per GPU; RCCL is resolved at run time from the shared object `rccl_path` names - the one
 * PyTorch has already loaded - so that the library itself has no link-time dependency on it) and
 * bean_hip_svi_run_exchanged enqueues, per step,
 *     [all-reduce GSUM] guide kernels [all-reduce TGRAD (+ SQ, grouped)] update
 * on `stream`: ncclAllReduce(sum, float64, in place) on the bound BEAN_BUF_XCHG_* buffers between the
 * kernels, no host synchronisation, no Python.  graph_chunk > 0 additionally captures 2^k steps,
 * collectives included, into hipGraphs (opt-in: whether RCCL's kernels can be captured depends on the
 * RCCL build; on refusal the call falls back to eager launches and says so in bean_hip_last_error).
 *
 *   bean_hip_comm_unique_id   rank 0 only: fills id[128] (ncclGetUniqueId); the caller broadcasts it
 *   bean_hip_comm_init        every rank, collectively (ncclCommInitRank on the current device)
 *   bean_hip_comm_all_reduce  one ncclAllReduce(sum, float64, in place) of `n` doubles on that communicator and `stream`:
 *                             what bean_hip_svi_run_exchanged issues between its kernels, callable by itself so that a
 *                             caller can CHECK a fresh communicator against a known sum before a fit depends on it
 *   bean_hip_comm_destroy     ncclCommDestroy
 * Returns 0, or -1 with bean_hip_last_error() (RCCL missing, refused, ...): callers then keep stepping
 * with bean_hip_sharded_* and their own all-reduce. */
#define BEAN_HIP_COMM_ID_BYTES 128
int bean_hip_comm_unique_id(const char* rccl_path, uint8_t* id);
int bean_hip_comm_init(bean_hip_ctx* ctx, const char* rccl_path, const uint8_t* id, int32_t rank, int32_t world);
int bean_hip_comm_all_reduce(bean_hip_ctx* ctx, double* buf, uint64_t n, void* stream);
int bean_hip_comm_destroy(bean_hip_ctx* ctx);
int bean_hip_svi_run_exchanged(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_step, uint64_t n_steps,
                               int32_t graph_chunk, void* stream);

/* Introspection for bench.py / DESIGN.md: algorithmic bytes one step moves
 * (each input read once, each parameter and moment read and written once) and
 * the name of the dominant kernel. */
uint64_t bean_hip_step_bytes(const bean_hip_ctx* ctx);
const char* bean_hip_dominant_kernel(const bean_hip_ctx* ctx);
/* Dynamic LDS (bytes per workgroup) the library requests when it launches that kernel for this shape -
 * the figure that, with the code object's register counts, decides how many waves a CU holds (profilers
 * report the static segment only). */
uint64_t bean_hip_dominant_lds_bytes(const bean_hip_ctx* ctx);
/* ... and the template instantiation that is launched for this shape, as it is spelt in the code object
 * (e.g. "k_guide_wave2<2, false>"), to look its register counts up there. */
const char* bean_hip_dominant_kernel_variant(const bean_hip_ctx* ctx);

/* Time (ms, HIP events on `stream`) of the dominant kernel averaged over the
 * launches issued since the previous call; enable with profile != 0 in
 * bean_hip_set_profile before running steps (eager mode only). */
int bean_hip_set_profile(bean_hip_ctx* ctx, int32_t enable);
int bean_hip_get_profile(bean_hip_ctx* ctx, double* avg_ms, uint64_t* launches);

/* Unit-test hooks for the device special functions (n elements, device ptrs):
 *   op 0: out0 = lgamma(a+x)-lgamma(a), out1 = digamma(a+x)-digamma(a)
 *   op 1: out0 = lgamma(a),             out1 = digamma(a)
 *   op 2: out0 = dirichlet_grad(x, a, total=b)
 *   op 3: out0 = Phi(a)
 *   op 4: out0, out1 = Dirichlet(a, b) draw (seed = x[0] bits, element index)
 *   op 5: as op 0 through the two-chain evaluation (element i paired with element i ^ 1)
 *   op 6: out0, out1 = max((float)Gamma(a), FLT_MIN), max((float)Gamma(b), FLT_MIN) from the plain pair sampler
 *   op 7: the same from the float32-floor sampler of the survival q0 site (must equal op 6 draw for draw)
 *   op 8: out0, out1 = max(Gamma(a), DBL_MIN), max(Gamma(b), DBL_MIN) from the plain pair sampler
 *   op 9: the same from the double-floor sampler of the wide tiling kernel (must equal op 8 draw for draw)
 *   op 10: as op 2 through dirichlet_grad_one_pre with digamma(a), digamma(b) supplied (must equal op 2 bit for bit)
 *   op 11: as op 10 through dirichlet_grad_one_tab, its x-free factors tabulated in the kernel as the finish tabulates
 *          them (must equal op 10 bit for bit)
 *   op 12 - 14: out0, out1 = Gamma(a), Gamma(b), unfloored, from the inlined pair sampler whose acceptance test is
 *          settled in float32 where it can be, FLOOR form 0, 1, 2 (seed = x[0] bits, element index)
 *   op 15 - 17: the same from the out-of-line samplers with the float64 test (must equal 12 - 14 draw for draw)
 *   op 18 - 23: as 12 - 17 with out0 = the generator position after the draw
 *   op 24: the acceptance test alone at (d, n, u) = (a, x, b): out0 = the float64 decision (-1: 1 + c n <= 0),
 *          out1 = the float32 form's decision + 2 where float32 settled it
 *   op 25: the four words (x, y, z, w) of the Philox4x32-10 block at (seed = x[0] bits, subsequence = a[i] bits,
 *          offset = b[i] bits, in 32-bit words): out0 bits = (y << 32) | x, out1 bits = (w << 32) | z.  All five are
 *          64-bit patterns carried in the doubles, loaded and stored as integers */
int bean_hip_test_special(int32_t op, uint64_t n, const double* a, const double* x,
                          const double* b, double* out0, double* out1, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BEAN_HIP_H */
