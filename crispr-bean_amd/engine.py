"""Host-side driver of the HIP SVI step.

Owns the torch tensors (parameters, ClippedAdam moments, gradients, loss
history) whose device pointers are bound into a ``libbean_hip`` handle, and
exposes the three operations the reference gets from Pyro
(``bean/model/run.py:366-396``): one ELBO+gradient evaluation, one ClippedAdam
update, and the fused ``for t in range(num_steps): svi.step(data)`` loop.

PyTorch is used for device memory and streams only; all arithmetic of the step
happens in the HIP kernels.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib

PI_NOISE_SD = 0.655  # bean/model/utils.py:133
PER_GUIDE = ("alpha_pi", "noise_loc", "noise_scale", "q0", "initial_abundance")  # parameters with a guide axis
POSITIVE = ("mu_scale", "sd_scale", "alpha_pi", "noise_scale", "q0", "initial_abundance", "mu_cov_scale")


def _quantile_edges(upper: torch.Tensor, lower: torch.Tensor):
    """z-scores of the bin edges; quantiles exactly 1.0 / 0.0 are open edges
    (``bean/model/utils.py:48-54``)."""
    std = torch.distributions.Normal(0.0, 1.0)
    uq, lq = upper.detach().cpu().double(), lower.detach().cpu().double()
    z_hi = torch.full_like(uq, float("inf"))
    z_lo = torch.full_like(lq, float("-inf"))
    z_hi[uq != 1.0] = std.icdf(uq[uq != 1.0])
    z_lo[lq != 0.0] = std.icdf(lq[lq != 0.0])
    return z_hi, z_lo


class EnsembleUnsupported(ValueError):
    """``HipSVI(..., n_members=K)`` on a shape the batched kernels do not take (neither ``bean_hip_ensemble_supported``
    nor ``bean_hip_survival_members_supported``)."""


class PredictiveUnsupported(ValueError):
    """A posterior predictive check on a shape the count simulator does not take (``bean_hip_predictive_supported``)."""


def _ptr(t):
    """A tensor's device address as the library takes it; ``None`` is a null pointer."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _nbytes(t):
    """The bytes a tensor holds; 0 for ``None``."""
    return 0 if t is None else t.numel() * t.element_size()


def particle_mean(values):
    """Mean of P tensors as a particle step forms it (``include/bean_hip.h``): a float64 accumulator that starts from the
    first and adds the others in order, ONE multiply by ``1.0 / P``, then one rounding to the inputs' dtype."""
    acc = values[0].to(torch.float64, copy=True)
    for v in values[1:]:
        acc += v.to(torch.float64)
    acc *= 1.0 / len(values)
    return acc.to(values[0].dtype)


class HipSVI:
    """One model family bound to one screen on one GPU."""

    def __init__(
        self,
        family: str,
        data,
        *,
        use_bcmatch: bool = True,
        scale_by_accessibility: bool = False,
        fit_noise: bool = True,
        sd_scale: float = 0.01,
        prior_params: Optional[dict] = None,
        initial_lr: float = 0.01,
        gamma: float = 0.1,
        num_steps: int = 2000,
        loss_capacity: Optional[int] = None,
        mask_thres: int = 10,
        dump_noise: bool = False,
        device=None,
        guide_offset: int = 0,
        target_offset: int = 0,
        n_guides_total: int = 0,
        mu_negctrl=(0.0, 0.1),
        t0_totals: Optional[torch.Tensor] = None,
        loss_owner: bool = True,
        alpha_prior: float = 1.0,
        lib_variant: Optional[str] = None,
        guide_ids: Optional[torch.Tensor] = None,
        n_members: int = 1,
        member_masks=None,
        member_counts=None,
        n_particles: int = 1,
    ):
        if family not in _lib.FAMILY:
            raise ValueError(f"unknown model family {family!r}")
        if not 1 <= int(n_particles) <= _lib.MAX_MEMBERS:
            raise ValueError(f"n_particles must be in [1, {_lib.MAX_MEMBERS}]")
        if int(n_particles) != 1 and int(n_members) != 1:
            raise ValueError("particles inside member sets are not batched: n_particles > 1 needs n_members == 1")
        if member_masks is not None:
            # per-member masks (bean_hip_bind_member_masks): checked before the library is touched
            if int(n_members) == 1:
                raise ValueError("member_masks belongs to an ensemble: n_members > 1")
            try:
                m_rg, m_sm = member_masks
            except (TypeError, ValueError):
                raise ValueError("member_masks is a pair (repguide (K, R, G) bool, sample_mask (K, R, B))") from None
            m_rg, m_sm = torch.as_tensor(m_rg), torch.as_tensor(m_sm)
            want_rg = (int(n_members), data.n_reps, data.n_guides)
            want_sm = (int(n_members), data.n_reps, data.n_condits)
            if tuple(m_rg.shape) != want_rg or tuple(m_sm.shape) != want_sm:
                raise ValueError(f"member_masks: repguide {tuple(m_rg.shape)} / sample_mask {tuple(m_sm.shape)} for "
                                 f"{int(n_members)} members, expected {want_rg} / {want_sm}")
        if member_counts is not None:
            # per-member counts (bean_hip_bind_member_counts): checked before the library is touched
            if int(n_members) == 1:
                raise ValueError("member_counts belongs to an ensemble: n_members > 1")
            try:
                m_x, m_xbc = member_counts
            except (TypeError, ValueError):
                raise ValueError("member_counts is a pair (X (K, R, B, G) float32, X_bcmatch (K, R, B, G) float32 or None)") from None
            want_x = (int(n_members), data.n_reps, data.n_condits, data.n_guides)
            needs_bc = bool(use_bcmatch) and getattr(data, "X_bcmatch_masked", None) is not None
            if (m_xbc is not None) != needs_bc:
                raise ValueError("member_counts: X_bcmatch goes with a fit that uses the barcode-matched counts "
                                 f"(this one {'does' if needs_bc else 'does not'}), got "
                                 f"{'None' if m_xbc is None else 'an array'}")
            for name, t in (("X", m_x), ("X_bcmatch", m_xbc)):
                if t is None:
                    continue
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                    raise ValueError(f"member_counts: {name} must be a float32 tensor, got "
                                     f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
                if tuple(t.shape) != want_x:
                    raise ValueError(f"member_counts: {name} {tuple(t.shape)} for {int(n_members)} members, expected {want_x}")
        survival = getattr(data, "selection", "sorting") == "survival"
        surv_normal = survival and family == "Normal"
        self.surv_normal = surv_normal
        self.survival = survival
        if not torch.cuda.is_available():
            raise RuntimeError("crispr-bean_amd needs a ROCm GPU: there is no CPU fallback")
        # the register-resident tiling kernels hold 8 alleles per guide (and 8 conditions) in the default
        # build, 16 in the second one, 32 alleles (16 conditions) in the third; more alleles per guide run in
        # the allele-parallel kernels of any build (csrc/bean_tiling_wide.hpp), so only the condition count
        # decides then
        amax = 8
        n_al = int(getattr(data, "n_max_alleles", 2)) if family == "MultiMixtureNormal" else 2
        if (8 < n_al <= 16) or data.n_condits > 8 or n_al > 256:  # (> 256: the wider allele-parallel kernels)
            amax = 16
        if 16 < n_al <= 32:
            amax = 32
        if lib_variant is not None:
            # "ab": libbean_hip_ab.so, the default kernels plus the superseded / opt-in forms the BEAN_HIP_*
            # switches select (A/B measurements, bit-identity tests); 8 alleles / conditions only
            if lib_variant != _lib.AB or amax != 8:
                raise ValueError("lib_variant must be 'ab' (and the screen must fit the 8-allele / 8-condition build)")
            amax = _lib.AB
        self.lib = _lib.load(amax)
        self.device = torch.device(device if device is not None else "cuda:0")
        self.family = family
        self.data = data
        data.validate()
        dev = self.device
        R, B, G = data.n_reps, data.n_condits, data.n_guides
        tiling = family == "MultiMixtureNormal"
        mixture = family in ("MixtureNormal", "MultiMixtureNormal")  # families with a Dirichlet pi site
        acc = bool(scale_by_accessibility) and mixture
        self.scale_by_accessibility = acc
        # tiling: fit_noise=~args.dont_fit_noise is always truthy (bean/model/run.py:416)
        self.fit_noise = (bool(fit_noise) or tiling) and acc
        has_bc = getattr(data, "X_bcmatch_masked", None) is not None
        self.use_bcmatch = bool(use_bcmatch) and has_bc
        if mixture and not has_bc:
            raise ValueError("MixtureNormal needs barcode-matched counts (X_bcmatch)")
        T = 1 if family == "ControlNormal" else (data.n_edits if tiling else data.n_targets)
        self.T = T
        A = int(data.n_max_alleles) if tiling else 2
        self.A = A
        nnz = 0
        if tiling:
            toff = g2t = None
            max_len = 0
            a2e_ptr = data.a2e_ptr.cpu().to(torch.int32)
            a2e_idx = data.a2e_idx.cpu().to(torch.int32)
            nnz = int(a2e_idx.numel())
            # transpose: edit -> allele slots containing it (stable, so sums keep a fixed order)
            rows = torch.repeat_interleave(
                torch.arange(a2e_ptr.numel() - 1, dtype=torch.int64), (a2e_ptr[1:] - a2e_ptr[:-1]).to(torch.int64))
            order = torch.argsort(a2e_idx.to(torch.int64), stable=True)
            e2a_idx = rows[order].to(torch.int32)
            counts = torch.bincount(a2e_idx.to(torch.int64), minlength=T)
            e2a_ptr = torch.zeros(T + 1, dtype=torch.int32)
            e2a_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
        elif family == "ControlNormal":
            toff = torch.tensor([0, G], dtype=torch.int32)
            g2t = torch.zeros(G, dtype=torch.int32)
            max_len = G
        else:
            off64 = data.target_offsets.cpu()
            toff = off64.to(torch.int32)
            g2t = data.guide_to_target.cpu()
            max_len = int(data.target_lengths.max())
        flags = 0
        if self.use_bcmatch:
            flags |= _lib.FLAG_USE_BCMATCH
        if acc:
            flags |= _lib.FLAG_SCALE_BY_ACC
        if self.fit_noise:
            flags |= _lib.FLAG_FIT_NOISE
        if dump_noise:
            flags |= _lib.FLAG_DUMP_PI
        if not loss_owner:
            flags |= _lib.FLAG_NOT_LOSS_OWNER
        # sample covariates (uns["sample_covariates"], data_class.py:75-92): only the sorting NormalModel
        # has the mu_cov site (model.py:73-91, 771-783); with any other family the reference fits with
        # the regrouped replicates and then fails in write_result_table (readwrite.py:88-90)
        covs = getattr(data, "sample_covariates", None)
        self.n_cov = 0
        if covs is not None and family == "ControlNormal":
            # the reference's ControlNormalModel / Guide have no mu_cov site (model.py:168-252, 861-875): the
            # negative-control fit of a screen with sample covariates just sees the regrouped
            # (replicate, covariate) replicates
            covs = None
        if covs is not None:
            if not (family == "Normal" and not survival):
                raise ValueError(
                    "this screen carries uns['sample_covariates']: only the sorting Normal model (--uniform-edit) "
                    f"models them (bean/model/model.py:73-91); the {family} family cannot write its result table "
                    "in the reference (readwrite.py:88-90) and is refused here")
            self.n_cov = int(data.n_sample_covariates)
        self.prior_params = prior_params
        if prior_params is not None and ("mu_loc" in prior_params or "mu_scale" in prior_params):
            flags |= _lib.FLAG_PRIOR_NORMAL_MU
        # survival NormalModel: prior_params["initial_abundance"] replaces the ones / G prior concentration of
        # the Dirichlet-over-guides site (survival_model.py:38-49); float32 values as the reference holds them
        prior_ia, prior_ia_total = None, 0.0
        if surv_normal and prior_params is not None and "initial_abundance" in prior_params:
            full = torch.as_tensor(prior_params["initial_abundance"]).detach().cpu().to(torch.float32).double().reshape(-1)
            g_all = int(n_guides_total) if n_guides_total else G
            if full.numel() != g_all:
                raise ValueError(f"prior_params['initial_abundance'] has {full.numel()} entries for {g_all} guides")
            if not bool((full > 0).all()):
                raise ValueError("prior_params['initial_abundance'] must be positive")
            prior_ia = full[int(guide_offset): int(guide_offset) + G]
            prior_ia_total = float(full.sum())
        self.num_steps = int(num_steps)
        self.lrd = float(gamma) ** (1.0 / self.num_steps)
        self.initial_lr = float(initial_lr)
        n_ctrl = int(data.allele_counts_control.shape[1]) if mixture else 0
        if survival and family == "ControlNormal":
            flags |= _lib.FLAG_PRIOR_NORMAL_MU  # mu_targets ~ Normal(0, 1) (survival_model.py:142)
        shape = _lib.bean_hip_shape(
            family=_lib.FAMILY[family], selection=1 if survival else 0, flags=flags, n_reps=R, n_condits=B, n_guides=G,
            n_targets=T, n_max_alleles=A, n_edits=T if tiling else 0, n_ctrl=n_ctrl, mask_thres=int(mask_thres),
            max_target_len=max_len, guide_offset=int(guide_offset), target_offset=int(target_offset),
            n_guides_total=int(n_guides_total), n_a2e_nnz=nnz,
            # the reference holds the prior scale in a float32 tensor (model.py:406)
            sd_prior_scale=1.0 if family == "ControlNormal" else float(np.float32(sd_scale)),
            initial_lr=self.initial_lr, lrd=self.lrd, clip_norm=10.0,
            negctrl_loc=float(mu_negctrl[0]), negctrl_scale=float(mu_negctrl[1]),
            n_sample_covariates=self.n_cov,
            prior_ia_total=prior_ia_total,
        )
        self._shape = shape
        handle = ctypes.c_void_p()
        with torch.cuda.device(dev):
            self._check(self.lib.bean_hip_create(ctypes.byref(shape), ctypes.byref(handle)), "create")
        self._h = handle
        # seed ensemble: K fits of this screen stepped by the same launches (bean_hip_svi_run_ensemble); parameters,
        # moments, gradients and the loss history get a leading member axis.  1: the single-fit engine.
        self.n_members = int(n_members)
        if self.n_members != 1:
            if not 1 <= self.n_members <= _lib.MAX_MEMBERS:
                self.lib.bean_hip_destroy(self._h)
                self._h = None
                raise ValueError(f"n_members must be in [1, {_lib.MAX_MEMBERS}]")
            if not (self.ensemble_supported or self.survival_members_supported):
                self.lib.bean_hip_destroy(self._h)
                self._h = None
                raise EnsembleUnsupported(f"the batched kernels do not take this shape ({family}): fit its seeds one "
                                          "after the other (run_inference_ensemble does)")
            with torch.cuda.device(dev):
                self._check(self.lib.bean_hip_set_members(self._h, self.n_members), "set_members")
        # multi-particle SVI (run_particles): P draws per step, one update with their mean gradient.  Where the batched
        # kernels take the shape the library steps the particles in the same launches (bean_hip_svi_run_particles);
        # everywhere else run_particles drives the defining loop itself.  Every tensor keeps its single-fit shape.
        # (One particle goes the same way: run_particles is then run() in the particle step's four launches.)
        self.n_particles = int(n_particles)
        self._particles_native = False
        # (a library named by BEAN_HIP_LIB may be an older build without the entry points: _lib.ENSEMBLE_SYMBOLS)
        if self.n_members == 1 and hasattr(self.lib, "bean_hip_set_particles") and self.ensemble_supported:
            with torch.cuda.device(dev):
                self._check(self.lib.bean_hip_set_particles(self._h, self.n_particles), "set_particles")
            self._particles_native = True
        self._keep: Dict[str, torch.Tensor] = {}
        self.stream = torch.cuda.Stream(device=dev)

        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        f64 = lambda t: t.to(dev, torch.float64).contiguous()
        self._bind("X", f32(data.X_masked))
        self._bind("REPGUIDE", data.repguide_mask.to(dev, torch.uint8).contiguous())
        self._bind("SIZE_FACTOR", f64(data.size_factor))
        self._bind("SAMPLE_MASK", f64(data.sample_mask))
        self._bind("A0", f64(data.a0))
        if survival:
            self._bind("TIMEPOINTS", f64(data.timepoints))
            if surv_normal:
                # `mu[data.negctrl_guide_idx, :] = 0.0` (survival_model.py:59-60); indexing with None
                # (no index given) zeroes every row there, which is kept
                negmask = torch.zeros(G, dtype=torch.uint8)
                idx = getattr(data, "negctrl_guide_idx", None)
                if idx is None:
                    negmask[:] = 1
                else:
                    negmask[torch.as_tensor(np.asarray(idx), dtype=torch.int64)] = 1
                self._bind("NEGCTRL_MASK", negmask.to(dev).contiguous())
            if mixture:
                if int(data.control_timepoint.numel()) != n_ctrl:
                    raise ValueError("control_timepoint must list one time per control condition")
                self._bind("CONTROL_TIME", f64(data.control_timepoint))
            if family == "MixtureNormal":
                # observed initial abundance (survival_model.py:310), formed in float32 as the reference does
                x_t0 = data.X[:, 0, :].to(torch.float32) + 1
                if n_guides_total and n_guides_total != G:
                    # guide shard: the normaliser is the whole screen's (R,) total of X[:, 0, :] + 1
                    if t0_totals is None:
                        raise ValueError("a guide-sharded survival fit needs t0_totals (all-reduced sums of X[:, 0, :] + 1)")
                    tot0 = torch.as_tensor(t0_totals).to(torch.float32).reshape(-1, 1).to(x_t0.device)
                else:
                    tot0 = x_t0.sum(-1, keepdim=True)
                obs0 = x_t0 / tot0
                self._bind("LOG_OBS0", f64(torch.log(obs0.double())))
        else:
            z_hi, z_lo = _quantile_edges(data.upper_bounds, data.lower_bounds)
            self._bind("Z_HI", f64(z_hi))
            self._bind("Z_LO", f64(z_lo))
        # tiling: `data` may hold the guides in another order than the caller's screen (parallel.order_by_alleles);
        # guide_ids[i] is then the index of this engine's guide i in the WHOLE screen.  It keys the guide's random
        # streams (same draws as the screen order), and constrained() hands per-guide values back in screen order.
        self.guide_order = None
        if guide_ids is not None:
            if not tiling:
                raise ValueError("guide_ids: only the tiling family takes its guides in another order")
            gi = torch.as_tensor(guide_ids).to(torch.int64).cpu().reshape(-1)
            local = gi - int(guide_offset)
            if gi.numel() != G or not torch.equal(torch.sort(local).values, torch.arange(G)):
                raise ValueError("guide_ids must be a permutation of guide_offset ... guide_offset + n_guides - 1")
            self.guide_order = local.to(dev)
            self._bind("GUIDE_IDS", gi.to(torch.int32).to(dev).contiguous())
        if tiling:
            self._bind("A2E_PTR", a2e_ptr.to(dev).contiguous())
            self._bind("E2A_PTR", e2a_ptr.to(dev).contiguous())
            if nnz:
                self._bind("A2E_IDX", a2e_idx.to(dev).contiguous())
                self._bind("E2A_IDX", e2a_idx.to(dev).contiguous())
            self._bind("ALLELE_MASK", data.allele_mask.to(dev, torch.uint8).contiguous())
        else:
            self._bind("TARGET_OFFSETS", toff.to(dev).contiguous())
            self._bind("GUIDE_TO_TARGET", g2t.to(dev).contiguous())
        if self.use_bcmatch:
            self._bind("X_BC", f32(data.X_bcmatch_masked))
            self._bind("SIZE_FACTOR_BC", f64(data.size_factor_bcmatch))
            self._bind("A0_BC", f64(data.a0_bcmatch))
        if mixture:
            self._bind("ALLELE_CTRL", f32(data.allele_counts_control))
            self._bind("PI_A0", f64(data.pi_a0))
        if prior_ia is not None:
            self._bind("PRIOR_IA", f64(prior_ia))
        if self.n_cov:
            self._bind("REP_BY_COV", f64(torch.as_tensor(data.rep_by_cov).reshape(R, self.n_cov)))
        if acc:
            if data.guide_accessibility is None:
                raise ValueError("scale_by_accessibility needs data.guide_accessibility")
            self._bind("ACCESSIBILITY", f64(data.guide_accessibility))
        if prior_params is not None:
            for key, slot in (("mu_loc", "PRIOR_MU_LOC"), ("mu_scale", "PRIOR_MU_SCALE"),
                              ("sd_loc", "PRIOR_SD_LOC"), ("sd_scale", "PRIOR_SD_SCALE")):
                if key in prior_params:
                    v = torch.as_tensor(prior_params[key], dtype=torch.float64).reshape(-1)
                    if v.numel() == 1:
                        v = v.expand(T)
                    elif v.numel() != T:
                        # guide shard of a target-aligned fit: the caller holds the whole screen's
                        # per-target priors (`--prior-params`); this rank's targets are
                        # [target_offset, target_offset + T).  (Tiling shards replicate the per-edit
                        # parameters, so T is the whole edit count there and nothing is cut.)
                        if tiling or v.numel() < int(target_offset) + T:
                            raise ValueError(f"prior_params[{key!r}] has {v.numel()} entries, expected {T}"
                                             + ("" if tiling else f" (or at least {int(target_offset) + T} "
                                                                  "for this shard)"))
                        v = v[int(target_offset): int(target_offset) + T]
                    self._bind(slot, f64(v))

        # ---- parameters (unconstrained), as pyro.param initialises them
        pshape = () if family == "ControlNormal" else ((T,) if tiling else (T, 1))
        init = {"mu_loc": torch.zeros(pshape), "mu_scale": torch.zeros(pshape)}
        if not survival:  # survival models have no sd latent (bean/cli/run.py:305)
            init["sd_loc"] = torch.zeros(pshape)
            init["sd_scale"] = torch.zeros(pshape)
        if survival and family == "MixtureNormal":  # q0 = ones(G) / G over the WHOLE screen (survival_model.py:660-664)
            g_all = int(n_guides_total) if n_guides_total else G
            init["q0"] = torch.full((G,), float(np.log(np.float32(1.0) / np.float32(g_all))))
        if surv_normal:  # initial_abundance = ones(G) / G over the WHOLE screen (survival_model.py:630-634)
            g_all = int(n_guides_total) if n_guides_total else G
            init["initial_abundance"] = torch.full((G,), float(np.log(np.float32(1.0) / np.float32(g_all))))
        if mixture:
            # pyro.param("alpha_pi", ones * alpha_prior) in the guide, which runs first
            # (model.py:820-830, 927-937)
            if not float(alpha_prior) > 0:
                raise ValueError("alpha_prior must be positive")
            init["alpha_pi"] = torch.full((G, A), float(np.log(np.float32(alpha_prior))))
            if tiling:  # alpha_pi0[~allele_mask] = epsilon (model.py:643)
                init["alpha_pi"][~data.allele_mask.cpu()] = float(np.log(1e-5))
        if self.fit_noise:
            init["noise_loc"] = torch.zeros(G)
            init["noise_scale"] = torch.full((G,), float(np.log(PI_NOISE_SD)))
        if self.n_cov:  # mu_cov_loc = 0, mu_cov_scale = 1 (model.py:773-780)
            init["mu_cov_loc"] = torch.zeros(self.n_cov)
            init["mu_cov_scale"] = torch.zeros(self.n_cov)
        self.unconstrained: Dict[str, torch.Tensor] = {}
        self.grads: Dict[str, torch.Tensor] = {}
        self._m: Dict[str, torch.Tensor] = {}
        self._v: Dict[str, torch.Tensor] = {}
        order = list(_lib.PARAM_ORDER)
        if surv_normal:
            order[order.index("q0")] = "initial_abundance"  # same slot: a positive (G,) Dirichlet concentration
        if self.n_cov:  # the noise slots are free in the Normal family (include/bean_hip.h)
            order[order.index("noise_loc")] = "mu_cov_loc"
            order[order.index("noise_scale")] = "mu_cov_scale"
        for i, name in enumerate(order):
            if name not in init:
                continue
            p = init[name].to(dev, torch.float32).contiguous()
            if self.n_members != 1:  # member-major: every member starts from the single fit's initial values
                p = p.unsqueeze(0).repeat(self.n_members, *([1] * p.dim())).contiguous()
            self.unconstrained[name] = p
            self.grads[name] = torch.zeros_like(p)
            self._m[name] = torch.zeros_like(p)
            self._v[name] = torch.zeros_like(p)
            self._bind_slot(_lib.BUF["P"] + i, p, f"P.{name}")
            self._bind_slot(_lib.BUF["G"] + i, self.grads[name], f"G.{name}")
            self._bind_slot(_lib.BUF["M"] + i, self._m[name], f"M.{name}")
            self._bind_slot(_lib.BUF["V"] + i, self._v[name], f"V.{name}")
        cap = int(loss_capacity) if loss_capacity is not None else self.num_steps + 8
        self.loss_hist = torch.zeros(max(cap, 1) if self.n_members == 1 else (self.n_members, max(cap, 1)),
                                     dtype=torch.float64, device=dev)
        self._loss_all = self.loss_hist
        if self.n_particles != 1 and not self._particles_native:
            # the defining loop evaluates every particle into a spare slot BEHIND the history, which only ever holds means
            self._loss_all = torch.zeros(max(cap, 1) + 1, dtype=torch.float64, device=dev)
            self.loss_hist = self._loss_all[:-1]
        self._bind("LOSS_HIST", self._loss_all)
        self._noise_out: Dict[str, torch.Tensor] = {}
        if dump_noise:
            self._noise_out["eps_mu"] = torch.zeros(T, dtype=torch.float64, device=dev)
            self._bind("EPS_MU_OUT", self._noise_out["eps_mu"])
            if not survival:
                self._noise_out["eps_sd"] = torch.zeros(T, dtype=torch.float64, device=dev)
                self._bind("EPS_SD_OUT", self._noise_out["eps_sd"])
            if survival and mixture:
                self._noise_out["eps_u"] = torch.zeros(G, dtype=torch.float64, device=dev)
                self._bind("EPS_U_OUT", self._noise_out["eps_u"])
            if survival and family == "MixtureNormal":
                self._noise_out["initial_abundance"] = torch.zeros((R, G), dtype=torch.float64, device=dev)
                self._bind("X0_OUT", self._noise_out["initial_abundance"])
            if surv_normal:
                self._noise_out["q_0"] = torch.zeros((R, G), dtype=torch.float64, device=dev)
                self._bind("X0_OUT", self._noise_out["q_0"])
            if mixture:
                self._noise_out["pi"] = torch.zeros((R, G, A), dtype=torch.float64, device=dev)
                self._bind("PI_OUT", self._noise_out["pi"])
            if acc:
                self._noise_out["eps_noise"] = torch.zeros(G, dtype=torch.float64, device=dev)
                self._bind("EPS_NOISE_OUT", self._noise_out["eps_noise"])
            if self.n_cov:
                self._noise_out["eps_cov"] = torch.zeros(self.n_cov, dtype=torch.float64, device=dev)
                self._bind("EPS_NOISE_OUT", self._noise_out["eps_cov"])
        self.steps_done = 0
        self.member_masks = member_masks is not None
        if member_masks is not None:
            # member k reads its (R, G) / (R, B) slice where a single fit reads REPGUIDE / SAMPLE_MASK
            rg_k = (m_rg != 0).to(dev, torch.uint8).contiguous()
            sm_k = f64(m_sm)
            self._keep["MEMBER_REPGUIDE"], self._keep["MEMBER_SAMPLE_MASK"] = rg_k, sm_k
            self._check(self.lib.bean_hip_bind_member_masks(
                self._h, ctypes.c_void_p(rg_k.data_ptr()), rg_k.numel(), ctypes.c_void_p(sm_k.data_ptr()),
                sm_k.numel() * 8), "bind_member_masks")
        self.member_counts = member_counts is not None
        if member_counts is not None:
            # member k reads its (R, B, G) slice where a single fit reads X / X_BC
            x_k = f32(m_x)
            xbc_k = None if m_xbc is None else f32(m_xbc)
            self._keep["MEMBER_X"], self._keep["MEMBER_X_BC"] = x_k, xbc_k
            self._check(self.lib.bean_hip_bind_member_counts(
                self._h, ctypes.c_void_p(x_k.data_ptr()), x_k.numel() * 4,
                None if xbc_k is None else ctypes.c_void_p(xbc_k.data_ptr()), 0 if xbc_k is None else xbc_k.numel() * 4),
                "bind_member_counts")
        with self._on_stream():
            self._check(self.lib.bean_hip_prepare(self._h, self._sptr()), "prepare")

    # -------------------------------------------------------------- plumbing
    def _check(self, status: int, what: str = ""):
        _lib.check(status, what, self.lib)

    def _bind(self, slot_name: str, t: torch.Tensor):
        self._bind_slot(_lib.BUF[slot_name], t, slot_name)

    def _bind_slot(self, slot: int, t: Optional[torch.Tensor], key: str):
        if t is None:
            self._keep.pop(key, None)
            self._check(self.lib.bean_hip_bind(self._h, slot, None, 0), f"bind {key}")
            return
        assert t.is_cuda and t.is_contiguous(), key
        self._keep[key] = t
        self._check(
            self.lib.bean_hip_bind(self._h, slot, ctypes.c_void_p(t.data_ptr()), t.numel() * t.element_size()),
            f"bind {key}",
        )

    def _sptr(self):
        return ctypes.c_void_p(self.stream.cuda_stream)

    class _StreamScope:
        def __init__(self, eng):
            self.eng = eng

        def __enter__(self):
            self.eng.stream.wait_stream(torch.cuda.current_stream(self.eng.device))
            return self

        def __exit__(self, *exc):
            torch.cuda.current_stream(self.eng.device).wait_stream(self.eng.stream)
            return False

    def _on_stream(self):
        return HipSVI._StreamScope(self)

    # ------------------------------------------------- guide-sharded stepping
    def exchange_buffers(self) -> Dict[str, torch.Tensor]:
        """Allocate and bind the exchange buffers this family needs when its guides are sharded
        over ranks (``bean_hip_sharded_*``): ``gsum`` (survival MixtureNormal) and/or ``tgrad``
        (ControlNormal, tiling).  Empty for the families that need no exchange."""
        if getattr(self, "_xchg", None) is None:
            self._xchg = {}
            R = self.data.n_reps
            # what is exchanged BEHIND the guide kernel lives in one allocation, so a step's post-guide exchange is
            # ONE all-reduce whatever the family (tgrad | sq | cov are views of `_xchg_post`)
            sizes = []
            if self.family in ("ControlNormal", "MultiMixtureNormal"):
                sizes.append(("tgrad", 2 * self.T, "XCHG_TGRAD"))
            if self.surv_normal:
                sizes.append(("sq", R, "XCHG_SQ"))
            if self.n_cov and int(self._shape.n_guides_total) not in (0, self.data.n_guides):
                # guide shard of a screen with sample covariates: mu_cov is shared by every guide
                sizes.append(("cov", R, "XCHG_COV"))
            self._xchg_post = None
            if sizes:
                self._xchg_post = torch.zeros(sum(n for _, n, _ in sizes), dtype=torch.float64, device=self.device)
                at = 0
                for name, n, slot in sizes:
                    self._xchg[name] = self._xchg_post[at:at + n]
                    self._bind(slot, self._xchg[name])
                    at += n
            if self.survival and self.family in ("MixtureNormal", "Normal"):
                self._xchg["gsum"] = torch.zeros(R + 1, dtype=torch.float64, device=self.device)
                self._bind("XCHG_GSUM", self._xchg["gsum"])
        return self._xchg

    def init_native_comm(self, group=None) -> bool:
        """Give the library its own RCCL communicator over the ranks of ``group`` (default group when
        None), so that ``run_exchanged`` steps without the host in the loop
        (``bean_hip_svi_run_exchanged``: kernels and ``ncclAllReduce`` enqueued by the library on the
        engine's stream).  Collective: every rank of the group must call it.  Only with the ``nccl``
        backend (the unique id travels by a ``torch.distributed`` broadcast); returns False - and the
        Python stepping loop stays in use - on any other backend or if RCCL refuses."""
        import torch.distributed as dist

        if getattr(self, "_native_comm", False):
            return True
        if not (dist.is_available() and dist.is_initialized()) or dist.get_backend(group) != "nccl":
            return False
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        path = _lib.rccl_path().encode()
        idt = torch.zeros(128, dtype=torch.uint8, device=self.device)
        # EVERY rank loads RCCL now (asking for an id does that; only rank 0's id is used) and the ranks agree
        # on the outcome BEFORE anyone enters ncclCommInitRank: a rank that could not load the library would
        # otherwise return while its peers block inside that collective
        buf = (ctypes.c_uint8 * 128)()
        loaded = self.lib.bean_hip_comm_unique_id(path, buf) == 0
        if rank == 0 and loaded:
            idt.copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
        ok = torch.tensor([1 if loaded else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
        if int(ok.item()) == 0:
            return False
        dist.broadcast(idt, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        raw = bytes(idt.cpu().numpy().tobytes())
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(raw)
        self.exchange_buffers()
        with torch.cuda.device(self.device):
            st = self.lib.bean_hip_comm_init(self._h, path, buf, rank, world)
        # all ranks agree on the outcome (a rank that failed alone would leave the others in a collective)
        flag = torch.tensor([1 if st == 0 else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag.item()) == 0:
            if st == 0:
                self.lib.bean_hip_comm_destroy(self._h)
            return False
        # ... and a fit depends on the communicator only after it has summed a known vector right: rank k contributes
        # (k + 1) * (1, 2, ..., n) - every entry of the sum is an exact integer in float64 - through the very call the
        # stepping loop issues (ncclAllReduce, sum, float64, in place, the engine's stream), over a length that takes
        # RCCL through its multi-channel path as the per-edit gradients of a tiling fit do; the ranks agree on the
        # outcome, and on any doubt all of them keep the Python stepping loop
        n = 4099
        probe = torch.arange(1, n + 1, dtype=torch.float64, device=self.device) * (rank + 1)
        with self._on_stream():
            rc = self.lib.bean_hip_comm_all_reduce(self._h, ctypes.c_void_p(probe.data_ptr()), n, self._sptr())
        self.stream.synchronize()
        want = torch.arange(1, n + 1, dtype=torch.float64, device=self.device) * (world * (world + 1) // 2)
        good = rc == 0 and bool(torch.equal(probe, want))
        flag = torch.tensor([1 if good else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        if int(flag.item()) == 0:
            self.lib.bean_hip_comm_destroy(self._h)
            return False
        self._native_comm = True
        return True

    def run_exchanged(self, n_steps: int, all_reduce, seed: int = 101, first_step: Optional[int] = None,
                      graph_chunk: Optional[int] = None):
        """``n_steps`` SVI steps of one guide shard.  With a native communicator (``init_native_comm``)
        the whole loop, collectives included, is enqueued by the library; otherwise the step is driven
        from here and ``all_reduce(tensor)`` must sum the tensor over the ranks in place on the current
        stream (``torch.distributed.all_reduce``).  ``graph_chunk`` > 1 (native path; default from
        ``BEAN_HIP_XCHG_GRAPH``, else 0) replays hipGraphs of that many steps, collectives captured."""
        first = self.steps_done if first_step is None else int(first_step)
        if first + n_steps > self.loss_hist.numel():
            raise ValueError("loss history too small: raise num_steps / loss_capacity")
        x = self.exchange_buffers()
        sp = self._sptr()
        if getattr(self, "_native_comm", False):
            import os

            chunk = int(os.environ.get("BEAN_HIP_XCHG_GRAPH", "0")) if graph_chunk is None else int(graph_chunk)
            with self._on_stream():
                self._check(self.lib.bean_hip_svi_run_exchanged(self._h, int(seed), first, int(n_steps), chunk, sp),
                            "svi_run_exchanged")
            self.last_exchange_path = ("native: kernels + ncclAllReduce enqueued by the library"
                                       + (f", hipGraphs of up to {chunk} steps" if chunk > 1 else ", eager launches"))
            self.steps_done = first + n_steps
            return
        self.last_exchange_path = ("python loop: 3 ctypes calls + at most 2 torch.distributed.all_reduce per step "
                                   "(one in front of the guide kernel, one packed behind it)")
        lib, h = self.lib, self._h
        sums, guide, update = lib.bean_hip_sharded_sums, lib.bean_hip_sharded_guide, lib.bean_hip_sharded_update
        pre, post = x.get("gsum"), self._xchg_post
        with self._on_stream(), torch.cuda.stream(self.stream):
            self._check(lib.bean_hip_sharded_begin(h, int(seed), first, int(n_steps), sp), "sharded_begin")
            for i in range(n_steps):
                rc = sums(h, sp)
                if pre is not None:
                    all_reduce(pre)
                rc |= guide(h, sp)
                if post is not None:
                    all_reduce(post)
                rc |= update(h, 1 if i == n_steps - 1 else 0, sp)
                if rc:
                    self._check(rc, "sharded step (sums / guide / update)")
        self.steps_done = first + n_steps

    # the four phases, for drivers that interleave several engines in one process (tests)
    def phase(self, name: str, *args):
        fn = getattr(self.lib, "bean_hip_sharded_" + name)
        with self._on_stream():
            self._check(fn(self._h, *args, self._sptr()), "sharded_" + name)

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            if getattr(self, "_native_comm", False):
                self.lib.bean_hip_comm_destroy(self._h)
                self._native_comm = False
            self.lib.bean_hip_destroy(self._h)
            self._h = None
            self._plant = None  # (simulate_power's mask: nothing reads it after the synchronisation above)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ operations
    def set_noise(self, noise: Optional[dict]):
        """Inject the draws of the next evaluation(s) (parity tests);
        ``None`` returns to the in-kernel generator."""
        dev = self.device
        names = {"eps_mu": "EPS_MU_IN", "eps_sd": "EPS_SD_IN", "pi": "PI_IN", "eps_noise": "EPS_NOISE_IN",
                 "eps_u": "EPS_U_IN"}
        # the draw of the Dirichlet-over-guides site: `initial_abundance` in the survival MixtureNormal
        # guide, `q_0` (site initial_guide_abundance) in the survival NormalModel
        names["q_0" if self.surv_normal else "initial_abundance"] = "X0_IN"
        if self.n_cov:
            names.pop("eps_noise")
            names["eps_cov"] = "EPS_NOISE_IN"
        if noise is not None and "mu_negctrl" in noise and "eps_u" not in noise:
            m0, s0 = float(np.float32(self._shape.negctrl_loc)), float(np.float32(self._shape.negctrl_scale))
            noise = dict(noise)
            noise["eps_u"] = (torch.as_tensor(noise["mu_negctrl"]).double() - m0) / s0
        for key, slot in names.items():
            t = None if noise is None else noise.get(key)
            if t is None:
                if slot in self._keep:
                    self._bind_slot(_lib.BUF[slot], None, slot)
                continue
            t = torch.as_tensor(t).to(dev, torch.float64)
            if key == "pi":
                t = t.reshape(self.data.n_reps, self.data.n_guides, self.A)
                t = self._to_engine_order(t, 1)
            elif slot == "X0_IN":
                t = self._to_engine_order(t.reshape(self.data.n_reps, self.data.n_guides), 1).reshape(-1)
            else:
                t = t.reshape(-1)
                if key in ("eps_noise", "eps_u"):
                    t = self._to_engine_order(t, 0)
            self._bind(slot, t.contiguous())

    # With guide_ids the engine holds its guides in another order than the caller's screen: engine guide i is the
    # screen's (shard's) guide guide_order[i].  Everything per-guide that crosses this class - injected and exported
    # draws, gradients, constrained() - is in SCREEN order.
    def _to_engine_order(self, t: torch.Tensor, axis: int) -> torch.Tensor:
        return t if self.guide_order is None else t.index_select(axis, self.guide_order)

    def _to_screen_order(self, t: torch.Tensor, axis: int) -> torch.Tensor:
        if self.guide_order is None:
            return t
        return torch.empty_like(t).index_copy_(axis, self.guide_order, t)

    def elbo_grad(self, step: int = 0, seed: int = 101, loss_index: int = 0):
        """One ELBO evaluation: returns ``(loss, {name: grad})`` w.r.t. the
        unconstrained parameters; parameters are not modified."""
        with self._on_stream():
            self._check(
                self.lib.bean_hip_elbo_grad(self._h, int(seed), int(step), int(loss_index), self._sptr()),
                "elbo_grad",
            )
        torch.cuda.synchronize(self.device)
        grads = {k: (self._to_screen_order(v, 0) if k in PER_GUIDE and self.guide_order is not None else v.clone())
                 for k, v in self.grads.items()}
        return float(self.loss_hist[loss_index]), grads

    def drawn_noise(self) -> Dict[str, torch.Tensor]:
        """Draws used by the last evaluation (needs ``dump_noise=True``)."""
        out = {k: v.clone() for k, v in self._noise_out.items()}
        if self.guide_order is not None:  # per-guide draws go back in screen order (see _to_screen_order)
            for k, axis in (("pi", 1), ("eps_noise", 0), ("eps_u", 0), ("initial_abundance", 1), ("q_0", 1)):
                if k in out and not (k == "eps_noise" and self.n_cov):
                    out[k] = self._to_screen_order(out[k], axis)
        if "pi" in out:
            out["pi"] = out["pi"].unsqueeze(1)  # (R, 1, G, A) as the reference shapes it
        if "eps_u" in out:  # the oracle takes the baseline draw itself: u = m0 + s0 * eps (float32 constants)
            m0, s0 = np.float32(self._shape.negctrl_loc), np.float32(self._shape.negctrl_scale)
            out["mu_negctrl"] = float(m0) + out.pop("eps_u") * float(s0)
        if self.family == "MultiMixtureNormal":
            pass  # per-edit draws are 1-D, as the reference shapes them
        elif self.family != "ControlNormal":
            for k in ("eps_mu", "eps_sd"):
                if k in out:
                    out[k] = out[k].reshape(self.T, 1)
        else:
            for k in ("eps_mu", "eps_sd"):
                if k in out:
                    out[k] = out[k].reshape(())
        return out

    def adam(self, t: int):
        with self._on_stream():
            self._check(self.lib.bean_hip_adam(self._h, int(t), self._sptr()), "adam")

    def run(self, n_steps: int, seed: int = 101, graph_chunk: int = 50, first_step: Optional[int] = None,
            resume: bool = False):
        """Enqueue ``n_steps`` fused SVI steps (no host synchronisation).

        ``resume=True`` (``bean_hip_svi_resume``): for a fit stepped in windows.  Same results; a call that
        continues exactly where the previous one ended starts stepping at once (the previous call has left
        the next step's draw and tables on the device).  The caller promises not to write the parameter /
        moment tensors between such calls - ``run_inference`` and ``bench.py`` do not."""
        first = self.steps_done if first_step is None else int(first_step)
        if first + n_steps > self.loss_hist.numel():
            raise ValueError("loss history too small: raise num_steps / loss_capacity")
        # a write to a parameter or moment tensor between two windows (warm start, clamping, a loaded checkpoint)
        # bumps the tensor's version counter - the kernels' own writes do not: the draw and the tables the previous
        # window left on the device belong to the OLD values then, so this window goes through the plain loop, as
        # include/bean_hip.h asks after such a write (the library cannot see it; a first_step / seed that does not
        # continue it does see)
        versions = self._tensor_versions()
        prev = getattr(self, "_resume_versions", None)
        if resume and ((prev is not None and versions != prev) or getattr(self, "_resume_broken", False)):
            resume = False
        self._resume_broken = False
        fn = self.lib.bean_hip_svi_resume if resume else self.lib.bean_hip_svi_run
        with self._on_stream():
            self._check(fn(self._h, int(seed), first, int(n_steps), int(graph_chunk), self._sptr()),
                        "svi_resume" if resume else "svi_run")
        self._resume_versions = versions
        self.steps_done = first + n_steps

    @property
    def ensemble_supported(self) -> bool:
        """Whether the batched kernels take this engine's shape (``bean_hip_ensemble_supported``)."""
        return self.lib.bean_hip_ensemble_supported(self._h) == 1

    @property
    def survival_members_supported(self) -> bool:
        """Whether the survival member kernels take this engine's shape (``bean_hip_survival_members_supported``): the
        survival variant Normal / MixtureNormal families on the wave-form path, unsharded, no sample covariates.  Such an
        engine takes ``n_members``, ``member_masks`` and ``member_counts`` as a sorting one does; ``ensemble_supported``
        stays false for it, and with it the particles stay on the Python loop."""
        fn = getattr(self.lib, "bean_hip_survival_members_supported", None)
        return fn is not None and fn(self._h) == 1

    @property
    def predictive_supported(self) -> bool:
        """Whether the count simulator takes this engine (``bean_hip_predictive_supported``): the sorting variant
        Normal / MixtureNormal families, unsharded, no sample covariates, one member, one particle."""
        fn = getattr(self.lib, "bean_hip_predictive_supported", None)
        return fn is not None and fn(self._h) == 1

    def _require_predictive(self, what: str, grid: bool = False, have: bool = True):
        """Raise ``PredictiveUnsupported`` unless the post-fit kernels take this engine; ``what`` begins the sentence
        ("the count simulator does not take"), ``grid`` also refuses accessibility, ``have`` is whether the library has
        the entry point."""
        acc = grid and self.scale_by_accessibility
        if self.predictive_supported and have and not acc:
            return
        raise PredictiveUnsupported(f"{what} this engine ({self.family}{', survival' if self.survival else ''}"
                                    f"{', accessibility' if acc else ''}): sorting variant Normal / MixtureNormal, "
                                    "unsharded, no sample covariates, one member, one particle"
                                    f"{', no accessibility' if grid else ''}")

    def _simulated(self, lead, call) -> Dict[str, torch.Tensor]:
        """What the simulators end with: ``X`` and, where the fit uses the barcode-matched counts, ``X_bcmatch`` -
        ``lead + (R, B, G)`` float32 - filled by ``call(x, xbc)`` on the engine's stream, and the resume invalidated."""
        shape = tuple(lead) + (self.data.n_reps, self.data.n_condits, self.data.n_guides)
        x = torch.empty(shape, dtype=torch.float32, device=self.device)
        xbc = torch.empty(shape, dtype=torch.float32, device=self.device) if self.use_bcmatch else None
        with self._on_stream():
            call(x, xbc)
        self.invalidate_resume()
        out = {"X": x}
        if xbc is not None:
            out["X_bcmatch"] = xbc
        return out

    def simulate(self, draw: int, seed: int = 101, alphas: bool = False) -> Dict[str, torch.Tensor]:
        """Replicate counts of one posterior draw (``bean_hip_simulate``): the latent sites of
        ``elbo_grad(step=draw, seed=seed)`` at the current parameters, then ``p ~ Dirichlet(alpha)`` and
        ``x_rep ~ Multinomial(n_obs, p)`` for every (replicate, guide).  Returns device tensors: ``X`` (R, B, G)
        float32, ``X_bcmatch`` where the fit uses the barcode-matched counts, and with ``alphas`` the floored
        concentrations ``alpha`` (2, R, B, G) float64.  Parameters, moments, gradients and the loss history are left as
        they are; the next ``run(resume=True)`` is a plain run."""
        self._require_predictive("the count simulator does not take")
        R, B, G = self.data.n_reps, self.data.n_condits, self.data.n_guides
        al = torch.zeros((2, R, B, G), dtype=torch.float64, device=self.device) if alphas else None
        out = self._simulated((), lambda x, xbc: self._check(self.lib.bean_hip_simulate(
            self._h, int(seed), int(draw), _ptr(x), _nbytes(x), _ptr(xbc), _nbytes(xbc), _ptr(al), _nbytes(al),
            self._sptr()), "simulate"))
        if al is not None:
            out["alpha"] = al
        return out

    @property
    def survival_predictive_supported(self) -> bool:
        """Whether the survival count simulator takes this engine (``bean_hip_survival_predictive_supported``): the
        survival variant Normal / MixtureNormal families, unsharded, no sample covariates, one member, one particle."""
        fn = getattr(self.lib, "bean_hip_survival_predictive_supported", None)
        return fn is not None and fn(self._h) == 1

    def simulate_survival(self, draw: int, seed: int = 101, alphas: bool = False) -> Dict[str, torch.Tensor]:
        """Replicate counts of one posterior draw of a survival screen (``bean_hip_simulate_survival``): the latent
        sites of ``elbo_grad(step=draw, seed=seed)`` at the current parameters - injected noise honoured, and
        ``drawn_noise()`` afterwards that of this draw - then ``p ~ Dirichlet(alpha)`` over the timepoints and
        ``x_rep ~ Multinomial(n_obs, p)`` for every (replicate, guide).  Returns what ``simulate`` returns: ``X``
        (R, B, G) float32, ``X_bcmatch`` where the fit uses the barcode-matched counts, and with ``alphas`` the floored
        concentrations ``alpha`` (2, R, B, G) float64.  Parameters, moments, gradients and the loss history are left as
        they are; the next ``run(resume=True)`` is a plain run."""
        if not self.survival_predictive_supported:
            raise PredictiveUnsupported(f"the survival count simulator does not take this engine ({self.family}"
                                        f"{', survival' if self.survival else ', sorting'}): survival variant Normal / "
                                        "MixtureNormal, unsharded, no sample covariates, one member, one particle")
        R, B, G = self.data.n_reps, self.data.n_condits, self.data.n_guides
        al = torch.zeros((2, R, B, G), dtype=torch.float64, device=self.device) if alphas else None
        out = self._simulated((), lambda x, xbc: self._check(self.lib.bean_hip_simulate_survival(
            self._h, int(seed), int(draw), _ptr(x), _nbytes(x), _ptr(xbc), _nbytes(xbc), _ptr(al), _nbytes(al),
            self._sptr()), "simulate_survival"))
        if al is not None:
            out["alpha"] = al
        return out

    def simulate_survival_members(self, first_draw: int, n_draws: int, seed: int = 101) -> Dict[str, torch.Tensor]:
        """``n_draws`` replicate screens of a survival fit in one launch (``bean_hip_simulate_survival_members``): ``X``
        (K, R, B, G) float32 and, where the fit uses the barcode-matched counts, ``X_bcmatch`` - device tensors,
        member-major.  The per-target and per-guide Normal sites and the Dirichlet-over-all-guides site are those of
        draw ``first_draw`` (or the injected ones, ``set_noise``) for every member; member k's baseline ``u_g`` (unless
        ``eps_u`` is injected: then that value for every member), pi, Dirichlet and categorical draws are those of draw
        ``first_draw + k``: plane 0 is ``simulate_survival(first_draw)``, and with the shared sites injected plane k is
        ``simulate_survival(first_draw + k)``, bit for bit.  Leaves the fit alone as ``simulate_survival`` does; the
        next ``run(resume=True)`` is a plain run."""
        if not self.survival_predictive_supported or not hasattr(self.lib, "bean_hip_simulate_survival_members"):
            raise PredictiveUnsupported(f"the survival count simulator does not take this engine ({self.family}"
                                        f"{', survival' if self.survival else ', sorting'}): survival variant Normal / "
                                        "MixtureNormal, unsharded, no sample covariates, one member, one particle")
        K = int(n_draws)
        return self._simulated((max(K, 0),), lambda x, xbc: self._check(self.lib.bean_hip_simulate_survival_members(
            self._h, int(seed), int(first_draw), K, _ptr(x), _nbytes(x), _ptr(xbc), _nbytes(xbc), self._sptr()),
            "simulate_survival_members"))

    def simulate_members(self, first_draw: int, n_draws: int, seed: int = 101) -> Dict[str, torch.Tensor]:
        """``n_draws`` replicate screens in one launch (``bean_hip_simulate_members``): ``X`` (K, R, B, G) float32 and,
        where the fit uses the barcode-matched counts, ``X_bcmatch`` - device tensors, member-major, what
        ``HipSVI(member_counts=...)`` binds.  The per-target and per-guide Normal sites are those of draw ``first_draw``
        (or the injected ones, ``set_noise``) for every member; member k's pi, Dirichlet and categorical draws are
        those of draw ``first_draw + k``: plane 0 is ``simulate(first_draw)``, and with every Normal site injected plane
        k is ``simulate(first_draw + k)``, bit for bit.  Leaves the fit alone as ``simulate`` does; the next
        ``run(resume=True)`` is a plain run."""
        self._require_predictive("the count simulator does not take")
        K = int(n_draws)
        return self._simulated((max(K, 0),), lambda x, xbc: self._check(self.lib.bean_hip_simulate_members(
            self._h, int(seed), int(first_draw), K, _ptr(x), _nbytes(x), _ptr(xbc), _nbytes(xbc), self._sptr()),
            "simulate_members"))

    def simulate_design(self, first_draw: int, n_draws: int, depths, seed: int = 101) -> Dict[str, torch.Tensor]:
        """``n_draws`` replicate screens at each of the read depths ``depths`` in one launch
        (``bean_hip_simulate_design``): ``X`` (D, K, R, B, G) float32 and, where the fit uses the barcode-matched counts,
        ``X_bcmatch`` - device tensors, member-major over (depth, draw).  Plane (i, j) is plane j of
        ``simulate_members(first_draw, n_draws)`` drawn with ``floor(depths[i] * n_obs + 0.5)`` reads per (replicate,
        guide) instead of ``n_obs``: the same pi, Dirichlet and categorical streams at every depth, so depth 1 is that
        plane bit for bit and a deeper screen is the shallower one plus further reads.  A depth under which the largest
        observed total would reach 2^24 reads (the categorical window, and the limit of exact float32 counts) is a
        ``ValueError`` before any launch.  Leaves the fit alone as ``simulate`` does; the next ``run(resume=True)`` is a
        plain run."""
        self._require_predictive("the count simulator does not take")
        K = int(n_draws)
        fs = [float(f) for f in depths]
        D = len(fs)
        finite = [f for f in fs if f == f and f != float("inf")]
        if finite:
            if getattr(self, "_largest_total", None) is None:  # read back once: the bound counts do not change
                keys = ("X", "X_BC") if self.use_bcmatch else ("X",)
                self._largest_total = max(float(self._keep[k].double().sum(1).max()) for k in keys)
            most = self._largest_total
            if max(finite) * most >= float(1 << 24):
                raise ValueError(f"simulate_design: depth {max(finite):g} times the largest observed total {most:.0f} is "
                                 f"{max(finite) * most:.0f} reads, not below 2^24 = {1 << 24} (the categorical window of "
                                 "a pair, and the limit of exact float32 counts)")
        arr = (ctypes.c_double * max(D, 1))(*fs)
        return self._simulated((D, max(K, 0)), lambda x, xbc: self._check(self.lib.bean_hip_simulate_design(
            self._h, int(seed), int(first_draw), K, arr, D, _ptr(x), _nbytes(x), _ptr(xbc), _nbytes(xbc), self._sptr()),
            "simulate_design"))

    def simulate_power(self, first_draw: int, n_draws: int, effects, plant=None, seed: int = 101) -> Dict[str, torch.Tensor]:
        """``n_draws`` replicate screens at each of the planted effects ``effects`` in one launch
        (``bean_hip_simulate_power``): ``X`` (D, K, R, B, G) float32 and, where the fit uses the barcode-matched counts,
        ``X_bcmatch`` - device tensors, member-major over (effect, draw).  Plane (i, j) is plane j of
        ``simulate_members(first_draw, n_draws)`` with ``mu_t = effects[i]`` - the value itself, not a shift of the fitted
        mean - on every planted target: the same pi, Dirichlet and categorical streams at every effect, the drawn ``sd``
        and every guide-level quantity as they are.  ``plant``: ``None`` (every target) or T booleans / uint8 (tensor or
        array; non-zero: planted), moved to the device as uint8 and held by the engine until the next call or ``close()``;
        any other length is a ``ValueError``.  With nothing planted the planes are those of ``simulate_members`` bit for
        bit, and the guides of unplanted targets are in every plane.  Leaves the fit alone as ``simulate`` does; the next
        ``run(resume=True)`` is a plain run."""
        self._require_predictive("the count simulator does not take")
        K = int(n_draws)
        es = [float(e) for e in effects]
        D = len(es)
        T = int(self.T)
        mask = None
        if plant is not None:
            mask = torch.as_tensor(plant)
            if mask.dim() != 1 or int(mask.numel()) != T or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"simulate_power: plant must be None or {T} booleans / uint8 (one per target), got "
                                 f"{mask.dtype} of shape {tuple(mask.shape)}")
        arr = (ctypes.c_double * max(D, 1))(*es)

        def call(x, xbc):
            # the launch reads the mask: kept alive until the next call or close()
            self._plant = None if mask is None else mask.to(self.device).to(torch.uint8).contiguous()
            self._check(self.lib.bean_hip_simulate_power(self._h, int(seed), int(first_draw), K, arr, D, _ptr(self._plant),
                                                         _ptr(x), _nbytes(x), _ptr(xbc), _nbytes(xbc), self._sptr()),
                        "simulate_power")

        return self._simulated((D, max(K, 0)), call)

    LOGW_PAIR_BYTES = 256 << 20  # the pair plane of one bean_hip_log_weights call stays at or below this

    def log_weights(self, first_draw: int, n_draws: int, seed: int = 101, pairs: bool = False,
                    integrate_pi: Optional[int] = None, tail_rule: bool = False) -> Dict[str, torch.Tensor]:
        """Per-target log importance weights of ``n_draws`` draws from the guide at the current parameters
        (``bean_hip_log_weights``): draw ``first_draw + j`` is the draw ``elbo_grad(step=first_draw + j, seed=seed)``
        evaluates (or, with ``set_noise``, the injected draw every time).  Returns float64 device tensors ``logw``
        (n_draws, T) - ``log p(x_t, z_t) - log q(z_t)``, whose negative sum over targets is that ``elbo_grad``'s loss -
        ``mu`` and ``y`` (n_draws, T), the drawn ``mu_t`` and ``log sd_t``, and with ``pairs`` the terms of every
        (draw, replicate, guide) pair, ``pairs`` (n_draws, R, G), guides in screen order.  The draws go to the library in
        chunks whose pair plane stays at or below 256 MiB; draw d is the same whatever the chunking.  Leaves the fit alone
        as ``simulate`` does; the next ``run(resume=True)`` is a plain run.

        ``integrate_pi=Q`` (16, 32 or 64; ``bean_hip_log_weights_marginal``): ``logw`` is the weight of ``(mu_t, sd_t)``
        alone - ``pi`` integrated out of the model by Q-node quadrature per (draw, replicate, guide), no term of
        ``q(pi)``; ``mu`` and ``y`` are the same bits; ``pairs`` then holds the pairs' constants plus the logs of their
        integrals; and ``n_unresolved`` (T, int32) counts, per target, the pairs at which the rule is not valid (the
        weights of such a target are not to be used).  For the ``Normal`` family, which has no ``pi``, ``logw`` is that of
        the plain call bit for bit.

        ``tail_rule=True`` with ``integrate_pi`` (``bean_hip_log_weights_marginal_tail``): the pairs ``n_unresolved``
        counts get the 64-node Gauss-Jacobi rule of ``marginal_grid(tail_rule=True)`` per draw, and ``tail_err``
        (n_draws, T) is added: per draw and target the sum over those pairs of the difference to the 48-node rule.
        Accessibility is admitted.  Same chunking - a chunk's share of the tail workspace, 8 bytes per (draw, tail
        pair), is at most its pair plane - and the same bits per draw; ``mu``, ``y``, ``n_unresolved``, the slots of
        every other pair and ``logw`` of the targets without such pairs are those of ``tail_rule=False`` bit for bit.
        Each library call then synchronises the engine's stream once (the number of such pairs)."""
        if tail_rule and integrate_pi is None:
            raise ValueError("log_weights: tail_rule sets the rule integrate_pi uses for the pairs it does not resolve "
                             "and needs integrate_pi")
        if tail_rule and getattr(self.lib, "bean_hip_log_weights_marginal_tail", None) is None:
            raise PredictiveUnsupported("this library build has no bean_hip_log_weights_marginal_tail")
        if integrate_pi is not None:
            if getattr(self.lib, "bean_hip_log_weights_marginal", None) is None:
                raise PredictiveUnsupported("this library build has no bean_hip_log_weights_marginal")
            if int(integrate_pi) not in _lib.MARGINAL_NODES:
                raise ValueError(f"log_weights: integrate_pi must be one of {_lib.MARGINAL_NODES} quadrature nodes, got "
                                 f"{integrate_pi!r}")
        self._require_predictive("the importance weights do not take",
                                 have=getattr(self.lib, "bean_hip_log_weights", None) is not None)
        S = int(n_draws)
        if S < 1:
            raise ValueError(f"log_weights: n_draws must be at least 1, got {S}")
        R, G, T = self.data.n_reps, self.data.n_guides, int(self.T)
        dev = self.device
        chunk = max(1, min(S, _lib.MAX_LOGW_DRAWS, self.LOGW_PAIR_BYTES // (8 * R * G)))
        logw = torch.empty((S, T), dtype=torch.float64, device=dev)
        mu = torch.empty((S, T), dtype=torch.float64, device=dev)
        y = torch.empty((S, T), dtype=torch.float64, device=dev)
        plane = torch.empty((S if pairs else chunk, R, G), dtype=torch.float64, device=dev)
        # (a draw-independent count: every chunk writes the same values)
        unresolved = None if integrate_pi is None else torch.empty(T, dtype=torch.int32, device=dev)
        tail_err = torch.empty((S, T), dtype=torch.float64, device=dev) if tail_rule else None
        with self._on_stream():
            for j0 in range(0, S, chunk):
                n = min(chunk, S - j0)
                pl = plane[j0:j0 + n] if pairs else plane[:n]
                lw, m, yy = logw[j0:j0 + n], mu[j0:j0 + n], y[j0:j0 + n]
                outs = (_ptr(lw), _nbytes(lw), _ptr(m), _nbytes(m), _ptr(yy), _nbytes(yy), _ptr(pl), _nbytes(pl))
                if integrate_pi is None:
                    self._check(self.lib.bean_hip_log_weights(self._h, int(seed), int(first_draw) + j0, n, *outs,
                                                              self._sptr()), "log_weights")
                elif not tail_rule:
                    self._check(self.lib.bean_hip_log_weights_marginal(
                        self._h, int(seed), int(first_draw) + j0, n, int(integrate_pi), *outs, _ptr(unresolved),
                        _nbytes(unresolved), self._sptr()), "log_weights_marginal")
                else:
                    te = tail_err[j0:j0 + n]
                    self._check(self.lib.bean_hip_log_weights_marginal_tail(
                        self._h, int(seed), int(first_draw) + j0, n, int(integrate_pi), *outs, _ptr(unresolved),
                        _nbytes(unresolved), _ptr(te), _nbytes(te), self._sptr()), "log_weights_marginal_tail")
        self.invalidate_resume()
        out = {"logw": logw, "mu": mu, "y": y}
        if unresolved is not None:
            out["n_unresolved"] = unresolved
        if tail_rule:
            out["tail_err"] = tail_err
        if pairs:
            out["pairs"] = self._to_screen_order(plane, 2)
        return out

    def marginal_grid(self, centre_mu, centre_y, step_mu, step_y, n_mu: int, n_y: int, nodes: int = 32,
                      pairs: bool = False, tail_rule: bool = False) -> Dict[str, torch.Tensor]:
        """The log joint of every target on its own ``n_mu x n_y`` grid of given ``(mu_t, y_t = log sd_t)``, ``pi``
        integrated out of the model by ``nodes``-point quadrature (``bean_hip_marginal_grid``): node (i, k) of target t
        is ``mu = centre_mu[t] + (i - (n_mu - 1) / 2) step_mu[t]``, ``y = centre_y[t] + (k - (n_y - 1) / 2) step_y[t]``
        (four tensors of T values, float64).  Returns ``lj`` (n_mu, n_y, T), a float64 device tensor - the log joint as
        a density in ``(mu, y)``: no draw, no seed, no term of the guide - ``n_unresolved`` (T, int32: the pairs of the
        target at which the rule is not valid; its values are not to be used) and, with ``pairs``, the pair planes
        ``pairs`` (n_mu, n_y, R, G), guides in screen order.

        Nodes go to the library in chunks whose pair plane stays at or below ``LOGW_PAIR_BYTES``: the whole grid, or
        one line of ``mu`` per call, or one node per call.  A line or node is sent as a grid of one with its coordinate
        as the centre, which the library's formula returns as it is, so a node's value is the same bits whatever the
        chunking.  Nothing of the fit is written; ``run(resume=True)`` continues its window.

        ``tail_rule=True`` (``bean_hip_marginal_grid_tail``): the pairs ``n_unresolved`` counts get a Gauss-Jacobi rule
        of 64 nodes in place of the ``nodes``-point rule, and ``tail_err`` (n_mu, n_y, T) is added: per node and target
        the sum over those pairs of the difference to the 48-node rule.  Same chunking, same bits per node; the slots
        of every other pair, and with no such pair ``lj`` itself, are those of ``tail_rule=False`` bit for bit.  Each
        library call then synchronises the engine's stream once (the number of such pairs)."""
        if getattr(self.lib, "bean_hip_marginal_grid", None) is None:
            raise PredictiveUnsupported("this library build has no bean_hip_marginal_grid")
        if tail_rule and getattr(self.lib, "bean_hip_marginal_grid_tail", None) is None:
            raise PredictiveUnsupported("this library build has no bean_hip_marginal_grid_tail")
        self._require_predictive("the grid posterior does not take", grid=True)
        if int(nodes) not in _lib.MARGINAL_NODES:
            raise ValueError(f"marginal_grid: nodes must be one of {_lib.MARGINAL_NODES} quadrature nodes, got {nodes!r}")
        n_mu, n_y = int(n_mu), int(n_y)
        if n_mu < 1 or n_y < 1 or n_mu * n_y > _lib.MAX_LOGW_DRAWS:
            raise ValueError(f"marginal_grid: n_mu >= 1, n_y >= 1 and n_mu * n_y <= {_lib.MAX_LOGW_DRAWS}, got "
                             f"{n_mu} x {n_y}")
        R, G, T = self.data.n_reps, self.data.n_guides, int(self.T)
        dev = self.device
        # Every tensor a library call reads or writes is formed HERE, on the caller's current stream: _on_stream() makes
        # the engine's stream wait for what is queued on the current stream when the scope is entered, and nothing else
        # orders torch's work before the library's launches.
        arrs = []
        for name, v in (("centre_mu", centre_mu), ("centre_y", centre_y), ("step_mu", step_mu), ("step_y", step_y)):
            v = torch.as_tensor(v, dtype=torch.float64).to(dev).reshape(-1).contiguous()
            if v.numel() != T:
                raise ValueError(f"marginal_grid: {name} must hold one value per target ({T}), got {v.numel()}")
            arrs.append(v)
        c_mu, c_y, s_mu, s_y = arrs
        N = n_mu * n_y
        per_node = 8 * R * G
        whole = N * per_node <= self.LOGW_PAIR_BYTES
        by_line = not whole and n_y * per_node <= self.LOGW_PAIR_BYTES
        lj = torch.empty((n_mu, n_y, T), dtype=torch.float64, device=dev)
        n_chunk = N if whole else (n_y if by_line else 1)
        plane = torch.empty((n_mu, n_y, R, G) if pairs else (n_chunk, R, G), dtype=torch.float64, device=dev)
        unresolved = torch.empty(T, dtype=torch.int32, device=dev)
        tail_err = torch.empty((n_mu, n_y, T), dtype=torch.float64, device=dev) if tail_rule else None
        # the library's coordinates of a line or node, two roundings each (a product, a sum)
        mus = [] if whole else [c_mu + s_mu * (i - (n_mu - 1) / 2.0) for i in range(n_mu)]
        ys = [] if whole or by_line else [c_y + s_y * (k - (n_y - 1) / 2.0) for k in range(n_y)]

        def call(cm, cy, nm, ny, out, pl, te=None):
            args = (self._h, int(nodes), nm, ny, _ptr(cm), _ptr(cy), _ptr(s_mu), _ptr(s_y), _ptr(out), _nbytes(out),
                    _ptr(pl), _nbytes(pl), _ptr(unresolved), _nbytes(unresolved))
            if te is None:
                self._check(self.lib.bean_hip_marginal_grid(*args, self._sptr()), "marginal_grid")
            else:
                self._check(self.lib.bean_hip_marginal_grid_tail(*args, _ptr(te), _nbytes(te), self._sptr()),
                            "marginal_grid_tail")

        with self._on_stream():
            if whole:
                call(c_mu, c_y, n_mu, n_y, lj, plane, tail_err)
            else:
                for i in range(n_mu):
                    if by_line:
                        call(mus[i], c_y, 1, n_y, lj[i], plane[i] if pairs else plane, tail_err[i] if tail_rule else None)
                    else:
                        for k in range(n_y):
                            call(mus[i], ys[k], 1, 1, lj[i, k:k + 1], plane[i, k:k + 1] if pairs else plane,
                                 tail_err[i, k:k + 1] if tail_rule else None)
        out = {"lj": lj, "n_unresolved": unresolved}
        if tail_rule:
            out["tail_err"] = tail_err
        if pairs:
            out["pairs"] = self._to_screen_order(plane, 3)
        return out

    def marginal_tail_nodes(self) -> Dict[str, torch.Tensor]:
        """The pairs ``marginal_grid(tail_rule=True)`` gives the Gauss-Jacobi rule, at the current parameters
        (``bean_hip_marginal_tail_nodes``), as device tensors: ``replicate`` and ``guide`` (n,) int64 - the guide in screen
        order; the list is ordered by target, guide, replicate in the engine's guide order - ``side`` (n,) int32, 1 where
        the smaller exponent of the pair's Beta-shaped factor is ``pi_1``'s, and ``z``, ``lw`` (n, 112) float64: the 64
        nodes, ascending, and log weights (normalised to sum 1) of the rule, then those of the 48-node rule.  Nothing of
        the fit is written."""
        if getattr(self.lib, "bean_hip_marginal_tail_nodes", None) is None:
            raise PredictiveUnsupported("this library build has no bean_hip_marginal_tail_nodes")
        self._require_predictive("the grid posterior does not take", grid=True)
        dev, G = self.device, self.data.n_guides
        count = ctypes.c_int32(0)
        with self._on_stream():
            self._check(self.lib.bean_hip_marginal_tail_nodes(self._h, 0, None, None, None, None, ctypes.byref(count),
                                                              self._sptr()), "marginal_tail_nodes")
        n = int(count.value)
        # (formed on the caller's stream, before the engine's stream is made to wait for it: marginal_grid)
        pair = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        side = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        z = torch.zeros((max(n, 1), _lib.TAIL_NODES), dtype=torch.float64, device=dev)
        lw = torch.zeros((max(n, 1), _lib.TAIL_NODES), dtype=torch.float64, device=dev)
        if n:
            with self._on_stream():
                self._check(self.lib.bean_hip_marginal_tail_nodes(self._h, n, _ptr(pair), _ptr(z), _ptr(lw), _ptr(side),
                                                                  ctypes.byref(count), self._sptr()), "marginal_tail_nodes")
        pair = pair[:n].long()
        g = pair % G
        if self.guide_order is not None:
            g = self.guide_order[g]
        return {"replicate": pair // G, "guide": g, "side": side[:n], "z": z[:n], "lw": lw[:n]}

    def run_ensemble(self, n_steps: int, seeds, graph_chunk: int = 50, first_step: Optional[int] = None):
        """Enqueue ``n_steps`` SVI steps of all ``n_members`` fits, member k with ``seeds[k]`` (no host
        synchronisation).  Member k is, bit for bit, a single engine's ``run(n_steps, seed=seeds[k])``;
        stepping in windows gives the bits of one call."""
        seeds = [int(s) for s in seeds]
        first = self.steps_done if first_step is None else int(first_step)
        if first + n_steps > self.loss_hist.shape[-1]:
            raise ValueError("loss history too small: raise num_steps / loss_capacity")
        arr = (ctypes.c_uint64 * max(len(seeds), 1))(*seeds)
        with self._on_stream():
            self._check(self.lib.bean_hip_svi_run_ensemble(self._h, arr, len(seeds), first, int(n_steps), int(graph_chunk),
                                                           self._sptr()), "svi_run_ensemble")
        self._resume_broken = True  # (a following run(resume=True) does not continue this call)
        self.steps_done = first + n_steps

    def run_particles(self, n_steps: int, seed: int = 101, graph_chunk: int = 50, first_step: Optional[int] = None):
        """Enqueue ``n_steps`` SVI steps that each draw every latent site ``n_particles`` times - particle p with
        ``particle_seeds(seed, n_particles)[p]`` - and apply ONE ClippedAdam update with the mean of the gradients (no
        host synchronisation).  The step is defined in ``include/bean_hip.h``; one particle is ``run(n_steps, seed)``
        bit for bit, stepping in windows gives the bits of one call, and ``loss_hist`` holds the particles' mean loss.

        Where the batched kernels take the shape (``ensemble_supported``) the particles share the launches
        (``bean_hip_svi_run_particles``); everywhere else - tiling, survival, ControlNormal, sample covariates, screens
        large enough for the one-launch stepper - the same step is driven from here: ``bean_hip_elbo_grad`` per
        particle, the float64 mean on the gradient tensors, ``bean_hip_adam``."""
        from .model.jackknife import particle_seeds

        if self.n_members != 1:
            raise ValueError("particles inside member sets are not batched: run_particles needs n_members == 1")
        seeds = particle_seeds(seed, self.n_particles)
        first = self.steps_done if first_step is None else int(first_step)
        if first + n_steps > self.loss_hist.numel():
            raise ValueError("loss history too small: raise num_steps / loss_capacity")
        if self._particles_native:
            arr = (ctypes.c_uint64 * len(seeds))(*seeds)
            with self._on_stream():
                self._check(self.lib.bean_hip_svi_run_particles(self._h, arr, len(seeds), first, int(n_steps),
                                                                int(graph_chunk), self._sptr()), "svi_run_particles")
        elif self.n_particles == 1:  # the single fit itself
            self.run(n_steps, seed=seed, graph_chunk=graph_chunk, first_step=first)
        else:
            self._run_particles_loop(seeds, first, int(n_steps))
        self._resume_broken = True  # (a following run(resume=True) does not continue this call)
        self.steps_done = first + n_steps

    def _run_particles_loop(self, seeds, first: int, n_steps: int):
        """The defining loop of a particle step on the engine's stream, nothing read back."""
        lib, h, sp = self.lib, self._h, self._sptr()
        spare = self._loss_all.numel() - 1
        names = list(self.grads)
        P = len(seeds)
        with self._on_stream(), torch.cuda.stream(self.stream):
            per_particle = [[torch.empty_like(self.grads[k]) for k in names] for _ in seeds]
            losses = torch.empty(P, dtype=torch.float64, device=self.device)
            for s in range(first, first + n_steps):
                for p, sd in enumerate(seeds):
                    self._check(lib.bean_hip_elbo_grad(h, int(sd), s, spare, sp), "elbo_grad")
                    for dst, k in zip(per_particle[p], names):
                        dst.copy_(self.grads[k])
                    losses[p] = self._loss_all[spare]
                for i, k in enumerate(names):
                    self.grads[k].copy_(particle_mean([per_particle[p][i] for p in range(P)]))
                self._check(lib.bean_hip_adam(h, s + 1, sp), "adam")
                self._loss_all[s] = particle_mean(list(losses.unbind(0)))

    def _tensor_versions(self):
        return tuple(t._version for d in (self.unconstrained, self._m, self._v) for t in d.values())

    def invalidate_resume(self):
        """Break the chain of resumed windows after writing parameters or moments through raw pointers (writes
        through torch are seen by themselves): the next ``run(resume=True)`` is a plain ``bean_hip_svi_run``."""
        self._resume_broken = True

    def losses(self):
        """The loss history: a list of ``steps_done`` floats; of an ensemble a ``(n_members, steps_done)`` array."""
        torch.cuda.synchronize(self.device)
        if self.n_members != 1:
            return self.loss_hist[:, : self.steps_done].cpu().numpy()
        return self.loss_hist[: self.steps_done].cpu().tolist()

    def set_profile(self, enable):
        """0 off; 1 time the dominant (guide) kernel; 2 time the fused k_param launches instead."""
        self._check(self.lib.bean_hip_set_profile(self._h, int(enable)), "set_profile")

    def get_profile(self):
        avg, n = ctypes.c_double(0.0), ctypes.c_uint64(0)
        self._check(self.lib.bean_hip_get_profile(self._h, ctypes.byref(avg), ctypes.byref(n)), "get_profile")
        return avg.value, n.value

    @property
    def step_bytes(self) -> int:
        return int(self.lib.bean_hip_step_bytes(self._h))

    @property
    def dominant_kernel(self) -> str:
        return self.lib.bean_hip_dominant_kernel(self._h).decode()

    @property
    def dominant_kernel_variant(self) -> str:
        """The template instantiation launched for this shape, as spelt in the code object."""
        return self.lib.bean_hip_dominant_kernel_variant(self._h).decode()

    @property
    def dominant_lds_bytes(self) -> int:
        """Dynamic LDS per workgroup the library requests for the dominant kernel at this shape."""
        return int(self.lib.bean_hip_dominant_lds_bytes(self._h))

    def snapshot(self) -> Dict[str, torch.Tensor]:
        """Device-side copy of the unconstrained parameters as they are when everything enqueued so far has
        run (``run_inference`` keeps the one taken at the start of a report window: if the window's loss
        turns non-finite, that is what ``tmp_result.pkl`` holds, not the NaN updates applied since)."""
        with self._on_stream():
            return {k: v.clone() for k, v in self.unconstrained.items()}

    def constrained(self, snapshot: Optional[Dict[str, torch.Tensor]] = None,
                    member: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Constrained parameter values, as ``pyro.get_param_store()[name]`` (of ``snapshot`` if given); of an
        ensemble, those of ``member``."""
        torch.cuda.synchronize(self.device)
        src = self.unconstrained if snapshot is None else snapshot
        if self.n_members != 1:
            if member is None or not 0 <= int(member) < self.n_members:
                raise ValueError(f"an ensemble of {self.n_members}: constrained(member=k), 0 <= k < {self.n_members}")
            src = {k: v[int(member)] for k, v in src.items()}
        elif member not in (None, 0):
            raise ValueError("a single fit has member 0 only")
        out = {k: (v.exp() if k in POSITIVE else v.clone()) for k, v in src.items()}
        if self.survival and self.family == "MultiMixtureNormal":
            # the reference's tiling survival guide registers this parameter and never uses it
            # (survival_model.py:770-774): it keeps its initial value
            g_all = int(self._shape.n_guides_total) or self.data.n_guides
            out["initial_abundance"] = torch.full((self.data.n_guides,), 1.0 / g_all, dtype=torch.float32,
                                                  device=self.device)
        if self.guide_order is not None:
            # engine guide i is the screen's guide guide_order[i]: per-guide values go back in screen order
            for k in PER_GUIDE:
                if k in out:
                    out[k] = self._to_screen_order(out[k], 0)
        return out


def test_special(op: int, a, x=None, b=None, device="cuda:0"):
    """Evaluate the device special functions (``bean_hip_test_special``)."""
    lib = _lib.load()
    dev = torch.device(device)
    a = torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()
    x = torch.zeros_like(a) if x is None else torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
    b = torch.zeros_like(a) if b is None else torch.as_tensor(b, dtype=torch.float64, device=dev).contiguous()
    o0, o1 = torch.zeros_like(a), torch.zeros_like(a)
    s = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(
        lib.bean_hip_test_special(
            int(op), a.numel(), ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(x.data_ptr()),
            ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(o0.data_ptr()), ctypes.c_void_p(o1.data_ptr()),
            ctypes.c_void_p(s),
        ),
        "test_special",
    )
    torch.cuda.synchronize(dev)
    return o0, o1
