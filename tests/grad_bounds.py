"""A tolerance for every element of every ELBO gradient, derived from the float64 oracle alone.

The kernels' contract is float64 arithmetic on float32-stored parameters, rounded once to a float32 gradient.  The
parity tests hold them to ``max|g - ref| <= 5e-7 max|ref|``, which lets an element 1e-4 of the tensor's largest be
wrong by a third of its value; ClippedAdam divides each element by its own history, so such an element moves its
parameter as far as any other.  ``elementwise_bounds`` returns for every element k

    tol_k = 2^-23 |ref_k| + 1e-12 S_k + c P_k

* ``2^-23 |ref_k|``: one float32 ulp - the kernel's single output rounding (2^-24) and as much again.
* ``S_k``: the magnitude of the terms that ``ref_k`` is the signed sum of.  For each count likelihood (X, X_bcmatch),
  replicate r and bin b, over the (replicate, guide) pairs the likelihood's mask keeps,
  ``(max(1, |psi(a_b + x_b) - psi(a_b)|) + max(1, |psi(A + n) - psi(A)|)) |d alpha[r, g, b] / d theta_k|``, plus
  ``|d lp_s / d theta_k|`` of every other model or guide site s.  ``1e-12`` is what ``test_lgamma_digamma_differences``
  (tests/test_gpu_parity.py) pins on each device digamma difference, relative to max(1, |difference|); here it is carried
  through the Jacobian d alpha / d theta.  The Jacobian is autograd's: one backward per (likelihood, r, b, group of
  guides), the groups chosen so that no two guides of a group share a parameter that is not per guide (the position of a
  guide inside its target; for tiling screens a colouring of the guides by the edits they share), which makes the
  absolute value exact for every element.
* ``P_k`` (only the parameters behind a Dirichlet's concentrations, ``alpha_pi`` and ``q0``): the magnitude of the
  pathwise part, ``sum_r |dirichlet_grad(x, c, sum c) (gpi - sum_a x gpi)| |dc / d theta_k|`` with
  ``gpi = d loss / d pi`` taken by a hook on the draw.  ``c = 1e-8`` is the 0.999 quantile that
  ``test_dirichlet_grad_matches_torch`` pins on the device's implicit gradient against torch's; its maximum, ``1e-6``
  (``C_PATH_TAIL``), is admitted for at most 1 % of a tensor's elements (``MAX_TAIL_SHARE``) - a condition the test
  checks and prints, not a fit.

Nothing here looks at what the code under test returns.
"""
from __future__ import annotations

import contextlib
import copy

import numpy as np
import torch

from oracle import elbo
from oracle import survival as osurv

ULP32 = 2.0 ** -23
C_DIGAMMA = 1e-12
C_PATH = 1e-8
C_PATH_TAIL = 1e-6
MAX_TAIL_SHARE = 0.01
BRANCHES = ("small_alpha", "small_beta", "saddle", "rational")


class _Patched:
    """Wrap a function of oracle.elbo in every oracle module that holds it by name."""

    def __init__(self, name, wrapper_of):
        self.name, self.wrapper_of, self.saved = name, wrapper_of, []

    def __enter__(self):
        for mod in (elbo, osurv):
            if hasattr(mod, self.name):
                orig = getattr(mod, self.name)
                self.saved.append((mod, orig))
                setattr(mod, self.name, self.wrapper_of(orig))
        return self

    def __exit__(self, *exc):
        for mod, orig in self.saved:
            setattr(mod, self.name, orig)


def guide_groups(data):
    """Index arrays that partition the guides so that no two guides of a group share a parameter that is not per guide:
    variant screens, the position of a guide inside its target; tiling screens, a greedy colouring by shared edits."""
    G = data.n_guides
    tl = getattr(data, "target_lengths", None)
    if tl is not None:
        pos = np.concatenate([np.arange(int(n)) for n in tl])
        return [torch.as_tensor(np.nonzero(pos == j)[0]) for j in range(int(pos.max()) + 1)]
    if getattr(data, "a2e_ptr", None) is None:
        return [torch.arange(G)]  # one parameter set shared by all guides is not covered (ControlNormal)
    ptr, idx = data.a2e_ptr.numpy().astype(np.int64), data.a2e_idx.numpy().astype(np.int64)
    A1 = data.n_max_alleles - 1
    edits_of = [set(idx[ptr[g * A1]:ptr[(g + 1) * A1]].tolist()) for g in range(G)]
    used = []  # per colour: the edits its guides hold
    members = []
    for g in range(G):
        for c, e in enumerate(used):
            if not (e & edits_of[g]):
                e |= edits_of[g]
                members[c].append(g)
                break
        else:
            used.append(set(edits_of[g]))
            members.append([g])
    return [torch.as_tensor(m) for m in members]


def elementwise_bounds(loss_fn, data64, params, noise, kw=None, mask_thres=10, dirichlet_grad=None, path_allowance=None):
    """``loss_fn`` is a family's oracle loss, ``data64`` the float64 screen (``elbo.as_float64``), ``params`` the
    unconstrained parameters (float64 values of the float32 storage) and ``noise`` the dumped draws.  Returns
    ``(loss, ref, tol, tol_tail)``: the oracle loss and, per parameter name, float64 arrays shaped like the parameter
    with the oracle gradient, ``tol_k`` and ``tol_k`` with ``C_PATH_TAIL`` in place of ``C_PATH``.

    ``dirichlet_grad(x, concentration, total)`` replaces ``torch._dirichlet_grad`` as the oracle's implicit gradient
    (``elbo.implicit_gradient``).  ``path_allowance(x, concentration, total, dgrad)`` returns, per evaluation, the
    absolute error admitted on the implicit gradient; it then stands where ``C_PATH |dgrad|`` and ``C_PATH_TAIL |dgrad|``
    stand in ``P_k``, and ``tol_tail`` is ``tol``: no element has a tail constant to fall back on.  With both unset every
    number returned is what it was without them."""
    kw = dict(kw or {})
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    leaves = list(p.values())
    counts, draws = [], []

    def spy_counts(orig):
        def f(conc, value):
            counts.append((conc, value))
            return orig(conc, value)
        return f

    def spy_draw(orig):
        def f(concentration, given):
            x = orig(concentration, given)
            rec = {"conc": concentration, "x": x.detach()}
            # d loss / d pi: the first backward through the draw is the loss's (the later ones are the Jacobians')
            def hook(g, rec=rec):
                rec.setdefault("gpi", g.detach().clone())

            x.register_hook(hook)
            draws.append(rec)
            return x
        return f

    rec = {"keep_terms": True}
    hook = elbo.implicit_gradient(dirichlet_grad) if dirichlet_grad is not None else contextlib.nullcontext()
    with _Patched("dirichlet_multinomial_log_prob", spy_counts), _Patched("dirichlet_rsample", spy_draw), hook:
        loss = loss_fn(data64, p, noise=noise, record=rec, **kw)
    grads = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    ref = {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), grads)}

    def add_abs(acc, out):
        gs = torch.autograd.grad(out, leaves, retain_graph=True, allow_unused=True)
        for k, g in zip(p, gs):
            if g is not None:
                acc[k] += g.abs()

    # ---- S_k
    S = {k: torch.zeros_like(v) for k, v in p.items()}
    groups = guide_groups(data64)
    G = data64.n_guides
    sel = torch.zeros(len(groups), G, dtype=torch.float64)
    for j, m in enumerate(groups):
        sel[j, m] = 1.0
    assert len(counts) in (1, 2)
    for conc, val in counts:
        dg = torch.digamma
        d_bin = (dg(conc + val) - dg(conc)).detach().abs().clamp(min=1.0)
        tot, n = conc.sum(-1, keepdim=True), val.sum(-1, keepdim=True)
        d_tot = (dg(tot + n) - dg(tot)).detach().abs().clamp(min=1.0)
        keep = torch.logical_and(val.sum(-1) > mask_thres, data64.repguide_mask).double()[..., None]
        w = (d_bin + d_tot) * keep  # (R, G, B)
        R, _, B = w.shape
        for r in range(R):
            for b in range(B):
                wa = w[r, :, b] * conc[r, :, b]
                for j in range(len(groups)):
                    if float((w[r, :, b] * sel[j]).sum()) == 0.0:
                        continue
                    add_abs(S, (wa * sel[j]).sum())
    lik = ("guide_counts", "guide_bcmatch_counts")
    for side in ("model", "guide"):
        for name, lp in rec["terms"][side].items():
            if name not in lik and lp.requires_grad:
                add_abs(S, lp.double())

    # ---- P_k
    P = {k: torch.zeros_like(v) for k, v in p.items()}
    for d in draws:
        conc, x, gpi = d["conc"], d["x"], d.get("gpi")
        if gpi is None or not conc.requires_grad:
            continue
        total = conc.detach().sum(-1, True).expand_as(conc).contiguous()
        dgrad = (dirichlet_grad or torch._dirichlet_grad)(x.contiguous(), conc.detach().contiguous(), total)
        if path_allowance is not None:
            dgrad = path_allowance(x.contiguous(), conc.detach().contiguous(), total, dgrad)
        D = (dgrad * (gpi - (x * gpi).sum(-1, True))).abs()
        D = torch.where(torch.isfinite(D), D, torch.zeros_like(D))
        if conc.dim() == 2:
            # the Dirichlet over all guides of the survival families: c_g = exp(theta_g), a diagonal Jacobian
            add_abs(P, (D * conc).sum())
        else:
            # c[g, a] depends on theta[g, :] only: one backward per allele, the replicates' terms share their sign
            for a in range(conc.shape[-1]):
                if float(D[..., a].sum()) > 0.0:
                    add_abs(P, (D[..., a] * conc[..., a]).sum())

    out_ref, tol, tol_tail = {}, {}, {}
    for k in p:
        r_ = ref[k].detach().numpy()
        s_, p_ = S[k].detach().numpy(), P[k].detach().numpy()
        out_ref[k] = r_
        c_path, c_tail = (C_PATH, C_PATH_TAIL) if path_allowance is None else (1.0, 1.0)
        tol[k] = ULP32 * np.abs(r_) + C_DIGAMMA * s_ + c_path * p_
        tol_tail[k] = ULP32 * np.abs(r_) + C_DIGAMMA * s_ + c_tail * p_
    return float(loss.detach()), out_ref, tol, tol_tail


def reverse_bins(data):
    """The same screen with its bin axis reversed: the same loss and gradients, summed in another order."""
    out = copy.copy(data)
    B = data.n_condits
    perm = torch.arange(B - 1, -1, -1)
    for k in ("X_masked", "X_bcmatch_masked", "size_factor", "size_factor_bcmatch", "sample_mask"):
        setattr(out, k, getattr(data, k)[:, perm].contiguous())
    for k in ("upper_bounds", "lower_bounds"):
        setattr(out, k, getattr(data, k)[perm].contiguous())
    return out


# ---------------------------------------------------------------- parameter points
def fitted_like_alpha_pi(data, alpha_pi: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """``alpha_pi`` (unconstrained, float32) at editing rates a fit reaches instead of the all-equal start: rates
    log-uniform in [1e-3, 0.5], in a quarter of the guides the OTHER allele the rare one; for tiling screens every
    unmasked allele its own log-uniform weight, masked alleles untouched."""
    rng = np.random.default_rng(seed)
    G, A = alpha_pi.shape
    lo, hi = np.log(1e-3), np.log(0.5)
    out = alpha_pi.detach().cpu().float().clone()
    mask = getattr(data, "allele_mask", None)
    if mask is None:
        assert A == 2
        rate = np.exp(rng.uniform(lo, hi, G))
        flip = rng.random(G) < 0.25
        raw = np.stack([1.0 - rate, rate], -1)
        raw[flip] = raw[flip][:, ::-1].copy()
        return torch.tensor(np.log(raw)).float()
    w = torch.tensor(rng.uniform(lo, hi, (G, A))).float()
    m = mask.cpu()
    out[m] = w[m]
    return out


# ---------------------------------------------------------------- branches of the implicit gradient
def dirichlet_grad_branch(x, alpha, total):
    """Index into ``BRANCHES`` of the formula torch's ``dirichlet_grad_one`` (ATen/native/Distributions.h) and the
    device's ``dirichlet_grad_one_t`` (csrc/bean_special.hpp) take, same operations in the same order."""
    x, alpha, total = (np.asarray(v, dtype=np.float64) for v in (x, alpha, total))
    beta = total - alpha
    boundary = total * x * (1.0 - x)
    small_a = (x <= 0.5) & (boundary < 2.5)
    small_b = (x >= 0.5) & (boundary < 0.75) & ~small_a
    mid = ~small_a & ~small_b & (alpha > 6.0) & (beta > 6.0)
    return np.where(small_a, 0, np.where(small_b, 1, np.where(mid, 2, 3)))


def variational_concentrations(data, alpha_pi, survival: bool):
    """(G, A) float64 concentrations of the guide's Dirichlet(pi) site from the unconstrained ``alpha_pi``, and which of
    them the kernels evaluate the implicit gradient for (not clamped to 1e-5, not a masked allele)."""
    a = alpha_pi.detach().cpu().double().exp()
    mask = getattr(data, "allele_mask", None)
    live = torch.ones_like(a, dtype=torch.bool)
    if mask is not None:
        a = torch.where(mask.cpu(), a, torch.full_like(a, 1e-5))
        live = mask.cpu().clone()
    c = a / a.sum(-1, keepdim=True) * data.pi_a0.cpu().double()[:, None]
    if mask is None or survival:
        live &= c >= 1e-5
        c = c.clamp(1e-5)
    return c, live


def branch_counts(data, alpha_pi, pi, survival: bool = False):
    """How many of the implicit-gradient evaluations of the dumped draw ``pi`` (R, 1, G, A) take each branch."""
    c, live = variational_concentrations(data, alpha_pi, survival)
    x = pi.detach().cpu().double().reshape(-1, *c.shape)
    cc = c[None].expand_as(x)
    tot = c.sum(-1, keepdim=True)[None].expand_as(x)
    br = dirichlet_grad_branch(x.numpy(), cc.numpy(), tot.numpy())
    lv = live[None].expand_as(x).numpy()
    return np.array([int(((br == i) & lv).sum()) for i in range(4)])
