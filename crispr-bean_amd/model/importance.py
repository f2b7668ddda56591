"""Importance-sampling check of the mean-field posterior, per target.

``HipSVI.log_weights`` (``csrc/bean_importance.hpp``) gives, for S draws z_s ~ q of the fitted guide, the per-target
``logw[s, t] = log p(x_t, z_st) - log q(z_st)``: in the sorting variant families the targets share no parameter, so the
importance weights factorise and every target is its own importance-sampling problem.  This module reads them - pure
torch float64, vectorised over targets, on whatever device the weights live.

* ``psis``: Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry 2024).  The ``M = min(floor(0.2 S),
  ceil(3 sqrt(S)))`` largest weights of a target, less the (M + 1)-th largest, are fitted with a generalised Pareto
  distribution by the Zhang-Stephens (2009) profile estimate; its shape, shrunk as ``(k M + 5) / (M + 10)``, is the
  diagnostic ``k``; the M tail weights are replaced by the fitted distribution's quantiles at ``(i - 0.5) / M`` and
  truncated at the raw maximum.
* ``importance_summary``: ``psis_k``, the self-normalised smoothed weights' effective sample size and the
  importance-corrected posterior mean and sd of ``mu``.
* ``marginal_summary``: the same of the weights of ``(mu_t, sd_t)`` alone - ``HipSVI.log_weights(integrate_pi=Q)``, ``pi``
  integrated out of the model by quadrature (``csrc/bean_importance_marg.hpp``) - keys suffixed ``_marg``, NaN for a target
  with a pair the rule does not resolve; with ``tail_err`` (``log_weights(..., tail_rule=True)``: a Gauss-Jacobi rule at
  those pairs, ``csrc/bean_importance_tail.hpp``) such a target is reported where the rule's own check passes.

What ``k`` says (Yao et al. 2018): below 0.5 the guide is a good proposal for this target and the corrected moments can
be trusted; up to 0.7 they are usable; above it the guide is too light-tailed or misplaced for importance sampling to
repair at this S - a finding about the guide (a mean-field Gaussian on ``mu`` next to a 2 R n_guides-dimensional block of
``pi`` draws is a hard proposal), not a fault of the fit or of the check.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

MIN_DRAWS = 25
PRIOR_BS, PRIOR_K = 3.0, 10.0  # Zhang-Stephens' prior on theta; the weakly informative prior on k counts as 10 draws


def tail_size(n_draws: int) -> int:
    return min(int(math.floor(0.2 * n_draws)), int(math.ceil(3.0 * math.sqrt(n_draws))))


def gpd_fit(x: torch.Tensor, shrink: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Zhang-Stephens estimate of the generalised Pareto shape ``k`` and scale ``sigma`` of exceedances ``x`` (M, T),
    ascending along the first axis, location 0; one fit per column.  ``shrink``: the weakly informative
    ``k <- (k M + 5) / (M + 10)``."""
    x = x.double()
    M = x.shape[0]
    m = 30 + int(math.sqrt(M))
    cols = max(1, (1 << 24) // (m * M))  # the (m, M, columns) grid of the profile likelihood stays at 128 MiB
    if x.dim() == 2 and x.shape[1] > cols:
        parts = [gpd_fit(x[:, c0:c0 + cols], shrink) for c0 in range(0, x.shape[1], cols)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    j = torch.arange(1, m + 1, dtype=torch.float64, device=x.device).reshape(m, 1)
    q1 = x[int(M / 4.0 + 0.5) - 1].clamp_min(torch.finfo(torch.float64).tiny)        # (T)
    xmax = x[-1].clamp_min(torch.finfo(torch.float64).tiny)
    theta = 1.0 / xmax + (1.0 - torch.sqrt(m / (j - 0.5))) / (PRIOR_BS * q1)             # (m, T)
    # profile log-likelihood of theta = -k / sigma: k(theta) = mean log1p(-theta x), l = M (log(-theta / k) - k - 1);
    # the estimate is the posterior mean of theta over the grid
    kk = torch.log1p(-theta.unsqueeze(1) * x.unsqueeze(0)).mean(1)                       # (m, T)
    ll = M * (torch.log(-theta / kk) - kk - 1.0)
    w = torch.softmax(ll, 0)
    th = (w * theta).sum(0)
    k = torch.log1p(-th * x).mean(0)
    sigma = -k / th
    if shrink:
        k = (k * M + PRIOR_K * 0.5) / (M + PRIOR_K)
    return k, sigma


def gpd_quantile(p: torch.Tensor, k: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    """Quantile function of GPD(k, sigma), location 0: ``sigma expm1(-k log1p(-p)) / k`` (``-sigma log1p(-p)`` at k = 0)."""
    l = -torch.log1p(-p)
    small = k.abs() < 1e-12
    ks = torch.where(small, torch.ones_like(k), k)
    return torch.where(small, sigma * l, sigma * torch.expm1(ks * l) / ks)


def psis(logw: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Pareto-smoothed log weights and the tail index: ``logw`` (S, T) -> (``logw_smoothed`` (S, T), ``k`` (T)).
    The smoothed weights are on the scale of ``logw`` less its per-target maximum (not normalised).  A target whose
    weights are all equal, or whose tail is degenerate, keeps its weights and reports ``k = -inf`` / ``inf``
    respectively, as the reference implementations do."""
    logw = torch.as_tensor(logw)
    if logw.dim() != 2:
        raise ValueError(f"psis: logw must be (S, T), got shape {tuple(logw.shape)}")
    S, T = logw.shape
    if S < MIN_DRAWS:
        raise ValueError(f"psis: at least {MIN_DRAWS} draws are needed to fit a tail, got {S}")
    lw = logw.double()
    lw = lw - lw.max(0, keepdim=True).values
    M = tail_size(S)
    srt, order = torch.sort(lw, 0)
    tail, tail_idx = srt[S - M:], order[S - M:]          # ascending
    cut = srt[S - M - 1]                                  # the largest weight outside the tail
    ecut = cut.exp()
    x = tail.exp() - ecut                                 # exceedances, ascending, (M, T)
    k, sigma = gpd_fit(x)
    p = ((torch.arange(1, M + 1, dtype=torch.float64, device=lw.device) - 0.5) / M).reshape(M, 1)
    smoothed = torch.log(gpd_quantile(p, k.unsqueeze(0), sigma.unsqueeze(0)) + ecut).clamp(max=0.0)
    flat = tail[-1] - tail[0] <= 0.0                       # equal tail weights: nothing to fit
    bad = ~torch.isfinite(k) | ~torch.isfinite(smoothed).all(0)
    keep = flat | bad
    smoothed = torch.where(keep.unsqueeze(0), tail, smoothed)
    k = torch.where(flat, torch.full_like(k, -math.inf), torch.where(bad, torch.full_like(k, math.inf), k))
    out = lw.scatter(0, tail_idx, smoothed)
    return out, k


def importance_summary(logw: torch.Tensor, mu: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Per target, from ``logw`` and the drawn ``mu`` (both (S, T)): ``psis_k``; with w~ the self-normalised smoothed
    weights ``is_ess = 1 / sum w~^2``, ``mu_is = sum w~ mu``, ``mu_sd_is = sqrt(sum w~ (mu - mu_is)^2)``; ``n_is = S``."""
    logw = torch.as_tensor(logw)
    mu = torch.as_tensor(mu).double().to(logw.device)
    if mu.shape != logw.shape:
        raise ValueError(f"importance_summary: logw {tuple(logw.shape)} and mu {tuple(mu.shape)} differ in shape")
    ls, k = psis(logw)
    w = torch.softmax(ls, 0)
    mu_is = (w * mu).sum(0)
    var = (w * (mu - mu_is) ** 2).sum(0)
    return {
        "psis_k": k,
        "is_ess": 1.0 / (w * w).sum(0),
        "mu_is": mu_is,
        "mu_sd_is": var.clamp_min(0.0).sqrt(),
        "n_is": torch.full_like(k, float(logw.shape[0])),
    }


MARGINAL_KEYS = ("psis_k_marg", "mu_is_marg", "mu_sd_is_marg", "is_ess_marg", "n_pairs_unresolved")


TAIL_KEYS = ("n_pairs_tail", "is_tail_err")  # the columns --importance-tail-rule adds behind MARGINAL_KEYS
TAIL_BOUND = 1e-3       # nat per tail pair: the bound section 21 sets for a pair's log integral
TAIL_WEIGHT_MIN = 1e-6  # a draw counts for is_tail_err where its raw weight is at least this share of the largest


def marginal_summary(logw_marg: torch.Tensor, mu: torch.Tensor, n_unresolved: torch.Tensor, *,
                     tail_err=None) -> Dict[str, torch.Tensor]:
    """``importance_summary`` of the weights with ``pi`` integrated out (``HipSVI.log_weights(integrate_pi=Q)``), keys
    suffixed ``_marg``, plus ``n_pairs_unresolved``: the (replicate, guide) pairs of the target at which the quadrature
    rule is not valid.  A target with such a pair has NaN in the four marginal values - its weights are not reported.

    ``tail_err`` (S, T) - ``HipSVI.log_weights(integrate_pi=Q, tail_rule=True)``, whose weights carry the Gauss-Jacobi
    rule at those pairs - adds ``n_pairs_tail``, the count of the pairs that took the rule (``n_unresolved``), and
    ``is_tail_err``: the largest ``tail_err[d, t]`` over the draws whose raw ``logw[d, t]`` is within ``log 1e6`` of the
    target's largest (a draw below that does not enter the sums at that precision either).  A target with such pairs then
    gets its four values where ``is_tail_err <= 1e-3 n_pairs_tail`` and NaN otherwise; both diagnostics are kept."""
    s = importance_summary(logw_marg, mu)
    n = torch.as_tensor(n_unresolved).to(s["psis_k"].device)
    if n.shape != s["psis_k"].shape:
        raise ValueError(f"marginal_summary: n_unresolved {tuple(n.shape)} is not one count per target "
                         f"{tuple(s['psis_k'].shape)}")
    nan = torch.full_like(s["psis_k"], math.nan)
    left_out = n > 0
    extra = {}
    if tail_err is not None:
        lw = torch.as_tensor(logw_marg).double()
        te = torch.as_tensor(tail_err).double().to(lw.device)
        if te.shape != lw.shape:
            raise ValueError(f"marginal_summary: tail_err has shape {tuple(te.shape)}, logw {tuple(lw.shape)}")
        counts = (lw - lw.max(0).values) >= math.log(TAIL_WEIGHT_MIN)
        worst = torch.where(counts, te, torch.zeros_like(te)).max(0).values
        # (not (worst <= bar): a NaN error refuses)
        left_out = left_out & ~(worst <= TAIL_BOUND * n.to(worst.dtype))
        extra = {"n_pairs_tail": n.to(s["psis_k"].dtype), "is_tail_err": worst}
    out = {f"{k}_marg": torch.where(left_out, nan, s[k]) for k in ("psis_k", "mu_is", "mu_sd_is", "is_ess")}
    out["n_pairs_unresolved"] = n.to(s["psis_k"].dtype)
    out.update(extra)
    return out


def importance_check(engine, n_draws: int = 1000, seed: int = 101, integrate_pi=None,
                     tail_rule: bool = False) -> Dict[str, torch.Tensor]:
    """``importance_summary`` of ``n_draws`` draws (0 .. n_draws - 1) from the guide of ``engine`` at its current
    parameters; device tensors of length T.  ``integrate_pi=Q`` (16, 32 or 64 quadrature nodes): merged with the
    ``marginal_summary`` of the same draws' weights of ``(mu_t, sd_t)`` alone; with ``tail_rule`` those weights take the
    Gauss-Jacobi rule at the pairs the quadrature does not resolve, and the summary its ``tail_err``."""
    if tail_rule and integrate_pi is None:
        raise ValueError("importance_check: tail_rule needs integrate_pi")
    out = engine.log_weights(0, int(n_draws), seed=seed)
    summary = importance_summary(out["logw"], out["mu"])
    if integrate_pi is not None:
        kw = {"tail_rule": True} if tail_rule else {}
        marg = engine.log_weights(0, int(n_draws), seed=seed, integrate_pi=int(integrate_pi), **kw)
        summary.update(marginal_summary(marg["logw"], marg["mu"], marg["n_unresolved"],
                                        **({"tail_err": marg["tail_err"]} if tail_rule else {})))
    return summary
