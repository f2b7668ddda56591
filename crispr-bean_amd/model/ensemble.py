"""Combining the members of a seed ensemble (``run_inference_ensemble``) into one set of result-table parameters.

Every member is an SVI fit of the same screen with another random stream; each leaves a Gaussian posterior
``Normal(mu_loc, mu_scale)`` per target (and ``LogNormal(sd_loc, sd_scale)`` for its spread, Gaussian in log
space).  The combination is the moment match of the equal-weight mixture of the members' posteriors: its mean is
the mean of the locations, its variance the mean of the variances plus the (population) variance of the locations.
Pure torch: no GPU involved.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from .run import ParamStore

# (location, scale) pairs of the Gaussian sites; sd_* are location and scale of log(sd)
GAUSSIAN_SITES = (("mu_loc", "mu_scale"), ("sd_loc", "sd_scale"))


def _params_of(member):
    """A member as ``run_inference`` returns it - ``(ParamStore, {"loss", "params"})`` - or its store / dict alone."""
    if isinstance(member, (tuple, list)):
        member = member[0]
    return member


def combine_ensemble(results: Sequence) -> Tuple[ParamStore, Dict[str, object]]:
    """``(store, spread)`` from K members.

    ``store``: ``mu_loc = mean_k mu_loc_k``; ``mu_scale = sqrt(mean_k mu_scale_k^2 + var_k(mu_loc_k))`` with the
    population variance; ``sd_loc`` / ``sd_scale`` likewise; every other parameter (``alpha_pi``, ``noise_loc``,
    ``noise_scale``, ...) the arithmetic mean over the members.  K = 1 gives the member back exactly; K > 1 is
    evaluated and returned in float64.
    ``spread``: ``{"mu_seed_sd": std_k(mu_loc_k) (population, shape of mu_loc), "n_seeds": K}``.
    """
    stores = [_params_of(m) for m in results]
    if not stores:
        raise ValueError("combine_ensemble needs at least one member")
    names = list(stores[0].keys())
    for s in stores[1:]:
        if list(s.keys()) != names:
            raise ValueError("the members of an ensemble hold the same parameters")
    k = len(stores)
    if k == 1:
        one = {n: stores[0][n].detach().clone() for n in names}
        sd = torch.zeros_like(one["mu_loc"]) if "mu_loc" in one else None
        return ParamStore(one), {"mu_seed_sd": sd, "n_seeds": 1}
    stack = {n: torch.stack([s[n].detach().cpu().to(torch.float64) for s in stores]) for n in names}
    out = {n: v.mean(0) for n, v in stack.items()}
    for loc, scale in GAUSSIAN_SITES:
        if loc in stack and scale in stack:
            between = stack[loc].var(0, unbiased=False)
            out[scale] = torch.sqrt((stack[scale] ** 2).mean(0) + between)
    sd = stack["mu_loc"].std(0, unbiased=False) if "mu_loc" in stack else None
    return ParamStore(out), {"mu_seed_sd": sd, "n_seeds": k}
