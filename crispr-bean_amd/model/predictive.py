"""Posterior predictive check of a fitted sorting screen.

``HipSVI.simulate`` draws replicate screens on the device (``csrc/bean_predictive.hpp``): the latent sites from the
fitted guide, then the counts from the Dirichlet-Multinomial likelihood at those sites, every (replicate, guide) with
its observed total.  This module compares discrepancy statistics of those replicates with the observed screen.  Pure
torch on the engine's device; the draws are accumulated, never kept.

Definitions, with S draws.  A pair (r, g) is *unmasked* where ``repguide_mask`` holds and its observed total exceeds
``mask_thres``; a cell (r, b, g) additionally needs ``sample_mask[r, b]``.

* cell: predictive ``mean`` and ``sd`` (unbiased) of ``x_rep``, ``z = (x_obs - mean) / sd`` (NaN where sd is 0) and the
  two-sided p-value ``min(1, 2 min((n_ge + 1) / (S + 1), (n_le + 1) / (S + 1)))`` with ``n_ge`` / ``n_le`` the draws with
  ``x_rep >= x_obs`` / ``x_rep <= x_obs``.
* pair: sorting score ``T_rg = sum_b mid_b x_b / n`` with ``mid_b`` the midpoint of bin b's quantile range.
* guide: ``T_g`` = mean of ``T_rg`` over the unmasked replicates, ``ppc_p_score`` its two-sided p-value against the
  replicates' ``T_g``, ``ppc_z_score = (T_g - mean) / sd`` over the draws; ``V_g`` = unbiased variance of ``T_rg`` over
  the unmasked replicates (NaN with fewer than two), ``ppc_p_spread = (n_ge + 1) / (S + 1)``, one-sided: the replicates
  disagree more than the model predicts.  Guides without an unmasked replicate hold NaN.
* sample (r, b): ``frac_cells_p05`` = share of the unmasked guides whose cell p is <= 0.05, ``mean_z`` = mean cell z over
  them (cells without a z left out).
* with barcode-matched counts the same quantities of X_bcmatch carry the suffix ``_bcmatch``.

Survival screens (``survival_predictive``, ``HipSVI.simulate_survival``, ``csrc/bean_survival_predictive.hpp``): the
conditions are the timepoints, and ``mid_b`` is the engine's normalised time ``t_b``.  The pair score is then the
read-weighted mean time ``T_rg = sum_b t_b x_b / n`` - larger for a guide that grows over the screen, smaller for one that
drops out - so ``ppc_z_score > 0`` reads "grows faster than the fitted model says" and ``ppc_p_score`` is the two-sided
p-value of that.  ``V_g`` / ``ppc_p_spread`` compare the replicates' mean times, and the cell and sample quantities are the
same per (replicate, timepoint, guide) and per (replicate, timepoint).  Every definition and column name above holds
unchanged.
"""
from __future__ import annotations

from typing import Dict, Iterable

import torch

NAN = float("nan")


def bin_midpoints(upper_bounds, lower_bounds) -> torch.Tensor:
    """``mid_b``: midpoint of condition b's quantile range (the bounds the engine turns into ``z_lo`` / ``z_hi``)."""
    return (torch.as_tensor(upper_bounds).double() + torch.as_tensor(lower_bounds).double()) * 0.5


def two_sided_p(n_ge: torch.Tensor, n_le: torch.Tensor, n_draws: int) -> torch.Tensor:
    lo = torch.minimum(n_ge.double() + 1.0, n_le.double() + 1.0) / (n_draws + 1.0)
    return torch.clamp(2.0 * lo, max=1.0)


def _moments(s1, s2, n):
    mean = s1 / n
    if n < 2:
        return mean, torch.full_like(mean, NAN)
    var = torch.clamp((s2 - n * mean * mean) / (n - 1.0), min=0.0)
    return mean, var.sqrt()


class _Lik:
    """Accumulators of one likelihood's counts."""

    def __init__(self, x_obs, repguide, sample, mask_thres, mid):
        self.x = x_obs.double()
        self.n = self.x.sum(1)                                    # (R, G)
        self.pair = repguide & (self.n > mask_thres)              # (R, G)
        self.cell = self.pair.unsqueeze(1) & sample.unsqueeze(2)  # (R, B, G)
        self.mid = mid.reshape(1, -1, 1)
        self.T_obs, self.V_obs = self.scores(self.x)
        z = torch.zeros_like
        self.s1, self.s2, self.ge, self.le = z(self.x), z(self.x), z(self.x), z(self.x)
        self.t1, self.t2, self.tge, self.tle, self.vge = (z(self.T_obs) for _ in range(5))

    def scores(self, x):
        """``T_g`` and ``V_g`` of one screen's counts ``x`` (R, B, G), float64."""
        n = x.sum(1)                                              # the screen's own totals (a draw keeps the observed ones)
        t = (x * self.mid).sum(1) / torch.where(n > 0, n, torch.ones_like(n))  # (R, G)
        w = self.pair.double()
        k = w.sum(0)
        tg = torch.where(k > 0, (t * w).sum(0) / k.clamp(min=1.0), torch.full_like(k, NAN))
        dev = (t - tg.unsqueeze(0)) * w
        vg = torch.where(k > 1, (dev * dev).sum(0) / (k - 1.0).clamp(min=1.0), torch.full_like(k, NAN))
        return tg, vg

    def add(self, x_rep):
        x = x_rep.double()
        self.s1 += x
        self.s2 += x * x
        self.ge += x >= self.x
        self.le += x <= self.x
        tg, vg = self.scores(x)
        self.t1 += tg
        self.t2 += tg * tg
        self.tge += tg >= self.T_obs
        self.tle += tg <= self.T_obs
        self.vge += vg >= self.V_obs

    def result(self, S, suffix):
        mean, sd = _moments(self.s1, self.s2, S)
        z = torch.where(sd > 0, (self.x - mean) / torch.where(sd > 0, sd, torch.ones_like(sd)), torch.full_like(sd, NAN))
        p = two_sided_p(self.ge, self.le, S)
        cell = self.cell
        k = cell.double().sum(2)                                  # (R, B)
        none = torch.full_like(k, NAN)
        frac = torch.where(k > 0, ((p <= 0.05) & cell).double().sum(2) / k.clamp(min=1.0), none)
        zok = cell & ~torch.isnan(z)
        kz = zok.double().sum(2)
        mean_z = torch.where(kz > 0, torch.where(zok, z, torch.zeros_like(z)).sum(2) / kz.clamp(min=1.0), none)
        t_mean, t_sd = _moments(self.t1, self.t2, S)
        has = ~torch.isnan(self.T_obs)
        has_v = ~torch.isnan(self.V_obs)
        nan_g = torch.full_like(self.T_obs, NAN)
        out = {
            "cell_mean": mean, "cell_sd": sd, "cell_z": z, "cell_p": p, "cell_unmasked": cell, "pair_unmasked": self.pair,
            "T_obs": self.T_obs, "V_obs": self.V_obs,
            "ppc_p_score": torch.where(has, two_sided_p(self.tge, self.tle, S), nan_g),
            "ppc_p_spread": torch.where(has_v, (self.vge + 1.0) / (S + 1.0), nan_g),
            "ppc_z_score": torch.where(has & (t_sd > 0), (self.T_obs - t_mean) / torch.where(t_sd > 0, t_sd, torch.ones_like(t_sd)),
                                       nan_g),
            "frac_cells_p05": frac, "mean_z": mean_z,
        }
        return {k_ + suffix: v for k_, v in out.items()}


GUIDE_COLUMNS = ("ppc_p_score", "ppc_p_spread", "ppc_z_score")
SAMPLE_COLUMNS = ("frac_cells_p05", "mean_z")


def predictive_summary(observed: Dict[str, torch.Tensor], replicates_iter: Iterable[Dict[str, torch.Tensor]],
                       masks: Dict[str, torch.Tensor], bin_mid: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The summary defined in this module's docstring.

    ``observed``: ``{"X": (R, B, G)}`` and optionally ``"X_bcmatch"``; ``replicates_iter`` yields dicts with the same
    keys, one per draw (consumed one at a time); ``masks``: ``{"repguide": (R, G), "sample": (R, B), "mask_thres": int}``;
    ``bin_mid``: (B,).  Returns a dict of tensors on ``observed``'s device plus ``"n_draws"``."""
    dev = observed["X"].device
    repguide = torch.as_tensor(masks["repguide"]).to(dev) != 0
    sample = torch.as_tensor(masks["sample"]).to(dev) != 0
    thres = float(masks.get("mask_thres", 10))
    mid = torch.as_tensor(bin_mid).to(dev, torch.float64)
    liks = {key: _Lik(observed[key].to(dev), repguide, sample, thres, mid)
            for key in ("X", "X_bcmatch") if observed.get(key) is not None}
    S = 0
    for rep in replicates_iter:
        for key, acc in liks.items():
            acc.add(rep[key].to(dev))
        S += 1
    if S < 1:
        raise ValueError("predictive_summary needs at least one replicate draw")
    out = {"n_draws": S}
    for key, acc in liks.items():
        out.update(acc.result(S, "" if key == "X" else "_bcmatch"))
    return out


def posterior_predictive(engine, n_draws: int = 200, seed: int = 101) -> Dict[str, torch.Tensor]:
    """Drive ``engine.simulate`` for draws 0 ... ``n_draws`` - 1 at the engine's current parameters and return the
    summary.  Raises ``PredictiveUnsupported`` where the count simulator does not take the engine."""
    from ..engine import PredictiveUnsupported

    n_draws = int(n_draws)
    if n_draws < 1:
        raise ValueError(f"n_draws must be >= 1, got {n_draws}")
    if not engine.predictive_supported:
        raise PredictiveUnsupported(f"a posterior predictive check is not available for this engine ({engine.family}"
                                    f"{', survival' if engine.survival else ''})")
    data = engine.data
    observed = {"X": engine._keep["X"]}
    if engine.use_bcmatch:
        observed["X_bcmatch"] = engine._keep["X_BC"]
    masks = {"repguide": data.repguide_mask, "sample": data.sample_mask, "mask_thres": int(engine._shape.mask_thres)}
    mid = bin_midpoints(data.upper_bounds, data.lower_bounds)
    return predictive_summary(observed, (engine.simulate(d, seed=seed) for d in range(n_draws)), masks, mid)


def survival_predictive(engine, n_draws: int = 200, seed: int = 101) -> Dict[str, torch.Tensor]:
    """Drive ``engine.simulate_survival`` for draws 0 ... ``n_draws`` - 1 at the engine's current parameters and return
    ``predictive_summary`` with ``bin_mid`` the engine's normalised timepoints (the survival reading in this module's
    docstring).  Raises ``PredictiveUnsupported`` where the survival count simulator does not take the engine."""
    from ..engine import PredictiveUnsupported

    n_draws = int(n_draws)
    if n_draws < 1:
        raise ValueError(f"n_draws must be >= 1, got {n_draws}")
    if not engine.survival_predictive_supported:
        raise PredictiveUnsupported(f"a survival predictive check is not available for this engine ({engine.family}"
                                    f"{', survival' if engine.survival else ', sorting'})")
    data = engine.data
    observed = {"X": engine._keep["X"]}
    if engine.use_bcmatch:
        observed["X_bcmatch"] = engine._keep["X_BC"]
    masks = {"repguide": data.repguide_mask, "sample": data.sample_mask, "mask_thres": int(engine._shape.mask_thres)}
    mid = torch.as_tensor(engine._keep["TIMEPOINTS"]).double().reshape(-1)
    return predictive_summary(observed, (engine.simulate_survival(d, seed=seed) for d in range(n_draws)), masks, mid)


def write_predictive_tables(summary: Dict[str, torch.Tensor], guide_info_df, data, prefix: str, model_label: str,
                            suffix: str = ""):
    """``bean_predictive_guides.<model>.csv``: one row per guide, the columns of ``guide_info_df`` (the sgRNA table)
    followed by the guide-level columns; ``bean_predictive_samples.<model>.csv``: one row per sample.  Returns the two
    paths."""
    import pandas as pd

    sfx = [s for s in ("", "_bcmatch") if "ppc_p_score" + s in summary]
    guides = guide_info_df.copy()
    if len(guides) != int(summary["ppc_p_score"].numel()):
        raise ValueError(f"the summary has {int(summary['ppc_p_score'].numel())} guides, the sgRNA table {len(guides)}")
    for s in sfx:
        for col in GUIDE_COLUMNS:
            guides[col + s] = summary[col + s].detach().cpu().numpy()
    R, B = int(data.n_reps), int(data.n_condits)
    samples = getattr(getattr(data, "screen", None), "samples", None)
    if samples is not None and len(samples) == R * B:  # sorted by replicate, then condition, as the tensors are
        index = pd.Index([str(i) for i in samples.index], name="sample")
    else:
        index = pd.Index([f"r{r}_c{b}" for r in range(R) for b in range(B)], name="sample")
    table = pd.DataFrame({"replicate": [r for r in range(R) for _ in range(B)],
                          "condition": [b for _ in range(R) for b in range(B)]}, index=index)
    table["masked"] = (torch.as_tensor(data.sample_mask).reshape(-1).cpu().numpy() == 0)
    for s in sfx:
        for col in SAMPLE_COLUMNS:
            table[col + s] = summary[col + s].detach().cpu().reshape(-1).numpy()
    table["n_draws"] = int(summary["n_draws"])
    paths = (f"{prefix}bean_predictive_guides.{model_label}{suffix}.csv",
             f"{prefix}bean_predictive_samples.{model_label}{suffix}.csv")
    guides.to_csv(paths[0])
    table.to_csv(paths[1])
    return paths
