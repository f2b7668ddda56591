"""Result tables: fitted parameters -> ``bean_element_result.*.csv`` /
``bean_sgRNA_result.*.csv``.

Restates ``bean/model/readwrite.py:9-246`` (same function names, arguments,
column names and row order) so that the HIP fit can be consumed exactly like the
reference's output.  Pinned by fixtures produced with the reference's own file
(``tests/golden/make_readwrite_golden.py``).  Quirk kept: ``"negctrl" in
param_hist_dict.keys()`` is never true, so the ``_adj`` columns always derive
from the unscaled ``mu`` / ``mu_sd``.
"""
from __future__ import annotations

from statistics import NormalDist
from typing import List, Optional, Sequence, Union

import numpy as np
import pandas as pd
from scipy.special import expit, logit
from scipy.stats import norm

ACC_A, ACC_B = 0.2513, -1.9458  # bean/model/readwrite.py:221-222


def get_novl(df: pd.DataFrame, mu_col: str, mu_sd_col: str) -> pd.Series:
    """1 - overlap of N(mu, mu_sd) with the standard normal, row by row."""
    std = NormalDist(mu=0, sigma=1)
    return df.apply(lambda r: 1 - NormalDist(mu=r[mu_col], sigma=r[mu_sd_col]).overlap(std), axis=1)


def get_quantile(mu, sd, q):
    return norm(mu, sd).ppf(q)


def add_credible_interval(df: pd.DataFrame, mu_col: str, mu_sd_col: str, alpha: float = 0.05) -> pd.DataFrame:
    out = df.copy()
    out[f"CI[{alpha/2}"] = get_quantile(out[mu_col], out[mu_sd_col], alpha / 2)
    out[f"{1-alpha/2}]"] = get_quantile(out[mu_col], out[mu_sd_col], 1 - alpha / 2)
    return out


def adjust_normal_params_by_control(param_df: pd.DataFrame, sd0: float, suffix: str = "_adj",
                                    mu_adjusted_col="mu", mu_sd_adjusted_col="mu_sd", mu0: float = 0.0):
    """Rescale the z-scores by the spread ``sd0`` of the negative-control z-scores."""
    param_df[f"mu{suffix}"] = param_df[mu_adjusted_col] - mu0
    param_df[f"mu_sd{suffix}"] = param_df[mu_sd_adjusted_col] * sd0
    param_df[f"mu_z{suffix}"] = param_df[f"mu{suffix}"] / param_df[f"mu_sd{suffix}"]
    param_df[f"novl{suffix}"] = get_novl(param_df, f"mu{suffix}", f"mu_sd{suffix}")
    return param_df


def _np(t):
    return t.detach().cpu().numpy()


def _scale_edited_pi(pi, guide_accessibility, a: float = ACC_A, b: float = ACC_B):
    return pi * np.exp(b) * guide_accessibility**a


def _add_noise_to_pi(pi, fitted_noise_logit):
    return expit(logit(pi.clip(min=1e-3, max=1 - 1e-3)) + fitted_noise_logit).clip(min=1e-3, max=1 - 1e-3)


def _scale_pi(pi, guide_acc, fitted_noise_logit=None):
    scaled = _scale_edited_pi(pi, guide_acc)
    return scaled if fitted_noise_logit is None else _add_noise_to_pi(scaled, fitted_noise_logit)


def _fitted_columns(P, sd_is_fitted: bool, covariates: Optional[List[str]]) -> pd.DataFrame:
    """One row per target: posterior mean / spread of mu, its z-score, the fitted sd, and - with sample covariates - the
    covariate-shifted copies of the three (variances add)."""
    loc = P["mu_loc"]
    if loc.dim() not in (1, 2):
        raise ValueError(f'`mu_loc` has invalid shape of {loc.shape}')
    first = (lambda arr: arr[:, 0]) if loc.dim() == 2 else (lambda arr: arr)
    centre, spread = first(_np(loc)), first(_np(P["mu_scale"]))
    table = {"mu": centre, "mu_sd": spread, "mu_z": centre / spread}
    if sd_is_fitted:
        table["sd"] = first(_np(P["sd_loc"].detach().exp()))
    if covariates is not None:
        assert "mu_cov_loc" in P and "mu_cov_scale" in P, P.keys()
        shift, shift_sd = _np(P["mu_cov_loc"]), _np(P["mu_cov_scale"])
        for i, name in enumerate(covariates):
            m = centre + shift[i]
            s_ = np.sqrt(spread**2 + shift_sd[i] ** 2)
            table.update({f"mu_{name}": m, f"mu_sd_{name}": s_, f"mu_z_{name}": m / s_})
    return pd.DataFrame(table)


def _rescale_by_control_fit(table: pd.DataFrame, negctrl_params, sd_is_fitted: bool,
                            covariates: Optional[List[str]]) -> None:
    """`_scaled` columns: the targets' posteriors in units of the common negative-control distribution (a separate
    ControlNormal fit: its mean and, when sd is fitted, its sd).  In place."""
    print("Normalizing with common negative control distribution")
    centre0 = _np(negctrl_params["mu_loc"]).mean()
    unit = _np(negctrl_params["sd_loc"].detach().exp()) if sd_is_fitted else 1.0
    print(f"Fitted mu0={centre0}" + (f", sd0={unit}." if sd_is_fitted else ""))
    table["mu_scaled"] = (table["mu"].values - centre0) / unit
    table["mu_sd_scaled"] = table["mu_sd"].values / unit
    table["mu_z_scaled"] = table.mu_scaled / table.mu_sd_scaled
    if sd_is_fitted:
        table["sd_scaled"] = table["sd"].values / unit
    table["novl_scaled"] = get_novl(table, "mu_scaled", "mu_sd_scaled")
    for name in covariates or ():
        table[f"mu_{name}_scaled"] = (table[f"mu_{name}"] - centre0) / unit
        table[f"mu_sd_{name}_scaled"] = table[f"mu_sd_{name}"] / unit
        table[f"mu_z_{name}_scaled"] = table[f"mu_{name}_scaled"] / table["mu_sd_scaled"]


def _ranked(table: pd.DataFrame, z_col: str) -> pd.DataFrame:
    """Rows by decreasing |z| (the reference's order: argsort of -|z|, missing values as pandas places them)."""
    return table.iloc[(-table[z_col].abs()).argsort()]


def _calibrated_by_negatives(table: pd.DataFrame, negatives, covariates: Optional[List[str]], from_scaled: bool) -> pd.DataFrame:
    """`_adj` columns: posterior spreads stretched by the spread of the negative-control VARIANTS' z-scores (a zero-mean
    normal fitted to them), then credible intervals and the |z| order.  Fewer than ten negatives: no calibration."""
    if len(negatives) < 10:
        print("Cannot adjust confidence by negative control due to too small number "
              f"({len(negatives)}) of negatives.")
        return _ranked(add_credible_interval(table, "mu", "mu_sd"), "mu_z")
    controls = table.iloc[negatives]
    if "mu_z_scaled" in controls.columns:
        print("Using mu_z_scaled for normalization input..")
        z_centre, z_spread = norm.fit(controls.mu_z_scaled, floc=0)
    else:
        z_centre, z_spread = norm.fit(controls.mu_z, floc=0)
    pick = (lambda base: base + "_scaled") if from_scaled else (lambda base: base)
    table = adjust_normal_params_by_control(table, z_spread, suffix="_adj", mu_adjusted_col=pick("mu"),
                                            mu_sd_adjusted_col=pick("mu_sd"), mu0=z_centre)
    table = _ranked(add_credible_interval(table, "mu_adj", "mu_sd_adj"), "mu_z_adj")
    for name in covariates or ():
        table = adjust_normal_params_by_control(table, z_spread, suffix=f"_{name}_adj",
                                                mu_adjusted_col=pick(f"mu_{name}"), mu_sd_adjusted_col=pick(f"mu_sd_{name}"))
        table = add_credible_interval(table, f"mu_{name}_adj", f"mu_sd_{name}_adj")
    return table


def _guide_editing_columns(guide_info_df: pd.DataFrame, P, guide_acc) -> None:
    """The sgRNA table's accessibility columns (in place): the fitted editing rate of every guide - the edited share of
    its `alpha_pi` - scaled by accessibility as the model scales it."""
    if guide_acc is None:
        return
    if "alpha_pi" in P.keys():
        conc = _np(P["alpha_pi"])
        edited_share = conc[..., 1:].sum(axis=1) / conc.sum(axis=1)
    else:
        edited_share = 1.0
    logit_noise = _np(P["noise_scale"]) if "noise_scale" in P.keys() else None
    guide_info_df.insert(1, "accessibility", guide_acc)
    guide_info_df.insert(2, "scaled_edit_eff", _scale_pi(edited_share, guide_acc, fitted_noise_logit=logit_noise))


def _flat(v) -> np.ndarray:
    return np.asarray(v.detach().cpu() if hasattr(v, "detach") else v, dtype=np.float64).reshape(-1)


def _add_summary_columns(element: pd.DataFrame, summary: dict, what: str, numeric: Sequence[str], names: Optional[str],
                         count: str, count_per_target: bool = False) -> None:
    """A member set's summary into the element table, in place and in this order: its ``numeric`` columns, its column
    of ``names`` (``None``: the set has none) and its ``count`` (one number or, ``count_per_target``, an int64 per
    target).  Every per-target entry must have the table's length."""
    n = [int(summary[count])] * len(element) if not count_per_target else _flat(summary[count]).astype(np.int64)
    columns = {**{k: _flat(summary[k]) for k in numeric}, **({names: list(summary[names])} if names else {}), count: n}
    if any(len(v) != len(element) for v in columns.values()):
        raise ValueError(f"{what} has {len(columns[numeric[0]])} entries for {len(element)} targets")
    for k, v in columns.items():
        element[k] = v


def write_result_table(
    target_info_df: pd.DataFrame,
    guide_info_df: pd.DataFrame,
    param_hist_dict,
    model_label: str,
    prefix: str = "",
    suffix: str = "",
    negctrl_params=None,
    adjust_confidence_by_negative_control: bool = True,
    adjust_confidence_negatives: Optional[np.ndarray] = None,
    guide_acc: Optional[Sequence] = None,
    sd_is_fitted: bool = True,
    sample_covariates: Optional[List[str]] = None,
    return_result: bool = False,
    is_survival_screen: bool = False,
    seed_sd=None,
    n_seeds: Optional[int] = None,
    jackknife: Optional[dict] = None,
    guide_jackknife: Optional[dict] = None,
    sample_jackknife: Optional[dict] = None,
    bootstrap: Optional[dict] = None,
    design: Optional[dict] = None,
    power: Optional[dict] = None,
    importance: Optional[dict] = None,
    grid: Optional[dict] = None,
) -> Union[pd.DataFrame, None]:
    """Combine target information and fitted scores into the element table (written
    or returned) and write the sgRNA table (``bean/model/readwrite.py:49-215``: same arguments, columns, row order
    and files; the steps are the helpers above).

    ``seed_sd`` / ``n_seeds`` (a seed ensemble, ``model/ensemble.py``): the element table gets the columns
    ``mu_seed_sd`` - the between-seed standard deviation of every target's ``mu`` - and ``n_seeds``.  Left at ``None``
    the tables are exactly those of a single fit.

    ``jackknife`` (a replicate jackknife, ``model/jackknife.py::jackknife_summary``): the element table gets exactly the
    columns ``mu_jk_se``, ``mu_jk_max_shift``, ``mu_jk_max_shift_rep`` and ``n_jk``; every other column and the sgRNA
    table are those of the run without it.  ``mu_jk_se`` and ``mu_jk_max_shift`` are statistics of the fits' ``mu_loc``,
    i.e. on the scale of the column ``mu``: with ``negctrl_params`` (``--fit-negctrl``) they are NOT rescaled with
    ``mu_scaled`` (divide by the control fit's sd to compare), nor stretched like ``mu_sd_adj``.

    ``guide_jackknife`` (a guide jackknife, ``model/jackknife.py::guide_jackknife_summary``): the element table gets
    exactly the columns ``mu_gjk_se``, ``mu_gjk_max_shift``, ``mu_gjk_max_shift_guide`` and ``n_gjk``, the sgRNA table
    the column ``mu_shift_left_out``; every other column of both is that of the run without it, and with ``None`` both
    tables are byte for byte what they were.  As the replicate columns, the numeric ones are on the scale of ``mu`` and
    are not rescaled with ``negctrl_params``.

    ``sample_jackknife`` (a sample jackknife, ``model/jackknife.py::sample_jackknife_summary``): the element table gets
    exactly the columns ``mu_sjk_max_shift``, ``mu_sjk_max_shift_sample`` and ``n_sjk`` (on the scale of ``mu``, not
    rescaled), and the summary's influence table - one row per left-out sample or condition - is written next to the
    element table as ``bean_sample_influence.<model_label><suffix>.csv``, also with ``return_result``.  With ``None``
    both tables are byte for byte what they were and no third one is written.

    ``bootstrap`` (a parametric bootstrap, ``model/jackknife.py::bootstrap_summary``): the element table gets exactly
    the columns ``mu_boot_se``, ``mu_boot_bias`` and ``n_boot`` (on the scale of ``mu``, not rescaled); every other
    column and the sgRNA table are those of the run without it.

    ``design`` (a depth study, ``model/jackknife.py::design_summary``): the element table gets exactly the columns
    ``mu_design_se_x{f:g}``, one per depth in the summary's order (on the scale of ``mu``, not rescaled), and the
    summary's table - one row per depth: ``depth, n_screens, median_total, median_mu_design_se, se_ratio, recovery,
    n_hits`` - is written next to the element table as ``bean_design.<model_label><suffix>.csv``, also with
    ``return_result``.  With ``None`` every file is byte for byte what it was and no further one is written.

    ``power`` (a power study, ``model/jackknife.py::power_summary``): the element table gets exactly the columns
    ``power_x{e:g}``, one per effect in the summary's order (the share of the refits that call the target; at effect 0 the
    false-positive rate), then ``mde{100 * level:g}`` (the minimal detectable effect at the summary's level: ``mde80``)
    and, where negative effects were given, ``mde{...}_neg``; the summary's table - one row per effect: ``effect,
    n_screens, n_planted, power_mean, power_median, shrinkage, median_mu_power_se`` - is written next to the element
    table as ``bean_power.<model_label><suffix>.csv``, also with ``return_result``.  With ``None`` every file is byte for
    byte what it was and no further one is written.

    ``importance`` (an importance-sampling check of the guide, ``model/importance.py::importance_summary``): the element
    table gets exactly the columns ``psis_k``, ``mu_is``, ``mu_sd_is``, ``is_ess`` and ``n_is`` (``mu_is`` / ``mu_sd_is``
    on the scale of ``mu``, not rescaled), after those of a member set; every other column and the sgRNA table are those
    of the run without it, and with ``None`` every file is byte for byte what it was.  Where the summary also holds the
    marginal check (``marginal_summary``: ``pi`` integrated out), ``psis_k_marg``, ``mu_is_marg``, ``mu_sd_is_marg``,
    ``is_ess_marg`` (empty for a target with unresolved pairs) and ``n_pairs_unresolved`` follow behind them, and where it
    holds ``is_tail_err`` (the tail rule) ``n_pairs_tail`` and ``is_tail_err`` behind those - ``n_pairs_tail`` once, also
    where ``grid`` holds it.

    ``grid`` (a grid posterior, ``model/grid_posterior.py::grid_posterior``): the element table gets the columns
    ``mu_grid``, ``mu_sd_grid``, ``sd_grid``, ``p_mu_pos_grid``, ``log_evidence_grid``, ``log_bf10_grid`` (on the scale of
    ``mu``, not rescaled; empty where ``grid_ok`` is 0 or the target has unresolved pairs), ``grid_ok`` (0 / 1) and, unless
    the marginal importance check has already written it, ``n_pairs_unresolved`` - behind the importance columns; with
    ``None`` every file is byte for byte what it was.  A grid posterior with the tail rule
    (``grid_posterior(tail_rule=True)``: it holds ``n_pairs_tail``) adds ``n_pairs_tail`` and ``grid_tail_err`` behind
    those; without them in ``grid`` nothing changes."""
    fitted = _fitted_columns(param_hist_dict, sd_is_fitted, sample_covariates)
    if negctrl_params is not None:
        _rescale_by_control_fit(fitted, negctrl_params, sd_is_fitted, sample_covariates)
    element = pd.concat([target_info_df.reset_index(), fitted.reset_index(drop=True)], axis=1)
    if seed_sd is not None or n_seeds is not None:
        if seed_sd is None or n_seeds is None:
            raise ValueError("seed_sd and n_seeds go together")
        spread = _flat(seed_sd)
        if len(spread) != len(element):
            raise ValueError(f"seed_sd has {len(spread)} entries for {len(element)} targets")
        element["mu_seed_sd"] = spread
        element["n_seeds"] = int(n_seeds)
    if jackknife is not None:
        _add_summary_columns(element, jackknife, "the jackknife summary", ("mu_jk_se", "mu_jk_max_shift"),
                             "mu_jk_max_shift_rep", "n_jk")
    if guide_jackknife is not None:
        per_guide = _flat(guide_jackknife["mu_shift_left_out"])
        if len(per_guide) != len(guide_info_df):
            raise ValueError(f"the guide jackknife summary has {len(per_guide)} entries for {len(guide_info_df)} guides")
        _add_summary_columns(element, guide_jackknife, "the guide jackknife summary", ("mu_gjk_se", "mu_gjk_max_shift"),
                             "mu_gjk_max_shift_guide", "n_gjk", count_per_target=True)
    if sample_jackknife is not None:
        _add_summary_columns(element, sample_jackknife, "the sample jackknife summary", ("mu_sjk_max_shift",),
                             "mu_sjk_max_shift_sample", "n_sjk")
    if bootstrap is not None:
        _add_summary_columns(element, bootstrap, "the bootstrap summary", ("mu_boot_se", "mu_boot_bias"), None, "n_boot")
    if design is not None:
        spread = np.asarray(design["mu_design_se"], dtype=np.float64)
        if spread.ndim != 2 or spread.shape != (len(design["depths"]), len(element)):
            raise ValueError(f"the depth study summary has shape {spread.shape} for {len(design['depths'])} depths and "
                             f"{len(element)} targets")
        for f, column in zip(design["depths"], spread):
            element[f"mu_design_se_x{float(f):g}"] = column
    if power is not None:
        rates = np.asarray(power["power"], dtype=np.float64)
        if rates.ndim != 2 or rates.shape != (len(power["effects"]), len(element)):
            raise ValueError(f"the power study summary has shape {rates.shape} for {len(power['effects'])} effects and "
                             f"{len(element)} targets")
        for e, column in zip(power["effects"], rates):
            element[f"power_x{float(e):g}"] = column
        mde = f"mde{100 * float(power['level']):g}"
        element[mde] = _flat(power["mde"])
        if "mde_neg" in power:
            element[mde + "_neg"] = _flat(power["mde_neg"])
    if importance is not None:
        _add_summary_columns(element, importance, "the importance-sampling summary",
                             ("psis_k", "mu_is", "mu_sd_is", "is_ess"), None, "n_is", count_per_target=True)
        if "psis_k_marg" in importance:
            # ... with pi integrated out (model/importance.py::marginal_summary): five more columns, behind those
            _add_summary_columns(element, importance, "the marginal importance-sampling summary",
                                 ("psis_k_marg", "mu_is_marg", "mu_sd_is_marg", "is_ess_marg"), None,
                                 "n_pairs_unresolved", count_per_target=True)
        if "is_tail_err" in importance:
            # ... with the Gauss-Jacobi rule at the unresolved pairs (marginal_summary(tail_err=...)): two more, behind
            element["n_pairs_tail"] = _flat(importance["n_pairs_tail"]).astype(np.int64)
            element["is_tail_err"] = _flat(importance["is_tail_err"]).astype(np.float64)
    if grid is not None:
        _add_summary_columns(element, grid, "the grid posterior summary",
                             ("mu_grid", "mu_sd_grid", "sd_grid", "p_mu_pos_grid", "log_evidence_grid", "log_bf10_grid"),
                             None, "grid_ok", count_per_target=True)
        if "n_pairs_unresolved" not in element.columns:
            element["n_pairs_unresolved"] = _flat(grid["n_pairs_unresolved"]).astype(np.int64)
        if "n_pairs_tail" in grid:
            # the Gauss-Jacobi rule for the unresolved pairs: how many pairs of the target took it, and the largest
            # disagreement of its two node counts where the posterior has mass
            if "n_pairs_tail" not in element.columns:  # (the marginal importance check's tail rule writes the same count)
                element["n_pairs_tail"] = _flat(grid["n_pairs_tail"]).astype(np.int64)
            element["grid_tail_err"] = _flat(grid["grid_tail_err"]).astype(np.float64)
    if adjust_confidence_by_negative_control:
        assert adjust_confidence_negatives is not None
        # (the reference asks the PARAMETER STORE for a "negctrl" key, which it never has: the `_adj` columns always
        # derive from the unscaled mu / mu_sd - SURVEY.md Appendix C item 4; kept, and pinned by the reference's own run)
        element = _calibrated_by_negatives(element, adjust_confidence_negatives, sample_covariates,
                                           from_scaled="negctrl" in param_hist_dict.keys())
    else:
        element = _ranked(add_credible_interval(element, "mu", "mu_sd"), "mu_z")
    _guide_editing_columns(guide_info_df, param_hist_dict, guide_acc)
    if guide_jackknife is not None:
        guide_info_df["mu_shift_left_out"] = per_guide
    guide_info_df.to_csv(f"{prefix}bean_sgRNA_result.{model_label}{suffix}.csv")
    if sample_jackknife is not None:
        pd.DataFrame(sample_jackknife["influence"]).to_csv(f"{prefix}bean_sample_influence.{model_label}{suffix}.csv",
                                                           index=False)
    if design is not None:
        pd.DataFrame({"depth": [float(f) for f in design["depths"]], "n_screens": int(design["n_screens"]),
                      "median_total": _flat(design["median_total"]),
                      "median_mu_design_se": np.median(spread, axis=1) if spread.shape[1] else np.full(len(spread), np.nan),
                      "se_ratio": _flat(design["se_ratio"]), "recovery": _flat(design["recovery"]),
                      "n_hits": int(design["n_hits"])}).to_csv(f"{prefix}bean_design.{model_label}{suffix}.csv", index=False)
    if power is not None:
        planted = ~np.isnan(rates[0]) if len(rates) else np.zeros(0, dtype=bool)
        se = np.asarray(power["mu_power_se"], dtype=np.float64)[:, planted]
        pd.DataFrame({"effect": [float(e) for e in power["effects"]], "n_screens": int(power["n_screens"]),
                      "n_planted": int(power["n_planted"]), "power_mean": _flat(power["power_mean"]),
                      "power_median": _flat(power["power_median"]), "shrinkage": _flat(power["shrinkage"]),
                      "median_mu_power_se": np.median(se, axis=1) if se.shape[1] else np.full(len(se), np.nan)}
                     ).to_csv(f"{prefix}bean_power.{model_label}{suffix}.csv", index=False)
    if return_result:
        return element
    element.to_csv(f"{prefix}bean_element_result.{model_label}{suffix}.csv")
