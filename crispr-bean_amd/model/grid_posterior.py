"""Grid posterior of ``(mu, sd)`` per target, ``pi`` integrated out.

In the sorting variant families the targets share no parameter; with the editing rates integrated out of the model
(``csrc/bean_importance_marg.hpp``) the posterior of a target is a function of two numbers, ``(mu_t, y_t = log sd_t)``.
``HipSVI.marginal_grid`` (``csrc/bean_grid.hpp``) evaluates its log joint at given nodes; this module places the nodes
and reads the result - pure torch float64, vectorised over targets, on whatever device the values live, with a fixed
number of passes and no host synchronisation.

* ``grid_summary``: posterior mean and sd of ``mu``, posterior mean of ``sd``, ``P(mu > 0 | x)`` and the log evidence of a
  target from the log joint on its grid, with the two diagnostics of the quadrature - the largest density on the grid's
  border relative to the peak, and how far the mean moves when every second grid line is dropped.
* ``grid_posterior``: zoom passes from the fitted guide's location towards the mass of each target, axis by axis, then
  the final grid and its summary; the same on the line ``mu = 0`` gives the evidence of the null and the Bayes factor.

No guide enters: the numbers are what ``mu_sd``, ``mu_is_marg`` and ``mu_boot_se`` each approximate.  A zoom follows one
peak: a second mode of ``mu`` outside the final box is not detected.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

BORDER_MAX = 1e-6      # the bar tests/marginal_reference.py::assert_marginal_claim sets for its reference grid
STEP_SHIFT_MAX = 1e-3  # |mean - mean from every second grid line| / sd
START_HALF_WIDTH = (4.0, 1.0)  # of the first zoom box, in mu and in y
TAIL_BOUND = 1e-3      # nat per tail pair: the bound section 21 sets for a pair's log integral
TAIL_KEYS = ("n_pairs_tail", "grid_tail_err")  # the columns --grid-tail-rule adds behind GRID_KEYS
GRID_KEYS = ("mu_grid", "mu_sd_grid", "sd_grid", "p_mu_pos_grid", "log_evidence_grid", "log_bf10_grid", "grid_ok")


def _coords(centre: torch.Tensor, step: torch.Tensor, n: int) -> torch.Tensor:
    """(n, T): the library's node coordinates of an axis."""
    i = torch.arange(n, dtype=torch.float64, device=centre.device) - (n - 1) / 2.0
    return centre.unsqueeze(0) + i.unsqueeze(1) * step.unsqueeze(0)


def _axis_moments(w: torch.Tensor, x: torch.Tensor):
    """Mean and sd per target of the coordinates ``x`` (n, T) under the weights ``w`` (n, T), each column summing to 1."""
    mean = (w * x).sum(0)
    return mean, (w * (x - mean) ** 2).sum(0).clamp_min(0.0).sqrt()


def _as_t(v, like: torch.Tensor) -> torch.Tensor:
    return torch.as_tensor(v, dtype=torch.float64).to(like.device).reshape(-1)


def _tail_err_where_it_counts(lj: torch.Tensor, tail_err: torch.Tensor) -> torch.Tensor:
    """(T,): the largest ``tail_err`` over the nodes whose density is at least ``BORDER_MAX`` of the target's peak;
    ``lj`` and ``tail_err`` are (nodes, T)."""
    counts = (lj - lj.max(0).values) >= math.log(BORDER_MAX)
    return torch.where(counts, tail_err, torch.zeros_like(tail_err)).max(0).values


def grid_summary(lj: torch.Tensor, centre_mu, centre_y, step_mu, step_y, tail_err=None) -> Dict[str, torch.Tensor]:
    """Per target, from ``lj`` (n_mu, n_y, T) - ``HipSVI.marginal_grid`` on the grid of these centres and steps:

    * ``mu_grid``, ``mu_sd_grid``: posterior mean and sd of ``mu``; ``sd_grid``: the posterior mean of ``exp(y)``;
    * ``p_mu_pos_grid``: ``P(mu > 0 | x)``.  The indicator is not smooth, so its plain sum over the nodes is first order
      in the step; the sum is taken of the difference between the marginal of ``mu`` and the Gaussian of its two grid
      moments on the same nodes, and that Gaussian's own probability is added in closed form (exact for a Gaussian
      marginal; a node at 0 counts half);
    * ``log_evidence_grid``: the log-sum-exp over the nodes plus ``log(step_mu step_y)`` (an axis of one node: its step
      is left out - the integral runs over the other axis alone);
    * ``grid_border``: the largest density on the border of the grid relative to the peak (an axis of one node has no
      border); ``grid_step_shift``: ``|mu_grid - the same from every second grid line| / mu_sd_grid`` (0 where the sd
      is 0), with ``mu_grid_coarse`` / ``mu_sd_grid_coarse`` the moments behind it;
    * ``grid_ok``: ``grid_border < 1e-6`` and ``grid_step_shift < 1e-3``;
    * with ``tail_err`` (n_mu, n_y, T) - ``HipSVI.marginal_grid(tail_rule=True)`` - ``grid_tail_err``: the largest
      ``tail_err`` over the nodes whose density is at least 1e-6 of the target's peak (the bar of ``grid_border``: what
      lies below it does not enter the summary at that precision either).

    Every value of a target is a function of that target's ``lj`` alone."""
    lj = torch.as_tensor(lj).double()
    if lj.dim() != 3:
        raise ValueError(f"grid_summary: lj must be (n_mu, n_y, T), got shape {tuple(lj.shape)}")
    n_mu, n_y, T = lj.shape
    c_mu, c_y, s_mu, s_y = (_as_t(v, lj) for v in (centre_mu, centre_y, step_mu, step_y))
    for name, v in (("centre_mu", c_mu), ("centre_y", c_y), ("step_mu", s_mu), ("step_y", s_y)):
        if v.numel() != T:
            raise ValueError(f"grid_summary: {name} has {v.numel()} entries for {T} targets")
    mus, ys = _coords(c_mu, s_mu, n_mu), _coords(c_y, s_y, n_y)

    def moments(l, m):
        w = torch.softmax(l.reshape(-1, T), 0).reshape(l.shape)
        return _axis_moments(w.sum(1), m), w

    (mean, sd), w = moments(lj, mus)
    (mean2, sd2), _ = moments(lj[::2, ::2], mus[::2])
    if n_mu == 1:  # one line of mu: its spread is 0, not the rounding of weights that sum to 1
        sd, sd2 = torch.zeros_like(sd), torch.zeros_like(sd2)
    w_mu = w.sum(1)                                                                       # (n_mu, T)
    ind = (mus > 0).double() + 0.5 * (mus == 0).double()
    some = sd > 0
    safe = torch.where(some, sd, torch.ones_like(sd))
    g = torch.softmax(-0.5 * ((mus - mean) / safe) ** 2, 0)
    p_gauss = 0.5 * torch.erfc(-mean / safe / math.sqrt(2.0))
    p_pos = torch.where(some, p_gauss + ((w_mu - g) * ind).sum(0), (w_mu * ind).sum(0)).clamp(0.0, 1.0)
    cell = (s_mu.abs().log() if n_mu > 1 else 0.0) + (s_y.abs().log() if n_y > 1 else 0.0)
    peak = lj.reshape(-1, T).max(0).values
    edges = ([lj[0], lj[-1]] if n_mu > 1 else []) + ([lj[:, 0], lj[:, -1]] if n_y > 1 else [])
    border = ((torch.cat(edges).max(0).values - peak).exp() if edges else torch.zeros_like(peak))
    shift = torch.where(some, (mean - mean2).abs() / safe, torch.zeros_like(sd))
    extra = {}
    if tail_err is not None:
        te = torch.as_tensor(tail_err).double().to(lj.device)
        if te.shape != lj.shape:
            raise ValueError(f"grid_summary: tail_err has shape {tuple(te.shape)}, lj {tuple(lj.shape)}")
        extra["grid_tail_err"] = _tail_err_where_it_counts(lj.reshape(-1, T), te.reshape(-1, T))
    return {
        **extra,
        "mu_grid": mean,
        "mu_sd_grid": sd,
        "sd_grid": (w.sum(0) * ys.exp()).sum(0),
        "p_mu_pos_grid": p_pos,
        "log_evidence_grid": torch.logsumexp(lj.reshape(-1, T), 0) + cell,
        "grid_border": border,
        "grid_step_shift": shift,
        "mu_grid_coarse": mean2,
        "mu_sd_grid_coarse": sd2,
        "grid_ok": (border < BORDER_MAX) & (shift < STEP_SHIFT_MAX),
    }


def _zoom(engine, c_mu, c_y, h_mu, h_y, n_zoom: int, n_zm: int, n_zy: int, zoom_nodes: int, width: float, **kw):
    """``n_zoom`` passes of an ``n_zm x n_zy`` grid over the box ``centre +- half-width``; each axis on its own: where its
    moment sd is at least one step the axis is resolved - the new centre is the moment mean, the new half-width
    ``width`` sds - otherwise the new centre is the coordinate of the largest node and the new half-width two steps.
    An axis of one node is left as it is and counts as resolved."""
    T = c_mu.numel()
    ok_mu = torch.ones(T, dtype=torch.bool, device=c_mu.device)
    ok_y = ok_mu.clone()
    for _ in range(int(n_zoom)):
        s_mu = 2.0 * h_mu / (n_zm - 1) if n_zm > 1 else h_mu
        s_y = 2.0 * h_y / (n_zy - 1) if n_zy > 1 else h_y
        lj = engine.marginal_grid(c_mu, c_y, s_mu, s_y, n_zm, n_zy, nodes=zoom_nodes, **kw)["lj"].double()
        flat = lj.reshape(-1, T)
        w = torch.softmax(flat, 0).reshape(n_zm, n_zy, T)
        top = flat.argmax(0)
        for axis in (0, 1):
            n = (n_zm, n_zy)[axis]
            if n == 1:
                continue
            centre, step = ((c_mu, s_mu), (c_y, s_y))[axis]
            x = _coords(centre, step, n)
            mean, sd = _axis_moments(w.sum(1 - axis), x)
            at_top = x.gather(0, (top // n_zy if axis == 0 else top % n_zy).unsqueeze(0)).squeeze(0)
            ok = sd >= step
            new_c = torch.where(ok, mean, at_top)
            new_h = torch.where(ok, width * sd, 2.0 * step)
            if axis == 0:
                c_mu, h_mu, ok_mu = new_c, new_h, ok
            else:
                c_y, h_y, ok_y = new_c, new_h, ok
    return c_mu, c_y, h_mu, h_y, ok_mu & ok_y


def log_prior_mu_at_zero(engine, like: torch.Tensor) -> torch.Tensor:
    """(T,): ``log p(mu = 0)`` of the fit's prior on ``mu``: Laplace(0, 1), or the Normal of the engine's ``prior_params``
    (``mu_loc`` default 0, ``mu_scale`` default 1), each one value or one per target as the engine binds them - any other
    length is a ``ValueError``, never a silently biased Bayes factor."""
    T = like.numel()
    pp = getattr(engine, "prior_params", None)
    if pp is not None and ("mu_loc" in pp or "mu_scale" in pp):
        def per_target(key, default):
            if key not in pp:
                return torch.full_like(like, default)
            v = _as_t(pp[key], like)
            if v.numel() == 1:
                return v.expand(T)
            if v.numel() != T:
                raise ValueError(f"grid_posterior: prior_params[{key!r}] has {v.numel()} entries for {T} targets")
            return v

        loc, scale = per_target("mu_loc", 0.0), per_target("mu_scale", 1.0)
        return -0.5 * (loc / scale) ** 2 - scale.log() - 0.5 * math.log(2.0 * math.pi)
    return torch.full((T,), -math.log(2.0), dtype=torch.float64, device=like.device)


def grid_posterior(engine, nodes: int = 32, zoom_nodes: int = 16, n_zoom: int = 5, n_z: int = 17, n_mu: int = 41,
                   n_y: int = 21, width: float = 6.5, tail_rule: bool = False) -> Dict[str, torch.Tensor]:
    """The grid posterior of every target of ``engine`` (anything with ``unconstrained`` and ``marginal_grid``):

    1. start at ``(mu_loc_t, sd_loc_t)`` of the engine's parameters with half-widths (4, 1);
    2. ``n_zoom`` zoom passes of ``n_z x n_z`` nodes with ``zoom_nodes`` quadrature nodes (``_zoom``);
    3. the final ``n_mu x n_y`` grid over the last box with ``nodes`` quadrature nodes, through ``grid_summary``;
    4. the same on the line ``mu = 0`` (one node of ``mu``, ``y`` zoomed the same way, ``n_y`` nodes at the end):
       ``log_evidence_null_grid = log int p(x | mu = 0, y) p(y) dy`` - the 1-D log-sum-exp plus ``log step_y`` less
       ``log p(mu = 0)`` - and ``log_bf10_grid = log_evidence_grid - log_evidence_null_grid``.

    A target is ``grid_ok`` when both axes were resolved in the last zoom pass, ``grid_border < 1e-6`` and
    ``grid_step_shift < 1e-3``; the Bayes factor also needs the same of the null line.  The values of a target that is
    not, or that has ``n_unresolved > 0``, are NaN; the diagnostics (``grid_border``, ``grid_step_shift``,
    ``grid_resolved``, ``n_pairs_unresolved``, the box) are kept.  Device tensors of length T; no host
    synchronisation.

    ``tail_rule=True``: every pass - the zooms and the null line included - is ``marginal_grid(tail_rule=True)``, the
    Gauss-Jacobi rule for the pairs ``n_unresolved`` counts (``n_pairs_tail``).  A target with such pairs then gets
    numbers if it passes the three checks above and ``grid_tail_err <= 1e-3 n_pairs_tail`` - section 21's bound of 1e-3
    nat per pair, times the target's tail pairs; ``log_bf10_grid`` needs the null line to pass the same bar
    (``grid_null_tail_err``).  Otherwise its values are NaN and the diagnostics are kept.  (Each library call then
    synchronises the engine's stream once.)"""
    kw = {"tail_rule": True} if tail_rule else {}
    P = engine.unconstrained
    c_mu = P["mu_loc"].detach().double().reshape(-1)
    c_y = P["sd_loc"].detach().double().reshape(-1).to(c_mu.device)
    h_mu = torch.full_like(c_mu, START_HALF_WIDTH[0])
    h_y = torch.full_like(c_mu, START_HALF_WIDTH[1])
    c_mu, c_y2, h_mu, h_y2, resolved = _zoom(engine, c_mu, c_y, h_mu, h_y, n_zoom, n_z, n_z, zoom_nodes, width, **kw)
    s_mu, s_y = 2.0 * h_mu / max(n_mu - 1, 1), 2.0 * h_y2 / max(n_y - 1, 1)
    out = engine.marginal_grid(c_mu, c_y2, s_mu, s_y, n_mu, n_y, nodes=nodes, **kw)
    summary = grid_summary(out["lj"], c_mu, c_y2, s_mu, s_y, tail_err=out["tail_err"] if tail_rule else None)
    n_un = torch.as_tensor(out["n_unresolved"]).to(c_mu.device)

    # the null line: mu = 0
    zero, one = torch.zeros_like(c_mu), torch.ones_like(c_mu)
    _, c_y0, _, h_y0, resolved0 = _zoom(engine, zero, c_y, one, h_y, n_zoom, 1, n_z, zoom_nodes, width, **kw)
    s_y0 = 2.0 * h_y0 / max(n_y - 1, 1)
    out0 = engine.marginal_grid(zero, c_y0, one, s_y0, 1, n_y, nodes=nodes, **kw)
    lj0 = out0["lj"].double().reshape(n_y, -1)
    peak0 = lj0.max(0).values
    border0 = (torch.maximum(lj0[0], lj0[-1]) - peak0).exp()
    line = lambda l, s: torch.logsumexp(l, 0) + s.log()  # noqa: E731
    ev0 = line(lj0, s_y0)
    ev0_coarse = line(lj0[::2], 2.0 * s_y0)
    log_p0 = log_prior_mu_at_zero(engine, c_mu)
    null_ok = resolved0 & (border0 < BORDER_MAX) & ((ev0 - ev0_coarse).abs() < STEP_SHIFT_MAX)

    if tail_rule:
        bar = TAIL_BOUND * n_un.to(torch.float64)
        tail_err0 = _tail_err_where_it_counts(lj0, torch.as_tensor(out0["tail_err"]).double().to(lj0.device).reshape(n_y, -1))
        tail_ok = summary["grid_tail_err"] <= bar
        null_ok = null_ok & (tail_err0 <= bar)
        ok = resolved & summary["grid_ok"] & tail_ok
    else:
        ok = resolved & summary["grid_ok"] & (n_un == 0)
    nan = torch.full_like(c_mu, math.nan)
    res = {k: torch.where(ok, summary[k], nan) for k in ("mu_grid", "mu_sd_grid", "sd_grid", "p_mu_pos_grid",
                                                         "log_evidence_grid")}
    res["log_evidence_null_grid"] = torch.where(ok & null_ok, ev0 - log_p0, nan)
    res["log_bf10_grid"] = res["log_evidence_grid"] - res["log_evidence_null_grid"]
    res["grid_ok"] = ok
    res["n_pairs_unresolved"] = n_un.to(torch.float64)
    res.update({k: summary[k] for k in ("grid_border", "grid_step_shift", "mu_grid_coarse", "mu_sd_grid_coarse")})
    res.update({"grid_resolved": resolved, "grid_null_ok": null_ok, "grid_null_border": border0,
                "log_evidence_null_step_move": (ev0 - ev0_coarse).abs(), "grid_null_centre_y": c_y0,
                "grid_null_step_y": s_y0,
                "grid_centre_mu": c_mu, "grid_centre_y": c_y2, "grid_step_mu": s_mu, "grid_step_y": s_y})
    if tail_rule:
        res.update({"n_pairs_tail": n_un.to(torch.float64), "grid_tail_err": summary["grid_tail_err"],
                    "grid_tail_ok": tail_ok, "grid_null_tail_err": tail_err0})
    return res
