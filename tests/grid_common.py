"""Shared by test_grid_posterior_cpu.py and test_gpu_grid_posterior.py: an engine that serves HipSVI.marginal_grid from
the CPU rule (marginal_reference.marginal_log_joint, one target at a time), and the bound both hold grid_posterior to.
A plain module imported by bare name."""
import math

import torch

import importance_common as ic
import marginal_reference as mr
from oracle import elbo


def node_coords(centre, step, n):
    """The library's node coordinates of one target's axis, float64."""
    return float(centre) + (torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0) * float(step)


class RuleEngine:
    """What grid_posterior asks of an engine - ``unconstrained`` and ``marginal_grid`` - on ``targets`` of ``data``
    (MixtureNormal, alpha_pi at its initial value, Laplace prior or the Normal / LogNormal of ``prior_params``), started
    at (mu_loc, sd_loc) = (0, 0)."""

    def __init__(self, data, targets, n_unresolved=None, prior_params=None):
        c_p = mr.model_conc(data, elbo.init_params("MixtureNormal", data))
        self.subs = []
        for t in targets:
            idx = ic.target_guides(data, t)
            self.subs.append((elbo.as_float64(data[idx]), c_p[idx]))
        T = len(targets)
        self.unconstrained = {"mu_loc": torch.zeros(T, 1), "sd_loc": torch.zeros(T, 1)}
        self.n_unresolved = torch.zeros(T, dtype=torch.int32) if n_unresolved is None else n_unresolved
        self.calls = []
        # per-target priors as HipSVI keeps them; served by the oracle's own distributions in place of the default ones
        self.prior_params = prior_params

    def marginal_grid(self, centre_mu, centre_y, step_mu, step_y, n_mu, n_y, nodes=32, pairs=False):
        self.calls.append((n_mu, n_y, nodes))
        lj = torch.empty((n_mu, n_y, len(self.subs)), dtype=torch.float64)
        for j, (sub, cp) in enumerate(self.subs):
            MU, Y = torch.meshgrid(node_coords(centre_mu[j], step_mu[j], n_mu), node_coords(centre_y[j], step_y[j], n_y),
                                   indexing="ij")
            mu, y = MU.reshape(-1), Y.reshape(-1)
            one = mr.marginal_log_joint(sub, cp, mu, y, Q=nodes)
            if self.prior_params is not None:
                own = {k: torch.as_tensor(v).double().reshape(-1)[j] for k, v in self.prior_params.items()}
                (d_mu, d_sd), (p_mu, p_sd) = elbo._priors((mu.numel(),), 0.01, None), elbo._priors((mu.numel(),), 0.01, own)
                one = one - d_mu.log_prob(mu) - d_sd.log_prob(y.exp()) + p_mu.log_prob(mu) + p_sd.log_prob(y.exp())
            lj[:, :, j] = one.reshape(n_mu, n_y)
        return {"lj": lj, "n_unresolved": self.n_unresolved}


def assert_meets_exact(res, j, ex, what):
    """Target j of ``res`` (grid_posterior) against ``ex`` (marginal_reference.exact_marginal_moments): it is grid_ok;
    |mu_grid - exact mean| and |mu_sd_grid - exact sd| are each at most the sum of the two quadratures' own
    step-doubling moves plus 1e-9; every one of those moves is below 1e-3 sd, so the bound cannot hide a failure."""
    f = lambda k: float(res[k][j])  # noqa: E731
    assert bool(res["grid_ok"][j]), (what, {k: f(k) for k in ("grid_border", "grid_step_shift", "grid_resolved")})
    assert ex["border"] < 1e-6 and f("grid_border") < 1e-6
    moves = {"mean": (abs(ex["mean"] - ex["mean_coarse"]), abs(f("mu_grid") - f("mu_grid_coarse"))),
             "sd": (abs(ex["sd"] - ex["sd_coarse"]), abs(f("mu_sd_grid") - f("mu_sd_grid_coarse")))}
    diff = {"mean": abs(f("mu_grid") - ex["mean"]), "sd": abs(f("mu_sd_grid") - ex["sd"])}
    print(f"{what}: mu_grid {f('mu_grid'):.9f} exact {ex['mean']:.9f} |diff| {diff['mean']:.2e} (moves: exact "
          f"{moves['mean'][0]:.2e}, grid {moves['mean'][1]:.2e}); mu_sd_grid {f('mu_sd_grid'):.9f} exact {ex['sd']:.9f} "
          f"|diff| {diff['sd']:.2e} (moves: exact {moves['sd'][0]:.2e}, grid {moves['sd'][1]:.2e}); border "
          f"{f('grid_border'):.2e}; step shift {f('grid_step_shift'):.2e}")
    for k, (a, b) in moves.items():
        assert a < 1e-3 * ex["sd"] and b < 1e-3 * ex["sd"], (what, k, a, b, ex["sd"])
        assert diff[k] <= a + b + 1e-9, (what, k, diff[k], a, b)
    assert math.isfinite(f("log_evidence_grid")) and 0.0 <= f("p_mu_pos_grid") <= 1.0
