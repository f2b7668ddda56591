"""Shared by test_grid_tail_cpu.py and test_gpu_grid_tail.py: screens with essentially unedited guides, and an engine that
serves HipSVI.marginal_grid(tail_rule=True) from the CPU rule (tail_reference.py).  A plain module imported by bare
name."""
import math

import torch

import grid_common as gc
import importance_common as ic
import marginal_reference as mr
import tail_reference as tr
from oracle import elbo

LOG2 = math.log(2.0)
UNEDITED = (2.0 * LOG2, -5.0 * LOG2)  # alpha_pi = (log 4, log 1/32): c_p1 = pi_a0 / 129


def zero_control_counts(data, guides, allele=1):
    """The control reads of ``allele`` (1: edited; 0: unedited; None: both) of ``guides`` set to 0, in a copy of the
    tensor: ``data`` itself is this test's own screen."""
    ctrl = data.allele_counts_control.clone()
    for g in guides:
        if allele is None:
            ctrl[:, :, g, :] = 0
        else:
            ctrl[:, :, g, allele] = 0
    data.allele_counts_control = ctrl
    return data


def claim_screen_with_unedited_guides():
    """importance_common.claim_screen() (40 x 3, 8 targets of 5 guides) with the first guide of every target made
    unedited: its edited control reads zeroed, and alpha_pi = UNEDITED there (the initial value elsewhere).  Returns the
    screen and alpha_pi (G, 2) float32."""
    data = ic.claim_screen()
    first = [int(data.target_offsets[t]) for t in range(data.n_targets)]
    zero_control_counts(data, first, 1)
    alpha = elbo.init_params("MixtureNormal", data)["alpha_pi"].detach().clone().reshape(data.n_guides, 2).float()
    for g in first:
        alpha[g] = torch.tensor(UNEDITED)
    return data, alpha


class TailRuleEngine:
    """gc.RuleEngine with alpha_pi given and the combined rule inside: ``marginal_grid(..., tail_rule=True)`` serves
    tail_reference.marginal_log_joint and its tail_err, ``tail_rule=False`` marginal_reference's."""

    def __init__(self, data, alpha_pi, targets):
        c_p = mr.model_conc(data, {"alpha_pi": alpha_pi})
        self.subs, n_un = [], []
        full = mr.n_unresolved(data, {"alpha_pi": alpha_pi})
        for t in targets:
            idx = ic.target_guides(data, t)
            self.subs.append((elbo.as_float64(data[idx]), c_p[idx]))
            n_un.append(int(full[t]))
        T = len(targets)
        self.unconstrained = {"mu_loc": torch.zeros(T, 1), "sd_loc": torch.zeros(T, 1)}
        self.n_unresolved = torch.tensor(n_un, dtype=torch.int32)
        self.prior_params = None
        self.calls = []

    def marginal_grid(self, centre_mu, centre_y, step_mu, step_y, n_mu, n_y, nodes=32, pairs=False, tail_rule=False):
        self.calls.append((n_mu, n_y, nodes, tail_rule))
        T = len(self.subs)
        lj = torch.empty((n_mu, n_y, T), dtype=torch.float64)
        err = torch.zeros((n_mu, n_y, T), dtype=torch.float64)
        for j, (sub, cp) in enumerate(self.subs):
            MU, Y = torch.meshgrid(gc.node_coords(centre_mu[j], step_mu[j], n_mu),
                                   gc.node_coords(centre_y[j], step_y[j], n_y), indexing="ij")
            mu, y = MU.reshape(-1), Y.reshape(-1)
            if tail_rule:
                one, e = tr.marginal_log_joint(sub, cp, mu, y, Q=nodes, with_err=True)
                err[:, :, j] = e.reshape(n_mu, n_y)
            else:
                one = mr.marginal_log_joint(sub, cp, mu, y, Q=nodes)
            lj[:, :, j] = one.reshape(n_mu, n_y)
        out = {"lj": lj, "n_unresolved": self.n_unresolved}
        if tail_rule:
            out["tail_err"] = err
        return out
