"""The direction of the power study on the CPU oracle (no GPU):

    python scripts/oracle_power_direction.py [--steps 300] [--screens 4] [--effects 1,1.5,2]

The 203-guide x 3-replicate screen of tests/test_gpu_power.py is fitted by oracle/svi.py (MixtureNormal).  From the fitted
model - the plug-in: mu_scale and sd_scale play no part, sd_t = exp(sd_loc), one pi ~ Dirichlet(q) per screen - screens
are drawn by tests/dm_reference.py::host_dm with mu_t set to 0 and to each candidate effect on EVERY target, with common
random numbers across the effects (one numpy seed per screen j), and refitted by the oracle with the fit's torch seed.
Printed per effect: the detection rate over (target, screen) - |mu_loc| / mu_scale >= 1.96 and, off the null, the
effect's sign - the mean mu_loc, and the medians over targets of |z| and of mu_scale.  tests/test_gpu_power.py asserts on
the GPU fits only the direction; this is where the effect it plants was chosen: the smallest candidate whose rate clears
the null's by a clear margin or, where none does at the test's 300 steps, the smallest candidate.
"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bean_amd  # noqa: E402,F401
import dm_reference as dm  # noqa: E402
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen  # noqa: E402
from oracle import elbo, svi  # noqa: E402


def fit(data, steps, seed=101):
    torch.manual_seed(seed)
    params = elbo.init_params("MixtureNormal", data)
    torch.manual_seed(seed)
    svi.run_svi(elbo.mixture_normal_loss, data, params, num_steps=steps)
    return elbo.constrained({k: v.detach() for k, v in params.items()})


def concentrations(data, P, mu_value, pi):
    """(2, R, B, G) float64: the Dirichlet-Multinomial concentrations of both likelihoods with mu_t = mu_value on every
    target, sd_t = exp(sd_loc), and the drawn pi (R, 1, G, 2) - the lines of oracle/elbo.py::mixture_normal_loss."""
    R, B, G, T = data.n_reps, data.n_condits, data.n_guides, data.n_targets
    mu_t = torch.full((T, 1), float(mu_value), dtype=P["sd_loc"].dtype)
    sd_t = P["sd_loc"].exp()
    mu = torch.repeat_interleave(torch.cat([torch.zeros((T, 1)), mu_t], -1), data.target_lengths, dim=0)
    sd = torch.repeat_interleave(torch.cat([torch.ones((T, 1)), sd_t], -1), data.target_lengths, dim=0)
    uq = data.upper_bounds[:, None, None].expand(-1, G, 2)
    lq = data.lower_bounds[:, None, None].expand(-1, G, 2)
    p_bin = elbo.std_normal_bin_prob(uq, lq, mu[None].expand(B, -1, -1), sd[None].expand(B, -1, -1))
    expected = (pi.expand(R, B, -1, -1) * p_bin[None]).sum(-1)
    a = elbo.dirmult_concentration(expected, data.size_factor, data.sample_mask, data.a0)
    a_bc = elbo.dirmult_concentration(expected, data.size_factor_bcmatch, data.sample_mask, data.a0_bcmatch)
    return torch.stack([a, a_bc]).permute(0, 1, 3, 2).double().numpy()  # (R, G, B) -> (R, B, G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--screens", type=int, default=4)
    ap.add_argument("--effects", default="1,1.5,2")
    a = ap.parse_args()
    effects = [0.0] + [float(e) for e in a.effects.split(",")]
    data = elbo.as_float64(make_sorting_variant_screen(203, 3, seed=11, mask_fraction=0.05, depth_per_guide=100.0))
    P = fit(data, a.steps)
    R, G = data.n_reps, data.n_guides
    q = (P["alpha_pi"] / P["alpha_pi"].sum(-1)[:, None] * data.pi_a0[:, None])[None, None].expand(R, 1, -1, -1).clamp(1e-5)
    n = data.X_masked.sum(1).numpy().astype(np.int64)
    n_bc = data.X_bcmatch_masked.sum(1).numpy().astype(np.int64)
    flat = lambda al: np.moveaxis(al, 1, 2).reshape(R * G, -1)  # noqa: E731  (R, B, G) -> (R G, B)
    back = lambda x: torch.as_tensor(np.moveaxis(x.reshape(R, G, -1), 2, 1)).to(data.X_masked.dtype)  # noqa: E731
    full_hits = float(((P["mu_loc"].abs() / P["mu_scale"]) >= 1.96).double().mean())
    print(f"the screen's own fit, {a.steps} steps: {full_hits:.3f} of {data.n_targets} targets at |z| >= 1.96")
    for e in effects:
        found, means, zs, scales = [], [], [], []
        for j in range(a.screens):
            torch.manual_seed(1000 + j)
            pi = torch.distributions.Dirichlet(q).sample()
            al = concentrations(data, P, e, pi)
            rng = np.random.default_rng(2000 + j)  # (the same streams at every effect)
            redrawn = copy.copy(data)
            redrawn.X_masked = back(dm.host_dm(n.reshape(-1), flat(al[0]), 1, rng)[0])
            redrawn.X_bcmatch_masked = back(dm.host_dm(n_bc.reshape(-1), flat(al[1]), 1, rng)[0])
            F = fit(redrawn, a.steps)
            m, s = F["mu_loc"].reshape(-1), F["mu_scale"].reshape(-1)
            hit = (m.abs() / s) >= 1.96
            if e != 0:
                hit &= torch.sign(m) == np.sign(e)
            found.append(float(hit.double().mean()))
            means.append(float(m.mean()))
            zs.append(float((m.abs() / s).median()))
            scales.append(float(s.median()))
        print(f"effect {e:g}: detection rate {np.mean(found):.3f} (per screen {[round(f, 3) for f in found]}), "
              f"mean mu_loc {np.mean(means):+.3f}, median |z| {np.mean(zs):.3f}, median mu_scale {np.mean(scales):.3f}",
              flush=True)


if __name__ == "__main__":
    main()
