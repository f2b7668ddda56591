"""The planted-sample ranking of the sample jackknife on the CPU oracle (no GPU):

    python scripts/oracle_planted_sample.py [--steps 300] [--corruption shuffle|by-edit-rate] [--scale 8]

`make_sorting_variant_screen(640, 3, seed=2)` with the counts of sample (1, 2) permuted across guides (a fixed
permutation: the signal is destroyed) and multiplied by `--scale` (1 keeps the depth; 8, the default, is what the test
plants: an over-amplified sample whose depth the screen's size factors, which stay as they were, do not describe) is
fitted whole and with each of its R x B samples left out
(model/jackknife.py::leave_out_samples) by oracle/svi.py, MixtureNormal, every fit from the same torch seed.  Printed: the
influence table of sample_jackknife_summary, most influential sample first.  tests/test_gpu_sample_jackknife.py asserts
on the GPU fits only that the planted sample comes first; this is where that ranking was looked at before the assertion
was written.
"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bean_amd  # noqa: E402,F401
from bean_amd.model.jackknife import leave_out_samples, sample_groups, sample_jackknife_summary  # noqa: E402
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen  # noqa: E402
from oracle import elbo, svi  # noqa: E402

PLANTED = (1, 2)


def permutation(data, pair=PLANTED, mode="shuffle"):
    """The fixed permutation of the guides that is applied to the sample's counts.  "shuffle": a seeded random one.
    "by-edit-rate": the one that hands the sample's counts, smallest first, to the guides in the order of their observed
    editing rate in the control sample - every target's well-edited guides then look enriched in that bin."""
    r, b = pair
    G = int(data.n_guides)
    if mode == "shuffle":
        return torch.randperm(G, generator=torch.Generator().manual_seed(12345))
    if mode != "by-edit-rate":
        raise ValueError(mode)
    ctrl = data.allele_counts_control.sum((0, 1)).double()  # (G, 2): unedited, edited
    rate = ctrl[:, 1] / ctrl.sum(-1).clamp(min=1.0)
    perm = torch.empty(G, dtype=torch.int64)
    perm[torch.argsort(rate, stable=True)] = torch.argsort(data.X[r, b].double(), stable=True)
    return perm


def plant(data, pair=PLANTED, mode="shuffle", scale=1.0):
    """The screen with the counts of sample `pair` permuted across guides by a fixed permutation and multiplied by
    `scale` (all four count tensors alike; everything derived - size factors, a0, masks - stays as it was)."""
    r, b = pair
    perm = permutation(data, pair, mode)
    out = copy.copy(data)
    for name in ("X", "X_masked", "X_bcmatch", "X_bcmatch_masked"):
        v = getattr(data, name).clone()
        v[r, b] = v[r, b][perm] * scale
        setattr(out, name, v)
    return out


def constrained(params):
    return {k: (v.detach().exp() if k in ("mu_scale", "sd_scale", "alpha_pi") else v.detach().clone()) for k, v in params.items()}


def fit(data, steps, seed=101):
    torch.manual_seed(seed)
    params = elbo.init_params("MixtureNormal", data)
    torch.manual_seed(seed)
    svi.run_svi(elbo.mixture_normal_loss, data, params, num_steps=steps)
    return constrained(params)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--corruption", choices=("shuffle", "by-edit-rate"), default="shuffle")
    ap.add_argument("--scale", type=float, default=8.0)
    a = ap.parse_args()
    data = plant(make_sorting_variant_screen(640, 3, seed=2), mode=a.corruption, scale=a.scale)
    groups, names = sample_groups(data, "sample")
    full = fit(data, a.steps)
    loo = [fit(leave_out_samples(data, g), a.steps) for g in groups]
    inf = sample_jackknife_summary(full, loo, groups, names)["influence"]
    order = sorted(range(len(groups)), key=lambda j: -inf["influence_median"][j])
    print(f"{1 + len(groups)} oracle fits of {a.steps} steps; planted sample r{PLANTED[0]}_c{PLANTED[1]} ({a.corruption}, counts x {a.scale:g})")
    for j in order:
        print(f"{inf['left_out'][j]:8s} influence_median {inf['influence_median'][j]:.6f}  max {inf['influence_max'][j]:.4f}  "
              f"targets moved {inf['n_targets_moved'][j]}")


if __name__ == "__main__":
    main()
