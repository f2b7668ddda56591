"""tests/grad_bounds.py on the host: the per-element tolerance is far above the oracle's own rounding noise, it catches a
relative error of 1e-5 in one element that the max-norm bound of the parity tests lets through, and the branch
classifier follows torch's rule at its edges."""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
import grad_bounds as gb
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen
from oracle import elbo


@pytest.fixture(scope="module")
def evaluation():
    """MixtureNormal with accessibility at 130 x 2, three guides per target, at the fitted-like point, on torch's draws."""
    data = make_sorting_variant_screen(130, 2, seed=31, guides_per_target=3, with_accessibility=True)
    kw = dict(scale_by_accessibility=True)
    g = torch.Generator().manual_seed(7)
    params = {k: (v.detach() + 0.3 * torch.randn(v.shape, generator=g)).float()
              for k, v in elbo.init_params("MixtureNormal", data, scale_by_acc=True).items()}
    params["alpha_pi"] = gb.fitted_like_alpha_pi(data, params["alpha_pi"], seed=7)
    c, _ = gb.variational_concentrations(data, params["alpha_pi"], survival=False)
    torch.manual_seed(5)
    T, G, R = data.n_targets, data.n_guides, data.n_reps
    noise = {"pi": torch.distributions.Dirichlet(c[None, None].expand(R, 1, -1, -1)).sample(),
             "eps_mu": torch.randn(T, 1, generator=g, dtype=torch.float64),
             "eps_sd": torch.randn(T, 1, generator=g, dtype=torch.float64),
             "eps_noise": torch.randn(G, generator=g, dtype=torch.float64)}
    d64 = elbo.as_float64(data)
    loss, ref, tol, tol_tail = gb.elementwise_bounds(elbo.mixture_normal_loss, d64, params, noise, kw)
    return dict(data=data, d64=d64, kw=kw, params=params, noise=noise, loss=loss, ref=ref, tol=tol, tol_tail=tol_tail)


def test_fitted_like_point_is_float32_and_reaches_every_branch(evaluation):
    e = evaluation
    assert e["params"]["alpha_pi"].dtype == torch.float32
    rate = e["params"]["alpha_pi"].double().softmax(-1)
    assert 0.9e-3 <= float(rate.min()) and float(rate.min(-1).values.max()) <= 0.5
    share_flipped = float((rate[:, 0] < rate[:, 1]).double().mean())
    assert 0.1 < share_flipped < 0.4  # a quarter of the guides have the other allele rare
    counts = gb.branch_counts(e["data"], e["params"]["alpha_pi"], e["noise"]["pi"])
    assert counts.sum() == 2 * 130 * 2 and counts.min() >= 0.1 * counts.sum(), counts
    assert all(np.isfinite(v).all() for v in e["ref"].values())


def test_bin_reversed_oracle_is_within_a_thousandth_of_the_tolerance(evaluation):
    """The oracle's own rounding noise, measured as the same oracle summing its bins in the other order."""
    e = evaluation
    _, alt, _, _ = gb.elementwise_bounds(elbo.mixture_normal_loss, gb.reverse_bins(e["d64"]), e["params"], e["noise"],
                                         e["kw"])
    for k, ref in e["ref"].items():
        assert np.all(np.abs(alt[k] - ref) <= e["tol"][k] / 1000.0), k
        assert np.all(e["tol"][k] > 0)


def test_planted_relative_error_fails_elementwise_and_passes_the_max_norm_bound(evaluation):
    """1e-5 of an element of median size is 5e-7 of the largest or less wherever the median is at most a twentieth of
    the largest: there the parity tests' bound cannot see it.  The per-element bound sees it in every tensor."""
    e = evaluation
    unseen = set()
    for k, ref in e["ref"].items():
        flat = np.abs(ref).reshape(-1)
        i = int(np.argsort(flat)[flat.size // 2])  # an element of median size
        got = ref.reshape(-1).copy()
        got[i] *= 1.0 + 1e-5
        err = np.abs(got - ref.reshape(-1))
        assert err[i] > e["tol_tail"][k].reshape(-1)[i], k  # fails the per-element bound, on either pathwise constant
        if flat[i] <= 0.05 * flat.max():
            assert err.max() <= 5e-7 * flat.max(), k        # passes the max-norm bound
            unseen.add(k)
    assert unseen >= {"alpha_pi", "noise_loc", "noise_scale"}, unseen  # the per-guide tensors, at the least


def test_branch_classifier_follows_torch_at_its_edges():
    """torch exposes no branch, but its value jumps where the formula changes (the approximations differ by 1e-6 ...
    1e-3 relative) and moves by rounding only where it does not: one ulp across each edge of the rule
    (boundary = 2.5 and 0.75, alpha = 6, beta = 6) the classifier must change class exactly where torch jumps."""
    def value(x, alpha, total):
        t = [torch.tensor([v], dtype=torch.float64) for v in (x, alpha, total)]
        return float(torch._dirichlet_grad(*t))

    below = lambda v: float(np.nextafter(v, 0.0))
    above = lambda v: float(np.nextafter(v, np.inf))
    # (x, alpha, total) on the edge and its neighbour across it, branch on the edge, branch across
    edges = [
        ((0.5, 5.0, 10.0), (0.5, 5.0, below(10.0)), "rational", "small_alpha"),      # boundary = 2.5, x <= 0.5
        ((0.75, 1.0, 4.0), (0.75, 1.0, below(4.0)), "rational", "small_beta"),       # boundary = 0.75, x >= 0.5
        ((0.5, 6.0, 20.0), (0.5, above(6.0), 20.0), "rational", "saddle"),           # alpha = 6
        ((0.5, 14.0, 20.0), (0.5, below(14.0), 20.0), "rational", "saddle"),         # beta = 6
        ((0.5, 0.8, 2.0), (above(0.5), 0.8, 2.0), "small_alpha", "small_beta"),      # x = 0.5, both series in reach
    ]
    for on, across, b_on, b_across in edges:
        assert gb.BRANCHES[int(gb.dirichlet_grad_branch(*on))] == b_on, on
        assert gb.BRANCHES[int(gb.dirichlet_grad_branch(*across))] == b_across, across
        v_on, v_across = value(*on), value(*across)
        assert abs(v_on - v_across) > 1e-9 * abs(v_on), (on, v_on, v_across)          # torch changes formula here
    # ... and one ulp inside a region torch's value moves by rounding only, the classifier not at all
    for p, q in [((0.3, 5.0, 10.0), (above(0.3), 5.0, 10.0)), ((0.5, 7.0, 20.0), (0.5, above(7.0), 20.0)),
                 ((0.9, 1.0, 4.0), (above(0.9), 1.0, 4.0)), ((0.6, 3.0, 8.0), (0.6, above(3.0), 8.0))]:
        assert gb.dirichlet_grad_branch(*p) == gb.dirichlet_grad_branch(*q)
        assert abs(value(*p) - value(*q)) <= 1e-12 * abs(value(*p)), (p, q)
