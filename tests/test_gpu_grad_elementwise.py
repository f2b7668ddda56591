"""Every element of every ELBO gradient against the float64 oracle, within the per-element tolerance of
tests/grad_bounds.py, at the usual `init + 0.3 randn` point and at a point a fit reaches (editing rates of 1e-3 ... 0.5,
where the implicit Dirichlet gradient leaves its saddle-point branch and the product kernels use the digamma tables that
k_param writes: DevArgs::dgq, dgq_t).  -m gpu.

The shapes are the smallest at which the kernels still split their work: 130 x 2 with 3 guides per target (three
64-guide tiles, one partial), 65 x 1, 257 x 3 with 100 guides per target (a target across tiles, DevArgs::tdesc), tiling
with 5 / 13 / 24 / 48 alleles per guide (the 8-, 16- and 32-allele builds and the allele-parallel kernel), survival
variant with and without accessibility, survival tiling.  The cases reach the five dirichlet_grad_one_pre call sites
(k_guide_wave2, k_guide_survival_wave, k_guide_tiling_rep, k_guide_tiling_wide, k_guide_tiling_wave) and, through the
A/B library's switches, the generic kernels that call dirichlet_grad_one (k_guide_wave, k_pi_terms behind k_lik,
k_guide_survival, k_guide_tiling).
"""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
import effect_regimes as er
import grad_bounds as gb
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                              make_survival_tiling_screen, make_survival_variant_screen)
from oracle import elbo
from oracle import survival as osurv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACC = dict(scale_by_accessibility=True)

MAKERS = {"variant": make_sorting_variant_screen, "tiling": make_sorting_tiling_screen,
          "survival": make_survival_variant_screen, "survival_tiling": make_survival_tiling_screen}
FAMILY = {"variant": "MixtureNormal", "tiling": "MultiMixtureNormal", "survival": "MixtureNormal",
          "survival_tiling": "MultiMixtureNormal"}
LOSS = {"variant": elbo.mixture_normal_loss, "tiling": elbo.multi_mixture_normal_loss,
        "survival": osurv.mixture_normal_loss, "survival_tiling": osurv.multi_mixture_normal_loss}

# Screens whose fitted-like point reaches every branch of the implicit gradient in expectation (torch's sampler, 30
# draws, on the host: at least 12 evaluations per branch and draw in every tiling and survival case, at least 18 % per
# branch in the variant cases).  One replicate of 65 guides at the default depth gives pi_a0 of 2 ... 60, which leaves the
# saddle-point branch (both concentrations above 6) 4 %; the tiling screens at the default depth give pi_a0 of 90 ... 400,
# which leaves the small-beta series (x >= 0.5, sum c x (1 - x) < 0.75) one evaluation in a thousand.
VARIANT = dict(n_guides=130, n_reps=2, guides_per_target=3, seed=31)
TILING_A5 = dict(n_guides=130, n_reps=2, n_max_alleles=5, seed=4, depth_per_guide=30.0)

# name: (kind, generator arguments, model arguments, kernel, environment, library variant)
CASES = {
    "variant_130x2": ("variant", dict(VARIANT), {}, "k_guide_wave2", {}, None),
    "variant_65x1": ("variant", dict(n_guides=65, n_reps=1, guides_per_target=3, seed=32, depth_per_guide=2000.0), {},
                     "k_guide_wave2", {}, None),
    "variant_257x3_long_targets": ("variant", dict(n_guides=257, n_reps=3, guides_per_target=100, seed=33), {},
                                   "k_guide_wave2", {}, None),
    "variant_130x2_acc": ("variant", dict(n_guides=130, n_reps=2, guides_per_target=3, seed=31, with_accessibility=True),
                          ACC, "k_guide_wave2", {}, None),
    "tiling_130x2_a5": ("tiling", dict(TILING_A5), {}, "k_guide_tiling_rep", {}, None),
    "tiling_130x2_a13": ("tiling", dict(n_guides=130, n_reps=2, n_max_alleles=13, seed=4), {}, "k_guide_tiling_rep", {},
                         None),
    "tiling_70x2_a24": ("tiling", dict(n_guides=70, n_reps=2, n_max_alleles=24, seed=14), {}, "k_guide_tiling_rep", {},
                        None),
    "tiling_70x2_a48": ("tiling", dict(n_guides=70, n_reps=2, n_max_alleles=48, seed=14), {}, "k_guide_tiling_wide", {},
                        None),
    "tiling_130x2_a5_wave": ("tiling", dict(TILING_A5), {}, "k_guide_tiling_wave",
                             {"BEAN_HIP_TILING": "wave"}, None),
    "survival_130x2": ("survival", dict(n_guides=130, n_reps=2, seed=4), {}, "k_guide_survival_wave", {}, None),
    "survival_130x2_acc": ("survival", dict(n_guides=130, n_reps=2, seed=4, with_accessibility=True), ACC,
                           "k_guide_survival_wave", {}, None),
    "survival_tiling_70x2": ("survival_tiling",
                             dict(n_guides=70, n_reps=2, n_max_alleles=5, seed=5, depth_per_guide=30.0), {},
                             "k_guide_tiling_rep", {}, None),
    # the generic kernels of the A/B library (dirichlet_grad_one, digammas evaluated in place)
    "variant_130x2_wave1": ("variant", dict(VARIANT), {}, "k_guide_wave", {"BEAN_HIP_GUIDE": "wave1"}, "ab"),
    "variant_130x2_split": ("variant", dict(VARIANT), {}, "k_lik", {"BEAN_HIP_GUIDE": "split"}, "ab"),
    "survival_130x2_block": ("survival", dict(n_guides=130, n_reps=2, seed=4), {}, "k_guide_survival",
                             {"BEAN_HIP_SURVIVAL": "block"}, "ab"),
    "tiling_130x2_a5_block": ("tiling", dict(TILING_A5), {}, "k_guide_tiling",
                              {"BEAN_HIP_TILING": "block"}, "ab"),
}
SWITCHES = ("BEAN_HIP_GUIDE", "BEAN_HIP_SURVIVAL", "BEAN_HIP_TILING", "BEAN_HIP_STEP")


@pytest.fixture(scope="module")
def engine():
    from bean_amd import engine as eng

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return eng


def point_parameters(kind, data, start, point, seed=7):
    """The unconstrained parameters of an evaluation point from the engine's start values, formed on the host:
    every tensor + 0.3 randn (masked alleles keep their fixed storage); "fitted": alpha_pi replaced by
    ``grad_bounds.fitted_like_alpha_pi``; "effect": the Normal side replaced too, ``effect_regimes.effect_point``."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in start.items():
        v = v.detach().cpu().float()
        noise = 0.3 * torch.randn(v.shape, generator=g)
        if k == "alpha_pi" and kind.endswith("tiling"):
            noise = noise * data.allele_mask
        out[k] = v + noise
    if point == "fitted":
        out["alpha_pi"] = gb.fitted_like_alpha_pi(data, out["alpha_pi"], seed=seed)
    if point == "effect":
        out = er.effect_point(kind, data, out, seed=seed)
    return out


def check_elementwise(name, point, grads, ref, tol, tol_tail):
    """|g_k - ref_k| <= tol_k for every element; the worst ratio and its index are printed per tensor."""
    bad = []
    for k, g in grads.items():
        got = g.detach().cpu().double().numpy().reshape(ref[k].shape)
        err = np.abs(got - ref[k])
        assert np.isfinite(got).all() and np.isfinite(ref[k]).all(), (name, point, k)
        ratio = np.where(tol[k] > 0, err / np.where(tol[k] > 0, tol[k], 1.0), np.where(err > 0, np.inf, 0.0))
        worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
        over = err > tol[k]
        n_tail = int(over.sum())
        beyond = int((err > tol_tail[k]).sum())
        print(f"ELEMENTWISE {name} {point} {k}: worst err/tol {float(ratio[worst]):.3f} at {tuple(int(i) for i in worst)} "
              f"(ref {float(ref[k][worst]):.6e}, got {float(got[worst]):.6e}); {n_tail} of {err.size} elements on the "
              f"1e-6 pathwise constant, {beyond} beyond it")
        if beyond or n_tail > gb.MAX_TAIL_SHARE * err.size:
            bad.append((k, float(ratio[worst]), worst, n_tail, beyond))
    assert not bad, (name, point, bad)


def run_case(engine, monkeypatch, name, point):
    kind, gen_kw, kw, kernel, env, variant = CASES[name]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    evaluate(engine, name, point, kind, MAKERS[kind](**gen_kw), kw, kernel, variant)


def evaluate(engine, name, point, kind, data, kw, kernel, variant=None, family=None, loss_fn=None, oracle_params=None,
             inject=None, **bounds_kw):
    """One evaluation of the screen `data` at `point` against the oracle: the kernel (where one is named), the loss to
    1e-9, every gradient element within its tolerance.  `family` / `loss_fn` default to the mixture family of `kind`;
    `bounds_kw` goes to grad_bounds.elementwise_bounds (another implicit gradient for the oracle, a per-evaluation
    allowance in place of the pathwise constants: then no element has a tail constant, and one beyond `tol` fails);
    `oracle_params` maps the point's float32 parameters to the ones the oracle is evaluated at; `inject(engine)` returns
    draws to hand in (`set_noise`) in place of the engine's own - the branches of the implicit gradient are then whatever
    those draws give and are not asserted.  At the "effect" point the census of the dumped draws is printed
    (effect_regimes.floor_census) and returned."""
    family, loss_fn = family or FAMILY[kind], loss_fn or LOSS[kind]
    extra = dict(lib_variant=variant) if variant else {}
    eng = engine.HipSVI(family, data.to(DEV), dump_noise=True, num_steps=50, **kw, **extra)
    if kernel is not None:
        assert eng.dominant_kernel == kernel, (name, eng.dominant_kernel)
    params = point_parameters(kind, data, eng.unconstrained, point)
    for k, v in eng.unconstrained.items():
        v.copy_(params[k].to(DEV))
    if inject is not None:
        eng.set_noise(inject(eng))
    loss, grads = eng.elbo_grad(step=2, seed=7)
    draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    eng.close()
    assert np.isfinite(loss)
    at = params if oracle_params is None else oracle_params(params)
    census = None
    if point == "effect":
        census = er.floor_census(data, at, draws, kw, loss_fn)
        print(f"CENSUS {name} {point}: {er.census_line(census)}")
    ref_loss, ref, tol, tol_tail = gb.elementwise_bounds(loss_fn, elbo.as_float64(data), at, draws, kw, **bounds_kw)
    print(f"LOSS {name} {point}: |loss - ref| / |ref| {abs(loss - ref_loss) / abs(ref_loss):.3e}")
    assert abs(loss - ref_loss) <= 1e-9 * abs(ref_loss), (name, point, loss, ref_loss)
    if "alpha_pi" not in params:  # the Normal family: no Dirichlet site in the guide, no implicit gradient
        check_elementwise(name, point, grads, ref, tol, tol_tail)
        return census
    if kind.endswith("tiling"):
        # the gradient of a masked allele's alpha is exactly zero (in-place write at model.py:645)
        assert torch.all(grads["alpha_pi"][~data.allele_mask.to(DEV)] == 0), (name, point)
    counts = gb.branch_counts(data, params["alpha_pi"], draws["pi"], survival=kind.startswith("survival"))
    print(f"BRANCHES {name} {point}: " + ", ".join(f"{b} {int(n)}" for b, n in zip(gb.BRANCHES, counts)) +
          f" of {int(counts.sum())}")
    if point in ("fitted", "effect") and inject is None:
        if kind == "variant":
            assert counts.min() >= 0.1 * counts.sum(), (name, counts)
        else:
            assert counts.min() >= 1, (name, counts)
    check_elementwise(name, point, grads, ref, tol, tol_tail)
    return census


PRODUCT = [n for n, c in CASES.items() if c[5] is None]
GENERIC = [n for n, c in CASES.items() if c[5] is not None]


@pytest.mark.parametrize("point", ["perturbed", "fitted"])
@pytest.mark.parametrize("name", PRODUCT)
def test_every_gradient_element_matches_the_oracle(engine, monkeypatch, name, point):
    run_case(engine, monkeypatch, name, point)


@pytest.mark.parametrize("point", ["perturbed", "fitted"])
@pytest.mark.parametrize("name", GENERIC)
def test_every_gradient_element_of_the_generic_kernels_matches_the_oracle(engine, monkeypatch, name, point):
    run_case(engine, monkeypatch, name, point)


def test_the_cases_reach_every_precomputed_digamma_call_site():
    """dirichlet_grad_one_pre is called from k_guide_wave2 (bean_guide_v2.hpp), k_guide_survival_wave
    (bean_survival_v2.hpp), k_guide_tiling_rep (bean_tiling_v2.hpp), k_guide_tiling_wide (bean_tiling_wide.hpp) and
    k_guide_tiling_wave (bean_kernels.hpp); run_case asserts the kernel of each case."""
    assert {c[3] for c in CASES.values()} >= {"k_guide_wave2", "k_guide_survival_wave", "k_guide_tiling_rep",
                                              "k_guide_tiling_wide", "k_guide_tiling_wave"}


def test_precomputed_digamma_form_is_bitwise_the_plain_function(engine):
    """dirichlet_grad_one_pre handed the device's own digamma(alpha), digamma(total) (op 10) returns what
    dirichlet_grad_one evaluates (op 2), bit for bit, over the inputs of test_dirichlet_grad_matches_torch: the kernels
    that read the digammas from k_param's tables compute the same implicit gradient as those that do not."""
    rng = np.random.default_rng(2)
    n = 200_000
    al = np.exp(rng.uniform(np.log(1e-3), np.log(2e3), n))
    be = np.exp(rng.uniform(np.log(1e-3), np.log(2e3), n))
    x = rng.beta(al, be).clip(1e-12, 1 - 1e-12)
    plain, _ = engine.test_special(2, al, x, al + be)
    pre, _ = engine.test_special(10, al, x, al + be)
    counts = np.bincount(gb.dirichlet_grad_branch(x, al, al + be), minlength=4)
    assert counts.min() > 1000, counts  # every branch is in the inputs
    assert torch.equal(plain.view(torch.int64), pre.view(torch.int64))
