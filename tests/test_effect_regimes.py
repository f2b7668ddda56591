"""tests/effect_regimes.py on the host: the effect-size point reaches concentrations floored by a bin's probability in waves
that mix floored and unfloored lanes, bin probabilities of exactly 0, and stays a relative 1e-6 or more away from the
floor's threshold in every case; the float64 oracle is a fit reference there (its own rounding noise is below a
thousandth of the per-element tolerance, its concentrations are within the float64 budget of a 50-digit evaluation); and
three mistakes planted in a copy of the oracle's concentration and gradient path each fail the per-element tolerance
there - the first of them passes it at the usual point, which is why the suite could not see it."""
import math

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
import count_regimes as cr
import effect_regimes as er
import grad_bounds as gb
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                              make_survival_tiling_screen, make_survival_variant_screen)
from oracle import elbo
from oracle import survival as osurv

MAKERS = {"variant": make_sorting_variant_screen, "tiling": make_sorting_tiling_screen,
          "survival": make_survival_variant_screen, "survival_tiling": make_survival_tiling_screen}


def host_case(name, point="effect", mu_max=None, small_a0=True):
    """(data, family, kw, params, noise) of a case of effect_regimes.CASES with torch's draws."""
    kind, gen_kw, kw, family, near_one, _ = er.CASES[name]
    data = MAKERS[kind](**gen_kw)
    if small_a0:
        data = er.with_small_a0(data)
    mod = osurv if kind.startswith("survival") else elbo
    start = mod.init_params(family, data, scale_by_acc=bool(kw.get("scale_by_accessibility")))
    g = torch.Generator().manual_seed(7)
    params = {}
    for k, v in start.items():
        noise = 0.3 * torch.randn(v.shape, generator=g)
        if k == "alpha_pi" and kind.endswith("tiling"):
            noise = noise * data.allele_mask
        params[k] = (v.detach() + noise).float()
    if point == "effect":
        params = er.effect_point(kind, data, params, seed=7, mu_max=mu_max)
    draws = cr.host_noise(kind, data, params, kw)
    if near_one:
        draws["pi"] = er.near_one_pi(tuple(draws["pi"].shape), seed=er.PI_SEED)
    return data, family, kw, params, draws


@pytest.fixture(scope="module")
def normal_case():
    data, family, kw, params, noise = host_case("variant_130x2")
    d64 = elbo.as_float64(data)
    loss, ref, tol, tol_tail = gb.elementwise_bounds(elbo.normal_loss, d64, params, noise, kw)
    return dict(data=data, d64=d64, params=params, noise=noise, kw=kw, loss=loss, ref=ref, tol=tol, tol_tail=tol_tail)


def test_with_small_a0_changes_the_two_precisions_only():
    data = make_sorting_variant_screen(**er.VARIANT)
    small = er.with_small_a0(data)
    assert float(data.a0.min()) >= 11.0 and float(data.a0_bcmatch.min()) >= 5.1  # no floor by probability as generated
    for k, v in vars(data).items():
        if k in ("a0", "a0_bcmatch"):
            got = getattr(small, k)
            assert got.dtype == v.dtype and got.shape == v.shape
            assert got[:8].tolist() == list(er.A0_PATTERN) and got[8:16].tolist() == list(er.A0_PATTERN)
        else:
            assert getattr(small, k) is v, k


def test_the_effect_point_is_float32_and_what_the_module_says():
    data = er.with_small_a0(make_sorting_variant_screen(**er.VARIANT))
    start = elbo.init_params("MixtureNormal", data)
    p = er.effect_point("variant", data, start, seed=7)
    assert set(p) == set(start) and all(v.dtype == torch.float32 and v.shape == start[k].shape for k, v in p.items())
    T = data.n_targets
    assert p["mu_loc"].reshape(-1).tolist() == [float(np.float32(er.MU[t % 11])) for t in range(T)]
    assert torch.equal(p["sd_loc"].reshape(-1), torch.tensor([er.SD[t % 5] for t in range(T)], dtype=torch.float64).float().log())
    for k in ("mu_scale", "sd_scale"):
        assert set(p[k].reshape(-1).tolist()) == set(er.LOG_SCALES)
    assert torch.equal(p["alpha_pi"], gb.fitted_like_alpha_pi(data, start["alpha_pi"], seed=7))
    s = er.effect_point("survival", data, {"mu_loc": torch.zeros(T, 1), "mu_scale": torch.zeros(T, 1)})
    assert float(s["mu_loc"].max()) == er.SURVIVAL_MU_MAX == -float(s["mu_loc"].min())


def test_near_one_pi_puts_a_third_of_the_pairs_next_to_one():
    pi = er.near_one_pi((2, 1, 130, 2), seed=er.PI_SEED)
    assert pi.dtype == torch.float64 and pi.shape == (2, 1, 130, 2)
    assert float((pi.sum(-1) - 1).abs().max()) <= 2.0 ** -52 and float(pi.min()) >= 1e-12
    p0 = pi[..., 0].reshape(-1)
    small = p0 <= 1e-6
    assert int(small.sum()) == math.ceil(260 / 3) and bool(small[::3].all())
    assert float(p0[~small].min()) >= 0.05 and float(p0[~small].max()) <= 0.95
    assert float(p0[small].max() / p0[small].min()) > 1e4   # spread over the decades, not one value


@pytest.mark.parametrize("name", list(er.CASES))
def test_the_point_reaches_the_regime_and_keeps_its_distance_from_the_threshold(name):
    data, family, kw, params, noise = host_case(name)
    c = er.floor_census(data, params, noise, kw, family)
    print(f"CENSUS {name} {family}: {er.census_line(c)}")
    assert c["nearest"] >= 1e-6, (name, c["nearest"])   # the device and the oracle take the same side at every bin
    if er.CASES[name][5]:
        er.assert_reaches_the_regime(c, name)
    if name == "variant_130x2":   # measured: 90 of 260 pairs, 16 / 27 / 2 floored lanes in the waves of a replicate, 120 zeros
        assert c["mixed_waves"][0] >= 4 and c["p_zero"] > 50


@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
def test_the_steppers_screen_at_the_effect_point(family):
    """The 65-target screen the stepper tests of test_gpu_effect_regimes.py run on: the `Normal` family reaches the
    regime; the mixture, whose steppers draw their own pi, reaches probabilities of exactly 0 and 1 and almost no floor."""
    data = er.with_small_a0(make_sorting_variant_screen(**er.STEPPER_SCREEN))
    assert data.n_targets == 65
    params = er.effect_point("variant", data, elbo.init_params(family, data))
    c = er.floor_census(data, params, cr.host_noise("variant", data, params), {}, family)
    print(f"CENSUS steppers {family}: {er.census_line(c)}")
    assert c["nearest"] >= 1e-6 and c["p_zero"] > 0 and c["p_one"] > 0
    if family == "Normal":
        er.assert_reaches_the_regime(c, "steppers")
    else:
        assert c["floored_pairs"][0] < 0.1 * c["kept_pairs"][0]


def test_the_usual_point_reaches_none_of_it():
    """The generated screen (a0 >= 11) has no bin floored by its probability, at `init + 0.3 randn` (where no probability
    is 0 either) as at the effect point; the small-a0 screen at `init + 0.3 randn` has a handful (6 of 1 300, where a
    draw of sd_t is small), the effect point 221: the regime needs the screen and the point."""
    data, family, kw, params, noise = host_case("variant_130x2", point="perturbed", small_a0=False)
    c = er.floor_census(data, params, noise, kw, family)
    assert c["floored_bins"] == [0, 0] and c["p_zero"] == 0
    data, family, kw, params, noise = host_case("variant_130x2", small_a0=False)
    c = er.floor_census(data, params, noise, kw, family)
    assert c["floored_bins"] == [0, 0] and c["p_zero"] > 0
    data, family, kw, params, noise = host_case("variant_130x2", point="perturbed")
    c = er.floor_census(data, params, noise, kw, family)
    assert c["floored_pairs"][0] < 0.05 * c["kept_pairs"][0]


def test_without_the_injected_pi_the_mixture_does_not_floor():
    """pi drawn from the guide's Dirichlet keeps the wild-type component's weight up: nothing floors, and the case
    needs `near_one_pi`."""
    data, family, kw, params, noise = host_case("variant_130x2_near_one_pi")
    noise = cr.host_noise("variant", data, params, kw)
    c = er.floor_census(data, params, noise, kw, family)
    assert c["floored_pairs"][0] < 0.1 * c["kept_pairs"][0]


# ---------------------------------------------------------------- the oracle is a fit reference here
def test_oracle_is_finite_and_its_tolerance_is_the_float32_term(normal_case):
    e = normal_case
    assert np.isfinite(e["loss"])
    for k, ref in e["ref"].items():
        assert np.isfinite(ref).all() and np.isfinite(e["tol"][k]).all() and (e["tol"][k] > 0).all(), k
        nz = ref != 0
        med = float(np.median(e["tol"][k][nz] / np.abs(ref[nz])))
        assert gb.ULP32 <= med <= 1.01 * gb.ULP32, (k, med)   # 1.19e-7 of the element: the float32 output term


@pytest.mark.parametrize("name", ["variant_130x2", "variant_130x2_near_one_pi"])
def test_bin_reversed_oracle_is_within_a_thousandth_of_the_tolerance_at_the_effect_point(name):
    data, family, kw, params, noise = host_case(name)
    d64 = elbo.as_float64(data)
    loss_fn = elbo.LOSSES[family]
    _, ref, tol, _ = gb.elementwise_bounds(loss_fn, d64, params, noise, kw)
    _, alt, _, _ = gb.elementwise_bounds(loss_fn, gb.reverse_bins(d64), params, noise, kw)
    for k in ref:
        assert np.all(tol[k] > 0), k
        ratio = float((np.abs(alt[k] - ref[k]) / tol[k]).max())
        print(f"NOISE {name} {k}: bin-reversed oracle worst err/tol {ratio:.2e}")
        assert ratio <= 1e-3, (name, k, ratio)


ALPHA_CASES = ["variant_130x2", "variant_130x2_near_one_pi", "variant_130x2_acc"]


@pytest.mark.parametrize("name", ALPHA_CASES)
def test_oracle_concentrations_are_within_the_float64_budget_of_exact_arithmetic(name):
    """torch's float64 evaluation against 50 digits, every element of both planes, in units of the budget: the multiple it
    needs is `effect_regimes.K_HOST` or less (the device is held to four times that), and floored elements are 1e-5."""
    data, family, kw, params, noise = host_case(name)
    pi = er.near_one_pi(tuple(noise["pi"].shape), seed=er.PI_SEED) if family == "MixtureNormal" else None
    acc = params.get("noise_loc")
    exact, budget, floored = er.exact_alpha(family, data, params, pi=pi, acc_noise=acc)
    got = er.oracle_alpha(family, data, params, pi=pi, acc_noise=acc, kw=kw)
    worst, on_floor = er.alpha_ratio(got, exact, budget, floored)
    print(f"ALPHA {name}: torch float64 worst |err| / budget {worst:.3f}; {int(floored.sum())} of {floored.size} floored")
    assert on_floor and worst <= er.K_HOST, (name, worst)
    assert np.array_equal(got == er.EPS, floored)
    if er.CASES[name][5]:
        on = data.sample_mask.cpu().numpy().astype(bool)   # (R, B): floors by probability, not by the sample mask
        assert floored[:, on].any()


# ---------------------------------------------------------------- the survival range
@pytest.mark.parametrize("name", ["survival_130x2", "survival_tiling_70x2"])
def test_survival_range_is_the_widest_rung_the_oracle_is_finite_at(name):
    data, family, kw, params, noise = host_case(name)
    loss, ref, tol, _ = gb.elementwise_bounds(osurv.LOSSES[family], elbo.as_float64(data), params, noise, kw)
    assert float(params["mu_loc"].abs().max()) == er.SURVIVAL_MU_MAX
    assert np.isfinite(loss)
    for k in ref:
        assert np.isfinite(ref[k]).all() and np.isfinite(tol[k]).all(), k
        assert not ((tol[k] == 0) & (ref[k] != 0)).any(), k


def test_the_next_rung_of_the_survival_range_is_not_finite():
    data, family, kw, params, noise = host_case("survival_tiling_70x2", mu_max=2 * er.SURVIVAL_MU_MAX)
    p = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        loss = osurv.multi_mixture_normal_loss(elbo.as_float64(data), p, noise=noise)
    assert not np.isfinite(float(loss))


# ---------------------------------------------------------------- the tests have teeth
def clamp_as_identity(orig):
    """(a) the floor differentiated as the identity: a floored bin's gradient is left in."""
    def f(egp, size_factor, sample_mask, a0, eps=er.EPS):
        p = egp.permute(0, 2, 1) * size_factor[:, None, :]
        a = (p + eps / p.shape[-1]) / (p.sum(-1)[:, :, None] + eps) * a0[None, :, None] * sample_mask[:, None, :]
        return a + (a.clamp(min=eps) - a).detach()
    return f


class total_term_as_data:
    """(b) the total term taken as lgamma(a0 + n) - lgamma(a0) for the pairs that hold a floored bin: the constant of
    DevArgs::tot_const without its correction."""

    def __init__(self):
        self.a0 = None

    def concentration(self, orig):
        def f(egp, size_factor, sample_mask, a0, eps=er.EPS):
            self.a0 = a0
            return orig(egp, size_factor, sample_mask, a0, eps)
        return f

    def log_prob(self, orig):
        def f(conc, value):
            def log_beta_1(a, x):
                return torch.lgamma(1 + x) + torch.lgamma(a) - torch.lgamma(x + a)

            floored = (conc == er.EPS).any(-1)
            total = torch.where(floored, self.a0[None, :].expand_as(floored).to(conc.dtype), conc.sum(-1))
            return log_beta_1(total, value.sum(-1)) - log_beta_1(conc, value).sum(-1)
        return f


def pdf_cut_beyond_six(orig):
    """(c) the density, which is the derivative of the bin probability, cut to 0 beyond |u| = 6; the values are the
    oracle's (Normal.cdf is 0.5 (1 + erf((z - mu) / sd / sqrt 2)))."""
    def f(uq, lq, mu, sd, mask=None):
        assert mask is None
        top, bottom = uq == 1.0, lq == 0.0
        std = torch.distributions.Normal(0.0, 1.0)
        half = torch.full_like(uq, 0.5)

        def cdf(z):
            u = (z - mu) * sd.reciprocal()
            u = torch.where(u.abs() <= 6.0, u, u.detach())
            return 0.5 * (1 + torch.erf(u / math.sqrt(2)))

        c_hi = torch.where(top, torch.ones_like(uq), cdf(std.icdf(torch.where(top, half, uq))))
        c_lo = torch.where(bottom, torch.zeros_like(lq), cdf(std.icdf(torch.where(bottom, half, lq))))
        return c_hi - c_lo
    return f


def _planted(mistake, case_data):
    d64, params, noise, kw = (case_data[k] for k in ("d64", "params", "noise", "kw"))
    if mistake == "a":
        ctx = [gb._Patched("dirmult_concentration", clamp_as_identity)]
    elif mistake == "b":
        t = total_term_as_data()
        ctx = [gb._Patched("dirmult_concentration", t.concentration),
               gb._Patched("dirichlet_multinomial_log_prob", t.log_prob)]
    else:
        ctx = [gb._Patched("std_normal_bin_prob", pdf_cut_beyond_six)]
    p = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    for c in ctx:
        c.__enter__()
    try:
        loss = elbo.normal_loss(d64, p, noise=noise, **kw)
    finally:
        for c in reversed(ctx):
            c.__exit__(None, None, None)
    grads = torch.autograd.grad(loss, list(p.values()))
    return float(loss.detach()), {k: g.numpy() for k, g in zip(p, grads)}


def _worst(grads, case_data):
    return {k: float((np.abs(g - case_data["ref"][k]) / case_data["tol_tail"][k]).max()) for k, g in grads.items()}


@pytest.mark.parametrize("mistake", ["a", "b", "c"])
def test_planted_mistakes_fail_the_tolerance_at_the_effect_point(normal_case, mistake):
    loss, grads = _planted(mistake, normal_case)
    worst = _worst(grads, normal_case)
    print(f"PLANTED ({mistake}) effect point: loss off by {abs(loss - normal_case['loss']) / abs(normal_case['loss']):.2e}, "
          f"worst err/tol " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) > 1.0, (mistake, worst)
    if mistake == "b":   # the value is wrong too, beyond the loss tolerance of 1e-9
        assert abs(loss - normal_case["loss"]) > 1e-9 * abs(normal_case["loss"])
    else:                # a mistake in the derivative alone: the copy's values are the oracle's
        assert abs(loss - normal_case["loss"]) <= 1e-13 * abs(normal_case["loss"])


def test_the_floor_differentiated_as_identity_passes_at_the_usual_point():
    """Masked samples are the only floors there and their gradient is zero on either reading: mistake (a) is invisible
    at `init + 0.3 randn` on the screen as generated, where the suite evaluated the kernels so far."""
    data, family, kw, params, noise = host_case("variant_130x2", point="perturbed", small_a0=False)
    d64 = elbo.as_float64(data)
    loss, ref, tol, tol_tail = gb.elementwise_bounds(elbo.normal_loss, d64, params, noise, kw)
    case_data = dict(d64=d64, params=params, noise=noise, kw=kw, ref=ref, tol_tail=tol_tail)
    got_loss, grads = _planted("a", case_data)
    assert abs(got_loss - loss) <= 1e-9 * abs(loss)
    assert max(_worst(grads, case_data).values()) <= 1.0
