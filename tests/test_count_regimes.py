"""tests/count_regimes.py on the host: the planes have the properties their regime states and leave alone what a depth
study conditions on; at every regime and screen kind the float64 oracle and the per-element tolerance of grad_bounds.py
are finite, far above the oracle's own rounding noise and not vacuous; and at the 2^24 - 1 cap the oracle's count
likelihood is within a ten-billionth of the loss, pair by pair, of a 40-digit evaluation - which is what lets the device
tests keep ``1e-9 |ref_loss|`` there."""
import mpmath
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
import count_regimes as cr
import dirichlet_grad_reference as dgr
import grad_bounds as gb
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                              make_survival_tiling_screen, make_survival_variant_screen)
from oracle import elbo
from oracle import survival as osurv

# the smallest shapes of test_gpu_grad_elementwise.py, one per screen kind
KINDS = {
    "variant": (make_sorting_variant_screen, dict(n_guides=130, n_reps=2, guides_per_target=3, seed=31),
                "MixtureNormal", elbo),
    "tiling": (make_sorting_tiling_screen, dict(n_guides=130, n_reps=2, n_max_alleles=5, seed=4, depth_per_guide=30.0),
               "MultiMixtureNormal", elbo),
    "survival": (make_survival_variant_screen, dict(n_guides=130, n_reps=2, seed=4), "MixtureNormal", osurv),
    "survival_tiling": (make_survival_tiling_screen,
                        dict(n_guides=70, n_reps=2, n_max_alleles=5, seed=5, depth_per_guide=30.0),
                        "MultiMixtureNormal", osurv),
}
LOSS = {"variant": elbo.mixture_normal_loss, "tiling": elbo.multi_mixture_normal_loss,
        "survival": osurv.mixture_normal_loss, "survival_tiling": osurv.multi_mixture_normal_loss}
ALL_REGIMES = cr.REGIMES + ("generated_deep",)
CONDITIONED = ("size_factor", "size_factor_bcmatch", "a0", "a0_bcmatch", "pi_a0", "allele_counts_control", "sample_mask",
               "repguide_mask", "upper_bounds", "lower_bounds", "allele_mask", "a2e_ptr", "a2e_idx", "target_lengths",
               "timepoints", "control_timepoint", "guide_accessibility", "X_control", "X_bcmatch_control")


@pytest.fixture(scope="module")
def base():
    return {kind: maker(**gen_kw) for kind, (maker, gen_kw, _, _) in KINDS.items()}


def _screen(base, kind, regime):
    maker, gen_kw, _, _ = KINDS[kind]
    return cr.generated_deep(maker, **gen_kw) if regime == "generated_deep" else cr.rewrite_counts(base[kind], regime)


def _kept(data, plane="X_masked"):
    n = torch.as_tensor(cr.pair_totals(getattr(data, plane)))
    return (n > cr.MASK_THRES) & data.repguide_mask


# ---------------------------------------------------------------- the planes
@pytest.mark.parametrize("regime", cr.REGIMES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_rewrite_touches_the_counts_alone(base, kind, regime):
    data = base[kind]
    before = {k: v.clone() for k, v in vars(data).items() if isinstance(v, torch.Tensor)}
    out = cr.rewrite_counts(data, regime)
    for k, v in before.items():  # the screen handed in is as it was
        assert torch.equal(getattr(data, k), v), k
    for k in CONDITIONED:
        assert getattr(out, k, None) is getattr(data, k, None), k
    sm = data.sample_mask[:, :, None].float()
    for k in cr.COUNT_PLANES:
        x = getattr(out, k)
        assert x.dtype == torch.float32 and x.shape == getattr(data, k).shape, k
        assert bool((x >= 0).all()) and torch.equal(x, x.round()), k
        assert float(cr.pair_totals(x).max()) <= cr.CAP, k
    assert torch.equal(out.X_bcmatch, torch.floor(0.8 * out.X.double() + 0.5).float())
    assert torch.equal(out.X_masked, out.X * sm) and torch.equal(out.X_bcmatch_masked, out.X_bcmatch * sm)
    assert not torch.equal(out.X, data.X)


@pytest.mark.parametrize("kind", list(KINDS))
def test_deep_puts_the_largest_pair_on_the_cap(base, kind):
    data, out = base[kind], cr.rewrite_counts(base[kind], "deep")
    n_old, n_new = cr.pair_totals(data.X), cr.pair_totals(out.X)
    assert float(n_new.max()) == cr.CAP and int(np.argmax(n_new)) == int(np.argmax(n_old))
    f = cr.CAP / n_old.max()
    assert np.abs(out.X.double().numpy() - np.floor(f * data.X.double().numpy() + 0.5)).max() <= data.n_condits
    assert float(np.median(n_new)) > 1e6  # the whole screen is deep, not one pair


@pytest.mark.parametrize("kind", list(KINDS))
def test_shallow_stays_in_the_product_form_on_both_sides_of_the_mask_threshold(base, kind):
    out = cr.rewrite_counts(base[kind], "shallow")
    n = cr.pair_totals(out.X)
    assert 12.0 <= float(np.median(n)) <= 12.5
    small = float((out.X <= 12).double().mean())
    kept = float((n > cr.MASK_THRES).mean())
    print(f"shallow {kind}: bins <= 12 {small:.3f}, pairs kept by the > 10 rule {kept:.3f}")
    assert small >= 0.97 and 0.4 <= kept <= 0.8
    assert bool(((out.X == 0).any(1) & base[kind].repguide_mask).any())  # zero bins inside pairs the mask keeps


@pytest.mark.parametrize("kind", list(KINDS))
def test_mixed_interleaves_deep_and_shallow_guides(base, kind):
    data = base[kind]
    out, deep, shallow = (cr.rewrite_counts(data, r) for r in ("mixed", "deep", "shallow"))
    B = data.n_condits
    g = torch.arange(data.n_guides)
    odd = (g >= 64) & (g % 2 == 1)
    assert data.n_guides > 65 and bool(odd.any())
    lifted = deep.X < 13  # (bins the screen has at 0)
    assert torch.equal(out.X[:, :, odd], shallow.X[:, :, odd]) and float(lifted.double().mean()) < 0.05
    want = torch.where(lifted, torch.full_like(deep.X, 13), deep.X)  # (cut back to the cap in one bin at the most)
    assert bool((out.X[:, :, ~odd] - want[:, :, ~odd]).abs().max() <= 13 * B)
    assert float(out.X[:, :, :64].min()) > 12  # the first wave: deep in every bin
    assert float(out.X[:, :, odd].max()) < 100 < float(out.X[:, :, ~odd].median())


@pytest.mark.parametrize("kind", list(KINDS))
def test_edges_plants_the_branch_edges(base, kind):
    data, out = base[kind], cr.rewrite_counts(base[kind], "edges")
    B, G = data.n_condits, data.n_guides
    kept, masked, one_bin = cr.edge_guides(data)
    assert len({kept, masked, one_bin}) == 3
    for g in range(G):
        if g not in (kept, masked, one_bin):
            assert bool((out.X[:, g % B, g] == cr.EDGE_VALUES[(g // B) % 4]).all()), g
    planted = {float(v) for g in range(G) if g not in (kept, masked, one_bin) for v in out.X[:, g % B, g]}
    assert planted == set(cr.EDGE_VALUES)
    n, n_bc = cr.pair_totals(out.X), cr.pair_totals(out.X_bcmatch)
    assert bool((n[:, kept] == 11).all()) and bool((n[:, masked] == 10).all()) and bool((n[:, one_bin] == cr.CAP).all())
    assert bool((out.X[:, 0, one_bin] == cr.CAP).all()) and float(out.X[:, 1:, one_bin].abs().sum()) == 0
    assert bool((n_bc[:, one_bin] == np.floor(0.8 * cr.CAP + 0.5)).all())
    keep = _kept(out)
    assert bool(keep[:, kept].all()) and not bool(keep[:, masked].any()) and bool(keep[:, one_bin].all())
    assert bool(((out.X == 0).any(1) & data.repguide_mask).any())


@pytest.mark.parametrize("kind", list(KINDS))
def test_generated_deep_has_both_arguments_large(kind):
    maker, gen_kw, _, _ = KINDS[kind]
    data = cr.generated_deep(maker, **gen_kw)
    n = cr.pair_totals(data.X)
    print(f"generated-deep {kind}: pair totals {n.min():.3g} ... {n.max():.3g}, a0 {float(data.a0.min()):.3g} ... "
          f"{float(data.a0.max()):.3g}, pi_a0 <= {float(data.pi_a0.max()):.3g}")
    assert float(np.median(n)) > 5e5 and float(n.max()) <= cr.CAP
    assert float(data.a0.median()) > 1e4 and float(data.pi_a0.max()) <= cr.PI_A0_MAX
    assert torch.equal(data.X, data.X.round())


# ---------------------------------------------------------------- the oracle and its tolerance on these planes
def _evaluation(base, kind, regime, **bounds_kw):
    _, _, family, mod = KINDS[kind]
    data = cr.regime_screen(*KINDS[kind][:2], regime) if regime == "generated_deep_unclamped" else _screen(base, kind, regime)
    g = torch.Generator().manual_seed(7)
    params = {k: (v.detach() + 0.3 * torch.randn(v.shape, generator=g)).float()
              for k, v in mod.init_params(family, data).items()}
    if kind.endswith("tiling"):  # masked alleles keep their fixed storage
        start = mod.init_params(family, data)["alpha_pi"].detach()
        params["alpha_pi"] = torch.where(data.allele_mask, params["alpha_pi"], start)
    noise = cr.host_noise(kind, data, params)
    d64 = elbo.as_float64(data)
    return d64, params, noise, gb.elementwise_bounds(LOSS[kind], d64, params, noise, {}, **bounds_kw)


@pytest.mark.parametrize("kind", ["variant", "tiling", "survival"])
def test_the_unclamped_screen_is_held_by_each_evaluations_own_budget(base, kind):
    """generated_deep_unclamped: pi_a0 as generated, at least a quarter of the implicit-gradient evaluations with a
    concentration above 2e3; with port64 as the oracle's implicit gradient and the per-evaluation allowance, tol and
    tol_tail are one finite array, the oracle with torch's implicit gradient lies within it (torch is within K of the
    same budget, K below the device's), and the typical element is still held to better than 1e-5 of itself."""
    k_dev, seen = dgr.device_k(), []
    d64, params, noise, (loss, ref, tol, tol_tail) = _evaluation(
        base, kind, "generated_deep_unclamped", dirichlet_grad=dgr.port64_torch, path_allowance=dgr.path_allowance(k_dev, seen))
    assert float(d64.pi_a0.max()) > cr.PI_A0_MAX
    al, tot = (np.concatenate([s[i] for s in seen]) for i in (1, 2))
    high = np.maximum(al, tot - al) > cr.PI_A0_MAX
    print(f"UNCLAMPED {kind}: pi_a0 {float(d64.pi_a0.min()):.3g} ... {float(d64.pi_a0.max()):.3g}, {int(high.sum())} of "
          f"{high.size} evaluations above 2e3")
    assert high.mean() >= 0.25
    loss_t, ref_t, _, _ = gb.elementwise_bounds(LOSS[kind], d64, params, noise, {})
    assert loss_t == loss
    for k, r in ref.items():
        assert np.isfinite(r).all() and np.isfinite(tol[k]).all() and np.array_equal(tol[k], tol_tail[k]), k
        assert np.all(np.abs(ref_t[k] - r) <= tol[k]), k
        live = r != 0
        assert float(np.median(tol[k][live] / np.abs(r[live]))) < 1e-5, k


@pytest.mark.parametrize("kind", ["variant", "tiling", "survival"])
def test_a_float32_exponential_of_the_concentrations_parameters_moves_tiling_alpha_pi_alone(base, kind):
    """The kernels take `alpha = (double)expf(alpha_pi)` (and q0 likewise) in float32, as the reference's float32
    parameters do; the float64 oracle takes the exponential in float64.  On the unclamped screen, with the
    per-evaluation allowance, the oracle at float32-exponentiated parameters stays within `tol_k` of itself in the variant
    and survival cases (2 alleles: the gradient is one product, moved by 2^-24 of itself) and leaves it in a few elements
    of tiling `alpha_pi` (5 alleles: `c_k (G_k - sum_a w_a G_a)` cancels) - which is why
    test_every_gradient_element_matches_the_oracle_above_2e3 (tests/test_gpu_count_regimes.py) evaluates the oracle at
    the kernels' constrained values.  No other tensor moves at all."""
    k_dev = dgr.device_k()
    bounds_kw = dict(dirichlet_grad=dgr.port64_torch, path_allowance=dgr.path_allowance(k_dev))
    d64, params, noise, (loss, ref, tol, _) = _evaluation(base, kind, "generated_deep_unclamped", **bounds_kw)
    as_kernels = {k: v.double() for k, v in params.items()}
    for k in ("alpha_pi", "q0"):
        if k in params:
            as_kernels[k] = params[k].float().exp().double().log()  # exp of it in float64 is the float32 exponential
    _, moved, _, _ = gb.elementwise_bounds(LOSS[kind], d64, as_kernels, noise, {}, dirichlet_grad=dgr.port64_torch)
    for k, r in ref.items():
        ratio = np.abs(moved[k] - r) / np.where(tol[k] > 0, tol[k], 1.0)
        print(f"FLOAT32 EXP {kind} {k}: worst |moved - ref| / tol {ratio.max():.3f}, {int((ratio > 1).sum())} of {ratio.size} beyond")
        if k not in ("alpha_pi", "q0"):
            assert ratio.max() < 1e-3, k
        elif kind == "tiling":
            assert 0 < (ratio > 1).sum() < 0.05 * ratio.size, k
        else:
            assert ratio.max() < 1.0, k


@pytest.mark.parametrize("regime", ALL_REGIMES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_oracle_and_its_tolerance_hold_on_the_plane(base, kind, regime):
    d64, params, noise, (loss, ref, tol, tol_tail) = _evaluation(base, kind, regime)
    assert np.isfinite(loss)
    _, alt, _, _ = gb.elementwise_bounds(LOSS[kind], _reversed(d64), params, noise, {})
    for k, r in ref.items():
        assert np.isfinite(r).all() and np.isfinite(tol[k]).all() and np.isfinite(tol_tail[k]).all(), k
        live = r != 0
        if kind.endswith("tiling") and k == "alpha_pi":
            assert not live[~d64.allele_mask.numpy()].any()  # a masked allele's gradient is exactly zero
        assert np.all(tol[k][live] > 0), k
        # the oracle's own rounding noise: the bin-reversed oracle, the rule of test_grad_bounds.py
        noise_ratio = np.abs(alt[k] - r)[live] / tol[k][live]
        assert np.all(np.abs(alt[k] - r) <= tol[k] / 1000.0), (k, float(noise_ratio.max()))
        # not vacuous: the typical element is held to better than 1e-5 of itself ...
        rel = tol[k][live] / np.abs(r[live])
        assert float(np.median(rel)) < 1e-5, (k, float(np.median(rel)))
        # ... and 1e-5 of an element of median size fails the bound, on either pathwise constant
        flat = np.abs(r).reshape(-1)
        idx = np.nonzero(flat)[0]
        i = int(idx[np.argsort(flat[idx])[idx.size // 2]])
        assert 1e-5 * flat[i] > tol_tail[k].reshape(-1)[i], (k, flat[i], tol_tail[k].reshape(-1)[i])
        print(f"ORACLE {kind} {regime} {k}: bin-reversed / tol {float(noise_ratio.max()):.2e}, "
              f"median tol / |ref| {float(np.median(rel)):.2e}")


def _reversed(d64):
    """gb.reverse_bins for every screen kind: the survival screens have timepoints in place of the quantile bounds, and
    their initial-abundance site reads condition 0 of ``X``, which must stay the first timepoint's."""
    import copy

    out = copy.copy(d64)
    B = d64.n_condits
    perm = torch.arange(B - 1, -1, -1)
    for k in ("X_masked", "X_bcmatch_masked", "size_factor", "size_factor_bcmatch", "sample_mask"):
        setattr(out, k, getattr(d64, k)[:, perm].contiguous())
    for k in ("upper_bounds", "lower_bounds", "timepoints"):
        if getattr(d64, k, None) is not None:
            setattr(out, k, getattr(d64, k)[perm].contiguous())
    return out


def test_reversing_the_bins_is_grad_bounds_own_on_a_sorting_screen(base):
    d64 = elbo.as_float64(base["variant"])
    a, b = gb.reverse_bins(d64), _reversed(d64)
    for k, v in vars(a).items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, getattr(b, k)), k


# ---------------------------------------------------------------- the oracle itself at the cap
def _mp_log_beta_1(a, x):
    return mpmath.loggamma(1 + x) + mpmath.loggamma(a) - mpmath.loggamma(x + a)


def test_the_oracle_count_likelihood_at_the_cap_against_forty_digits(base):
    """Per kept pair of the `deep` variant screen, oracle.elbo.dirichlet_multinomial_log_prob in float64 against the same
    formula at 40 digits on the same float64 concentrations: within 1e-10 |loss| / sqrt(n_pairs), so that the pairs'
    errors, added as independent roundings, stay two orders below the 1e-9 |ref_loss| the device is held to."""
    d64, params, noise, (loss, _, _, _) = _evaluation(base, "variant", "deep")
    seen = []
    orig = elbo.dirichlet_multinomial_log_prob

    def spy(conc, value):
        seen.append((conc.detach(), value.detach()))
        return orig(conc, value)

    with gb._Patched("dirichlet_multinomial_log_prob", lambda _orig: spy):
        elbo.mixture_normal_loss(d64, {k: v.double() for k, v in params.items()}, noise=noise)
    assert len(seen) == 2
    n_pairs = sum(int(_kept(d64, p).sum()) for p in ("X_masked", "X_bcmatch_masked"))
    assert n_pairs >= 500
    allowance = 1e-10 * abs(loss) / np.sqrt(n_pairs)
    mpmath.mp.dps = 40
    worst, largest, done = 0.0, 0.0, 0
    for (conc, val), plane in zip(seen, ("X_masked", "X_bcmatch_masked")):
        got = orig(conc, val)
        keep = _kept(d64, plane)
        assert float(val.sum(-1).max()) >= np.floor(0.8 * cr.CAP + 0.5) - d64.n_condits  # (0.8 X, rounded bin by bin)
        pairs = np.argwhere(keep.numpy())
        order = np.argsort(-val.sum(-1).numpy()[keep.numpy()])  # the deepest pairs first
        for r, g in pairs[order[:30]]:
            a = [mpmath.mpf(float(v)) for v in conc[r, g]]
            x = [mpmath.mpf(float(v)) for v in val[r, g]]
            want = _mp_log_beta_1(mpmath.fsum(a), mpmath.fsum(x)) - mpmath.fsum(_mp_log_beta_1(ai, xi)
                                                                              for ai, xi in zip(a, x))
            worst = max(worst, abs(float(mpmath.mpf(float(got[r, g])) - want)))
            largest = max(largest, abs(float(want)))
            done += 1
    print(f"ORACLE AT THE CAP: {done} pairs, worst |float64 - 40 digits| {worst:.3e} (allowance {allowance:.3e}), "
          f"largest |log p| {largest:.1f}, loss {loss:.6e}")
    assert done == 60 and worst <= allowance
