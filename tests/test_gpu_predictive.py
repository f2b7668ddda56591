"""Posterior predictive check on the GPU: the count simulator (bean_hip_simulate, csrc/bean_predictive.hpp), its
concentrations against the oracle's get_alpha, its draws against the closed-form Dirichlet-Multinomial moments, the
state it must leave alone, its refusals, and the check end to end.  -m gpu."""
import copy
import ctypes
import os
from functools import partial

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.preprocessing.synthetic import (_dirmult_counts, make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

from dm_reference import flat_screen
from members_common import CONFIGS, DEV, VAR, _h5ad_reader_present, _kw_of, _mini, _run, _state  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = 101
BIG = 5003   # one pair's total inside a wave of totals near 500
G_BIG, G_ZERO, R_EDIT = 70, 75, 1  # both in the second tile of replicate 1


# ------------------------------------------------------------------ screens and engines, built once per module
def _edited(data):
    """The screen with one pair's counts set to zero and one pair's total raised to BIG (both likelihoods)."""
    out = copy.copy(data)
    for name in ("X_masked", "X_bcmatch_masked"):
        x = getattr(data, name).clone()
        x[R_EDIT, :, G_ZERO] = 0
        B = x.shape[1]
        x[R_EDIT, :, G_BIG] = torch.tensor([BIG // B + (1 if b < BIG % B else 0) for b in range(B)], dtype=x.dtype)
        setattr(out, name, x)
    return out


@pytest.fixture(scope="module")
def screens(tmp_path_factory):
    return {
        # (a fifth of the default depth: totals near 500, the deep pair of _edited is ten times its wave's)
        "203": _edited(make_sorting_variant_screen(203, 3, seed=11, mask_fraction=0.05, depth_per_guide=100.0)),
        "203acc": _edited(make_sorting_variant_screen(203, 3, seed=11, mask_fraction=0.05, depth_per_guide=100.0,
                                                      with_accessibility=True)),
        "mini": _mini(tmp_path_factory.mktemp("mini")),
    }


@pytest.fixture(scope="module")
def engines(screens):
    from bean_amd import engine

    cache = {}

    def get(which, family, kw, **extra):
        key = (which, family, tuple(sorted((k, str(v)) for k, v in kw.items())), tuple(sorted(extra.items())))
        if key not in cache:
            data = screens[which]
            cache[key] = engine.HipSVI(family, data.to(DEV), num_steps=50, **_kw_of(kw, data), **extra)
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def _which(kw, mini=False):
    return "mini" if mini else ("203acc" if kw.get("scale_by_accessibility") else "203")


def _observed(eng):
    out = {"X": eng._keep["X"]}
    if eng.use_bcmatch:
        out["X_bcmatch"] = eng._keep["X_BC"]
    return out


# ------------------------------------------------------------------ 1. invariants
def _check_invariants(eng):
    obs = _observed(eng)
    a = eng.simulate(3, seed=SEED)
    torch.cuda.synchronize()
    assert set(a) == set(obs)
    for key, x in a.items():
        assert x.dtype == torch.float32 and x.shape == obs[key].shape
        assert bool((x >= 0).all()) and bool((x == x.round()).all()), key
        assert torch.equal(x.double().sum(1), obs[key].double().sum(1)), key  # every pair keeps its observed total
    again = eng.simulate(3, seed=SEED)
    other_draw = eng.simulate(4, seed=SEED)
    other_seed = eng.simulate(3, seed=SEED + 1)
    for key in a:
        assert torch.equal(a[key], again[key]), key
        assert not torch.equal(a[key], other_draw[key]), key
        assert not torch.equal(a[key], other_seed[key]), key
    return a


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_invariants(engines, family, kw):
    eng = engines(_which(kw), family, kw)
    assert eng.predictive_supported
    obs = _observed(eng)
    n = obs["X"].double().sum(1)
    assert float(n[R_EDIT, G_BIG]) == BIG and float(n[R_EDIT, G_ZERO]) == 0 and bool((n % 4 != 0).any())
    assert 300 < float(n[R_EDIT, 64:128].median()) < 800  # the deep pair sits in a wave of totals near 500
    assert not bool(eng._keep["REPGUIDE"].bool().all()) and float(eng._keep["SAMPLE_MASK"].min()) == 0  # masks present
    a = _check_invariants(eng)
    assert float(a["X"][R_EDIT, :, G_ZERO].abs().sum()) == 0
    # a guide's replicate counts do not depend on other guides' counts: double every other guide's, then restore
    keep = torch.zeros(obs["X"].shape[2], dtype=torch.bool, device=DEV)
    keep[torch.tensor([0, 63, 64, G_BIG, 130, 202], device=DEV)] = True
    saved = {k: v.clone() for k, v in obs.items()}
    try:
        for v in obs.values():
            v[:, :, ~keep] *= 2
        b = eng.simulate(3, seed=SEED)
        torch.cuda.synchronize()
    finally:
        for k, v in obs.items():
            v.copy_(saved[k])
    for key in a:
        assert torch.equal(a[key][:, :, keep], b[key][:, :, keep]), key
        assert torch.equal(b[key].double().sum(1), 2 * saved[key].double().sum(1) * (~keep) + saved[key].double().sum(1) * keep)


@pytest.mark.parametrize("family,kw", [CONFIGS[0], CONFIGS[2]])
def test_invariants_on_the_mini_screen(engines, family, kw):
    """30 guides: one partial tile, and the generic k_param prepares the draw."""
    eng = engines("mini", family, kw)
    assert eng.predictive_supported and eng.data.n_guides == 30
    _check_invariants(eng)


# ------------------------------------------------------------------ 2. the draw is the ELBO's
def _oracle_alpha(family, data, eng, kw, noise):
    """The concentrations the oracle's get_alpha (oracle.elbo.dirmult_concentration) forms inside its own forward pass
    for these parameters and this noise, float64 mode: (2, R, B, G), plane 1 zero without X_bcmatch."""
    from oracle import elbo

    seen = []
    real = elbo.dirmult_concentration

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out.detach().permute(0, 2, 1).clone())
        return out

    params = {k: v.detach().cpu().double() for k, v in eng.unconstrained.items()}
    elbo.dirmult_concentration = spy
    try:
        elbo.LOSSES[family](elbo.as_float64(data), params, noise=noise, **kw)
    finally:
        elbo.dirmult_concentration = real
    out = torch.zeros((2,) + tuple(seen[0].shape), dtype=torch.float64)
    for i, a in enumerate(seen):
        out[i] = a
    return out


def _assert_alpha(got, want, n_lik):
    got = got.cpu()
    rel = ((got[:n_lik] - want[:n_lik]).abs() / want[:n_lik]).max().item()
    print(f"alpha_out against the oracle's get_alpha: largest relative difference {rel:.3e}")
    assert rel <= 1e-9, rel
    assert float(got[:n_lik].min()) >= 1e-5


@pytest.mark.parametrize("family,kw", [("Normal", dict()), ("MixtureNormal", dict()),
                                       ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True))])
def test_concentrations_are_the_oracles(engines, screens, family, kw):
    which = _which(kw)
    data = screens[which]
    eng = engines(which, family, kw, dump_noise=True)
    torch.manual_seed(3)
    for v in eng.unconstrained.values():
        v.add_(0.3 * torch.randn_like(v))
    n_lik = 2 if eng.use_bcmatch else 1
    d = 5
    eng.elbo_grad(step=d, seed=SEED)
    noise = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    sim = eng.simulate(d, seed=SEED, alphas=True)
    torch.cuda.synchronize()
    after = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    for k in noise:  # the simulator drew what the ELBO drew, bit for bit
        assert torch.equal(noise[k], after[k]), k
    _assert_alpha(sim["alpha"], _oracle_alpha(family, data, eng, kw, noise), n_lik)
    # handed-in noise is honoured the same way
    g = torch.Generator().manual_seed(9)
    given = {k: (torch.randn(v.shape, generator=g, dtype=torch.float64) if k != "pi" else None) for k, v in noise.items()}
    if "pi" in noise:
        p1 = 0.05 + 0.9 * torch.rand(noise["pi"].shape[:-1], generator=g, dtype=torch.float64)
        given["pi"] = torch.stack([1 - p1, p1], -1)
    eng.set_noise(given)
    try:
        sim = eng.simulate(d + 1, seed=SEED, alphas=True)
        torch.cuda.synchronize()
    finally:
        eng.set_noise(None)
    _assert_alpha(sim["alpha"], _oracle_alpha(family, data, eng, kw, given), n_lik)


# ------------------------------------------------------------------ 3. distribution
@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
def test_draws_have_the_dirichlet_multinomial_moments(family):
    from bean_amd import engine

    S = 512
    data = flat_screen()  # 128 guides x 2 replicates x 5 conditions, no masks, totals 400 ... 600, a0 = 50
    kw = dict(use_bcmatch=False) if family == "Normal" else {}
    eng = engine.HipSVI(family, data.to(DEV), num_steps=50, **kw)
    for k in ("mu_scale", "sd_scale"):
        eng.unconstrained[k].fill_(-20.0)  # the latent sites are fixed
    if family == "MixtureNormal":
        g = torch.Generator().manual_seed(2)
        p1 = 0.1 + 0.8 * torch.rand((data.n_reps, data.n_guides), generator=g, dtype=torch.float64)
        eng.set_noise({"pi": torch.stack([1 - p1, p1], -1)})
    keys = ["X"] + (["X_bcmatch"] if eng.use_bcmatch else [])
    first = eng.simulate(0, seed=SEED, alphas=True)
    alpha = first["alpha"].clone()
    s1 = {k: torch.zeros_like(first[k], dtype=torch.float64) for k in keys}
    s2 = {k: torch.zeros_like(first[k], dtype=torch.float64) for k in keys}
    for d in range(S):
        sim = eng.simulate(d, seed=SEED, alphas=True)
        # scales of exp(-20) fix the sites to 2e-9: the same concentrations at every draw, to that order
        assert float(((sim["alpha"] - alpha).abs() / alpha.clamp(min=1e-5)).max()) < 1e-7
        for k in keys:
            x = sim[k].double()
            s1[k] += x
            s2[k] += x * x
    torch.cuda.synchronize()
    for i, k in enumerate(keys):
        al = alpha[i]
        A0 = al.sum(1, keepdim=True)
        n = eng._keep["X" if k == "X" else "X_BC"].double().sum(1, keepdim=True)
        m = n * al / A0
        v = m * (1 - al / A0) * (n + A0) / (1 + A0)
        assert float(m.min()) >= 40, float(m.min())
        mean = s1[k] / S
        var = (s2[k] - S * mean * mean) / (S - 1)
        z = (mean - m) / (v / S).sqrt()
        ratio = var / v
        pooled = float(var.sum() / v.sum())
        print(f"{family} {k}: max |z| {float(z.abs().max()):.2f}, sd of z {float(z.std()):.3f}, pooled variance ratio "
              f"{pooled:.4f}, cell ratios {float(ratio.min()):.3f} ... {float(ratio.max()):.3f}")
        assert float(z.abs().max()) <= 5.0
        assert 0.9 <= float(z.std()) <= 1.1
        assert 0.95 <= pooled <= 1.05
        assert 0.6 <= float(ratio.min()) and float(ratio.max()) <= 1.5
    eng.close()


# ------------------------------------------------------------------ 4. untouched state
def test_simulate_leaves_the_fit_alone(screens):
    from bean_amd import engine

    data = screens["203"].to(DEV)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(20, seed=SEED)
    torch.cuda.synchronize()
    before = _state(eng)
    grads = {k: v.clone() for k, v in eng.grads.items()}
    hist = eng.loss_hist.clone()
    eng.simulate(2, seed=7)
    torch.cuda.synchronize()
    after = _state(eng)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k in grads:
        assert torch.equal(grads[k], eng.grads[k]), k
    assert torch.equal(hist, eng.loss_hist)
    eng.close()

    def fit(simulate_first, resume):
        e = engine.HipSVI("MixtureNormal", data, num_steps=300)
        if resume:
            e.run(10, seed=SEED, resume=True)
        if simulate_first == "raw":
            # the library call alone, behind the engine's back: the handle itself must forget the prepared draw
            x = torch.empty_like(e._keep["X"])
            xbc = torch.empty_like(e._keep["X_BC"])
            nb = x.numel() * 4
            assert e.lib.bean_hip_simulate(e._h, SEED + 5, 1, ctypes.c_void_p(x.data_ptr()), nb,
                                           ctypes.c_void_p(xbc.data_ptr()), nb, None, 0, e._sptr()) == 0
        elif simulate_first:
            e.simulate(1, seed=SEED + 5)
        e.run(40, seed=SEED, resume=resume)
        torch.cuda.synchronize()
        st = _state(e)
        e.close()
        return st

    plain, simulated = fit(False, False), fit(True, False)
    for k in plain:
        assert torch.equal(plain[k], simulated[k]), k
    # a resumed window after a simulate does not step on the simulator's draw
    plain = fit(False, True)
    for how in (True, "raw"):
        simulated = fit(how, True)
        for k in plain:
            assert torch.equal(plain[k], simulated[k]), (how, k)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["203"].to(DEV)
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    n = R * B * G
    x = torch.zeros(n, dtype=torch.float32, device=DEV)
    xbc = torch.zeros(n, dtype=torch.float32, device=DEV)
    al = torch.zeros(2 * n, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    sim = lambda *a: lib.bean_hip_simulate(eng._h, SEED, 0, *a, eng._sptr())  # noqa: E731
    assert sim(p(x), 4 * n - 4, p(xbc), 4 * n, None, 0) < 0 and "x_out" in err()
    assert sim(None, 0, p(xbc), 4 * n, None, 0) < 0 and "x_out" in err()
    assert sim(p(x), 4 * n, p(xbc), 4 * n + 4, None, 0) < 0 and "xbc_out" in err()
    assert sim(p(x), 4 * n, None, 0, None, 0) < 0 and "xbc_out" in err()
    assert sim(p(x), 4 * n, p(xbc), 4 * n, p(al), 8 * n) < 0 and "alpha_out" in err()
    assert sim(p(x), 4 * n, p(xbc), 4 * n, None, 8) < 0 and "alpha_out" in err()
    assert lib.bean_hip_simulate(None, SEED, 0, p(x), 4 * n, None, 0, None, 0, None) < 0 and "null handle" in err()
    assert sim(p(x), 4 * n, p(xbc), 4 * n, p(al), 16 * n) == 0
    torch.cuda.synchronize()
    assert float(x.sum()) == float(eng._keep["X"].sum())
    eng.close()

    nobc = engine.HipSVI("MixtureNormal", data, num_steps=50, use_bcmatch=False)
    assert lib.bean_hip_simulate(nobc._h, SEED, 0, p(x), 4 * n, p(xbc), 4 * n, None, 0, nobc._sptr()) < 0 and "xbc_out" in err()
    assert set(nobc.simulate(0)) == {"X"}
    # an unprepared handle of the same shape
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(nobc._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_predictive_supported(h) == 1
    assert lib.bean_hip_simulate(h, SEED, 0, p(x), 4 * n, None, 0, None, 0, None) < 0 and "bean_hip_prepare" in err()
    assert lib.bean_hip_destroy(h) == 0
    nobc.close()

    for extra in (dict(n_members=2), dict(n_particles=2)):
        many = engine.HipSVI("MixtureNormal", data, num_steps=50, **extra)
        assert not many.predictive_supported
        assert lib.bean_hip_simulate(many._h, SEED, 0, p(x), 4 * n, p(xbc), 4 * n, None, 0, many._sptr()) < 0
        assert "bean_hip_predictive_supported" in err()
        with pytest.raises(PredictiveUnsupported):
            many.simulate(0)
        if "n_members" in extra:
            many.run_ensemble(5, [1, 2])
        else:
            many.run_particles(5, SEED)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(many.loss_hist[..., :5]).all())
        many.close()

    for other in (engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10)):
        assert not other.predictive_supported
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.simulate(0)
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()


# ------------------------------------------------------------------ 6. end to end
def _true_parameter_share(data, n_draws=200, seed=0):
    """Share of guides with ppc_p_score <= 0.05 when the replicate screens come from the generator's own true mu, sd and
    pi (through the model's concentrations, the oracle's get_alpha) - a numpy loop around _dirmult_counts, on the CPU."""
    from scipy.special import ndtr, ndtri

    from bean_amd.model.predictive import bin_midpoints, predictive_summary
    from oracle import elbo

    R, B, G = data.n_reps, data.n_condits, data.n_guides
    lo, hi = data.lower_bounds.numpy(), data.upper_bounds.numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        z_hi = np.where(hi >= 1.0, np.inf, ndtri(np.clip(hi, 1e-300, 1)))
        z_lo = np.where(lo <= 0.0, -np.inf, ndtri(np.clip(lo, 1e-300, 1)))
    g2t = data.guide_to_target.numpy()
    mu, sd, pi = data.truth["mu"][g2t], data.truth["sd"][g2t], data.truth["pi"]
    p_wt = ndtr(z_hi) - ndtr(z_lo)
    p_ed = ndtr((z_hi[:, None] - mu[None]) / sd[None]) - ndtr((z_lo[:, None] - mu[None]) / sd[None])
    e = (1 - pi)[None] * p_wt[:, None] + pi[None] * p_ed
    expected = torch.as_tensor(e, dtype=torch.float64)[None].expand(R, B, G)
    alpha = elbo.dirmult_concentration(expected, data.size_factor, data.sample_mask.double(), data.a0).numpy()
    x_obs = data.X_masked.double()
    n = x_obs.sum(1).numpy().astype(np.int64)
    rng = np.random.default_rng(seed)
    reps = ({"X": torch.as_tensor(np.moveaxis(_dirmult_counts(rng, n, alpha), -1, 1).astype(np.float64))}
            for _ in range(n_draws))
    masks = {"repguide": data.repguide_mask, "sample": data.sample_mask, "mask_thres": 10}
    p = predictive_summary({"X": x_obs}, reps, masks, bin_midpoints(data.upper_bounds, data.lower_bounds))["ppc_p_score"]
    ok = ~torch.isnan(p)
    return float((p[ok] <= 0.05).double().mean())


# _true_parameter_share(make_sorting_variant_screen(640, 3, seed=2), 200, seed=0), measured on the CPU: 320 of 640 guides.
# (Half of them, with the TRUE parameters: the generator sequences the bulk sample at a fifth of its share of the cells,
# while the model's concentrations give a sample the share e_b sf_b with sf the normalised column means - the bulk's
# expected share is 0.55 where the screen holds 0.2, so the replicates' scores are pulled towards the bulk's midpoint
# and vary less than the observed ones.  The check reports that; the cap below is relative to it.)
TRUE_SHARE_MEASURED = 0.5


def test_check_finds_planted_misfit_and_passes_the_rest():
    """A screen drawn from the model itself, fitted for 300 steps: ten guides whose reads all sit in the top bin must be
    flagged at the smallest p the check can give, and among the untouched guides the share with ppc_p_score <= 0.05
    stays below the share measured with the generator's true parameters plus 0.05 (the room a 300-step fit's error
    takes).  Measured share with the true parameters, S = 200, seed 0: 0.5 (TRUE_SHARE_MEASURED), so the cap is 0.55."""
    import bean_amd.model.model as m
    from bean_amd.model.run import run_inference, run_posterior_predictive

    S = 200
    data = make_sorting_variant_screen(640, 3, seed=2)
    share_true = _true_parameter_share(data, S)
    assert abs(share_true - TRUE_SHARE_MEASURED) < 1e-12, share_true  # seeded: the recorded figure
    cap = share_true + 0.05
    model, guide = partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)
    planted = copy.copy(data)
    top = int(np.lexsort((data.lower_bounds.numpy(), data.upper_bounds.numpy()))[-1])
    assert float(data.lower_bounds[top]) == 0.8 and float(data.upper_bounds[top]) == 1.0
    picked = torch.tensor([3 + 61 * k for k in range(10)])
    assert bool(data.repguide_mask[:, picked].all())
    for name in ("X", "X_masked", "X_bcmatch", "X_bcmatch_masked"):
        x = getattr(data, name).clone()
        tot = x[:, :, picked].sum(1)
        x[:, :, picked] = 0
        x[:, top, picked] = tot
        setattr(planted, name, x)
    shares = {}
    for what, screen in (("as drawn", data), ("planted", planted)):
        store, _ = run_inference(model, guide, screen, num_steps=300, verbose=False)
        summ = run_posterior_predictive(model, guide, screen, store, n_draws=S)
        p = summ["ppc_p_score"].cpu()
        rest = torch.ones(data.n_guides, dtype=torch.bool)
        if what == "planted":
            rest[picked] = False
            assert bool((p[picked] <= 2.0 / (S + 1)).all()), p[picked]
        ok = rest & ~torch.isnan(p)
        shares[what] = float((p[ok] <= 0.05).double().mean())
        print(f"{what}: share of untouched guides with ppc_p_score <= 0.05: {shares[what]:.4f} "
              f"(true parameters {share_true:.4f}, cap {cap:.4f})")
        assert summ["n_draws"] == S and summ["ppc_p_score_bcmatch"].shape == p.shape
    assert shares["as drawn"] <= cap and shares["planted"] <= cap, (shares, cap)


# ------------------------------------------------------------------ 7. CLI
def test_cli_posterior_predictive(tmp_path, capsys):
    from bean_amd.cli.execute import main as bean_main

    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    d1 = _run(str(tmp_path / "ppc"), *base, "--posterior-predictive", "50")
    d0 = _run(str(tmp_path / "plain"), *base)
    for name in ("bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"):
        assert open(f"{d1}/{name}", "rb").read() == open(f"{d0}/{name}", "rb").read(), name
    assert not os.path.exists(f"{d0}/bean_predictive_guides.MixtureNormal.csv")
    guides = pd.read_csv(f"{d1}/bean_predictive_guides.MixtureNormal.csv", index_col=0)
    sg = pd.read_csv(f"{d1}/bean_sgRNA_result.MixtureNormal.csv", index_col=0)
    own = [c + s for s in ("", "_bcmatch") for c in ("ppc_p_score", "ppc_p_spread", "ppc_z_score")]
    assert list(guides.columns) == list(sg.columns) + own and list(guides.index) == list(sg.index) and len(guides) == 30
    p = guides["ppc_p_score"].dropna()
    assert len(p) and bool(((p >= 1 / 51) & (p <= 1)).all())
    samples = pd.read_csv(f"{d1}/bean_predictive_samples.MixtureNormal.csv", index_col=0)
    data = _mini(tmp_path / "data")
    assert len(samples) == data.n_reps * data.n_condits
    assert {"replicate", "condition", "masked", "frac_cells_p05", "mean_z", "frac_cells_p05_bcmatch", "mean_z_bcmatch",
            "n_draws"} <= set(samples.columns)
    assert bool((samples["n_draws"] == 50).all())
    til = os.path.join(os.path.dirname(VAR), "tiling_mini_screen.h5ad")
    with pytest.raises(SystemExit) as exc:
        bean_main(["run", "sorting", "tiling", til, "--posterior-predictive", "50", "-o", str(tmp_path / "til")])
    assert exc.value.code == 2
    msg = capsys.readouterr().err
    assert "--posterior-predictive" in msg and "tiling" in msg and "MultiMixtureNormal" in msg
