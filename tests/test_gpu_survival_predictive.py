"""Posterior predictive check of survival screens on the GPU: the survival count simulator (bean_hip_simulate_survival,
csrc/bean_survival_predictive.hpp), its draws against the ELBO's, its concentrations against the oracle's get_alpha
inside oracle.survival, its counts against the exact beta-binomial marginals, the state it must leave alone, its
refusals, and the check end to end.  Every screen has depth_per_guide = 100: totals near 500.  -m gpu."""
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
from bean_amd.preprocessing.synthetic import (make_sorting_variant_screen, make_survival_tiling_screen,
                                               make_survival_variant_screen)

import dm_reference as dm
from members_common import DEV, GOLD, _h5ad_reader_present, _run, _state  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = 101
DEPTH = 100.0
BIG = 5003   # one pair's total inside a wave of totals near 500
G_BIG, G_ZERO, R_EDIT = 70, 75, 1  # both in the second tile of replicate 1
SURV = os.path.join(GOLD, "survival_var_mini_screen.h5ad")
T3 = (0.0, 7.0, 14.0)
T11 = tuple(float(t) for t in range(0, 22, 2))
T40 = tuple(0.5 * t for t in range(0, 40))

FAMILIES = [("Normal", dict()), ("MixtureNormal", dict()),
            ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True))]


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


def _screen(n_guides, n_reps, acc=False, **kw):
    return make_survival_variant_screen(n_guides, n_reps, depth_per_guide=DEPTH, with_accessibility=acc, **kw)


@pytest.fixture(scope="module")
def screens():
    return {
        "203": _edited(_screen(203, 3, seed=11, mask_fraction=0.05)),
        "203acc": _edited(_screen(203, 3, acc=True, seed=11, mask_fraction=0.05)),
    }


def _which(kw):
    return "203acc" if kw.get("scale_by_accessibility") else "203"


def _observed(eng):
    out = {"X": eng._keep["X"]}
    if eng.use_bcmatch:
        out["X_bcmatch"] = eng._keep["X_BC"]
    return out


# ------------------------------------------------------------------ 1. invariants
def _check_invariants(eng):
    obs = _observed(eng)
    a = eng.simulate_survival(3, seed=SEED)
    torch.cuda.synchronize()
    assert set(a) == set(obs) == {"X", "X_bcmatch"}
    for key, x in a.items():
        assert x.dtype == torch.float32 and x.shape == obs[key].shape
        assert bool((x >= 0).all()) and bool((x == x.round()).all()), key
        assert torch.equal(x.double().sum(1), obs[key].double().sum(1)), key  # every pair keeps its observed total
    again = eng.simulate_survival(3, seed=SEED)
    other_draw = eng.simulate_survival(4, seed=SEED)
    other_seed = eng.simulate_survival(3, seed=SEED + 1)
    for key in a:
        assert torch.equal(a[key], again[key]), key
        assert not torch.equal(a[key], other_draw[key]), key
        assert not torch.equal(a[key], other_seed[key]), key
    return a


@pytest.mark.parametrize("family,kw", FAMILIES)
def test_invariants(screens, family, kw):
    from bean_amd import engine

    eng = engine.HipSVI(family, screens[_which(kw)].to(DEV), num_steps=50, **kw)
    try:
        assert eng.survival_predictive_supported and not eng.predictive_supported
        obs = _observed(eng)
        n = obs["X"].double().sum(1)
        assert float(n[R_EDIT, G_BIG]) == BIG and float(n[R_EDIT, G_ZERO]) == 0 and bool((n % 4 != 0).any())
        assert 300 < float(n[R_EDIT, 64:128].median()) < 800  # the deep pair sits in a wave of totals near 500
        assert not bool(eng._keep["REPGUIDE"].bool().all()) and float(eng._keep["SAMPLE_MASK"].min()) == 0  # masks present
        a = _check_invariants(eng)
        for key in a:
            assert float(a[key][R_EDIT, :, G_ZERO].abs().sum()) == 0, key
        # a guide's replicate counts do not depend on other guides' counts: double every other guide's, then restore
        keep = torch.zeros(obs["X"].shape[2], dtype=torch.bool, device=DEV)
        keep[torch.tensor([0, 63, 64, G_BIG, 130, 202], device=DEV)] = True
        saved = {k: v.clone() for k, v in obs.items()}
        try:
            for v in obs.values():
                v[:, :, ~keep] *= 2
            b = eng.simulate_survival(3, seed=SEED)
            torch.cuda.synchronize()
        finally:
            for k, v in obs.items():
                v.copy_(saved[k])
        for key in a:
            assert torch.equal(a[key][:, :, keep], b[key][:, :, keep]), key
            n0 = saved[key].double().sum(1)
            assert torch.equal(b[key].double().sum(1), 2 * n0 * (~keep) + n0 * keep)
    finally:
        eng.close()


@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
@pytest.mark.parametrize("gen_kw", [
    dict(n_guides=30, n_reps=1),                 # one partial tile
    dict(n_guides=90, n_reps=2, times=T3),       # odd B: a lone bin in the last gamma pair
    dict(n_guides=90, n_reps=2, times=T11),      # the 16-condition build, B beyond the register batch
    dict(n_guides=70, n_reps=2, times=T40),      # 40 timepoints: the columns take more than 64 KB of LDS
], ids=["30x1", "3-timepoints", "11-timepoints", "40-timepoints"])
def test_invariants_at_other_shapes(family, gen_kw):
    from bean_amd import engine

    # (a masked sample needs a second replicate that holds the timepoint)
    data = make_survival_variant_screen(seed=4, depth_per_guide=DEPTH, mask_fraction=0.05 if gen_kw["n_reps"] > 1 else 0.0,
                                        **gen_kw)
    eng = engine.HipSVI(family, data.to(DEV), num_steps=50)
    try:
        assert eng.survival_predictive_supported and data.n_condits == len(gen_kw.get("times", range(6)))
        _check_invariants(eng)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. the draw is the ELBO's
def _oracle_alpha(family, data, eng, kw, noise):
    """The concentrations the oracle's get_alpha (oracle.elbo.dirmult_concentration) forms inside the forward pass of
    oracle.survival.LOSSES[family] for these parameters and this noise, float64 mode: (2, R, B, G)."""
    from oracle import elbo
    from oracle import survival as osurv

    seen = []
    real = elbo.dirmult_concentration

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out.detach().permute(0, 2, 1).clone())
        return out

    params = {k: v.detach().cpu().double() for k, v in eng.unconstrained.items()}
    elbo.dirmult_concentration = spy
    try:
        osurv.LOSSES[family](elbo.as_float64(data), params, noise=noise, **kw)
    finally:
        elbo.dirmult_concentration = real
    assert len(seen) == 2
    return torch.stack(seen)


def _assert_alpha(got, want):
    got = got.cpu()
    rel = ((got - want).abs() / want).max().item()
    print(f"alpha_out against the oracle's get_alpha: largest relative difference {rel:.3e}")
    assert rel <= 1e-9, rel
    assert float(got.min()) >= 1e-5


@pytest.mark.parametrize("family,kw,drop_idx", [(f, k, False) for f, k in FAMILIES] + [("Normal", dict(), True)],
                         ids=["Normal", "MixtureNormal", "MixtureNormal+Acc", "Normal-no-negctrl-index"])
def test_draws_and_concentrations_are_the_elbos(screens, family, kw, drop_idx):
    from bean_amd import engine

    data = screens[_which(kw)]
    if drop_idx:
        data = copy.copy(data)
        data.negctrl_guide_idx = None
    else:
        assert data.negctrl_guide_idx is not None and 0 < len(data.negctrl_guide_idx) < data.n_guides
    eng = engine.HipSVI(family, data.to(DEV), num_steps=50, dump_noise=True, **kw)
    try:
        torch.manual_seed(3)
        for v in eng.unconstrained.values():
            v.add_(0.3 * torch.randn_like(v))
        d = 5
        eng.elbo_grad(step=d, seed=SEED)
        noise = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        want_keys = {"eps_mu", "q_0"} if family == "Normal" else {"eps_mu", "pi", "mu_negctrl", "initial_abundance"}
        if kw.get("scale_by_accessibility"):
            want_keys.add("eps_noise")
        assert want_keys <= set(noise), sorted(noise)
        eng.elbo_grad(step=d + 1, seed=SEED)
        other = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        assert all(not torch.equal(noise[k], other[k]) for k in want_keys)
        sim = eng.simulate_survival(d, seed=SEED, alphas=True)
        torch.cuda.synchronize()
        after = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        assert set(after) == set(noise)
        for k in noise:  # the simulator drew what the ELBO drew, bit for bit
            assert torch.equal(noise[k], after[k]), k
        _assert_alpha(sim["alpha"], _oracle_alpha(family, data, eng, kw, noise))
        # handed-in noise is honoured the same way
        g = torch.Generator().manual_seed(9)
        given = {}
        for k, v in noise.items():
            if k == "pi":
                p1 = 0.05 + 0.9 * torch.rand(v.shape[:-1], generator=g, dtype=torch.float64)
                given[k] = torch.stack([1 - p1, p1], -1)
            elif k in ("q_0", "initial_abundance"):
                e = -torch.log(torch.rand(v.shape, generator=g, dtype=torch.float64))
                given[k] = e / e.sum(-1, keepdim=True)
            elif k == "mu_negctrl":
                given[k] = 0.1 * torch.randn(v.shape, generator=g, dtype=torch.float64)
            else:
                given[k] = torch.randn(v.shape, generator=g, dtype=torch.float64)
        eng.set_noise(given)
        try:
            sim = eng.simulate_survival(d + 1, seed=SEED, alphas=True)
            torch.cuda.synchronize()
        finally:
            eng.set_noise(None)
        _assert_alpha(sim["alpha"], _oracle_alpha(family, data, eng, kw, given))
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. the law
# p-values per configuration: timepoints x 2 likelihoods (both are tested everywhere)
LAW = [
    ("Normal", dict(), dict(), 12),
    ("MixtureNormal", dict(), dict(), 12),
    ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True), dict(), 12),
    ("MixtureNormal", dict(), dict(times=T3), 6),
    ("MixtureNormal", dict(), dict(times=T11), 22),
]
N_P = sum(c[3] for c in LAW)
assert N_P == 64
P_MIN = 1e-3 / N_P
LAW_DRAWS = 64


def _fixed_noise(eng, data, family, kw, seed=2):
    """Every latent of the draw handed in: pi, the Dirichlet-over-guides draw, the baseline and the guide noise."""
    g = torch.Generator().manual_seed(seed)
    R, G = data.n_reps, data.n_guides
    e = -torch.log(torch.rand((R, G), generator=g, dtype=torch.float64))
    noise = {("q_0" if family == "Normal" else "initial_abundance"): e / e.sum(-1, keepdim=True)}
    if family == "MixtureNormal":
        p1 = 0.1 + 0.8 * torch.rand((R, G), generator=g, dtype=torch.float64)
        noise["pi"] = torch.stack([1 - p1, p1], -1)
        noise["mu_negctrl"] = 0.1 * torch.randn(G, generator=g, dtype=torch.float64)
    if kw.get("scale_by_accessibility"):
        noise["eps_noise"] = torch.randn(G, generator=g, dtype=torch.float64)
    return noise


@pytest.mark.parametrize("family,kw,gen_kw,n_p", LAW,
                         ids=["Normal", "MixtureNormal", "MixtureNormal+Acc", "3-timepoints", "11-timepoints"])
def test_counts_follow_the_beta_binomial_marginals(family, kw, gen_kw, n_p):
    """64 screens of 128 guides x 2 replicates with every latent fixed, held to the exact marginals of the exported
    concentrations and the observed totals: every p-value above 1e-3 / 64.  The draws are deterministic."""
    from bean_amd import engine

    data = _screen(128, 2, acc=bool(kw.get("scale_by_accessibility")), seed=21, mask_fraction=0.05, **gen_kw)
    eng = engine.HipSVI(family, data.to(DEV), num_steps=50, **kw)
    try:
        torch.manual_seed(5)
        for k, v in eng.unconstrained.items():
            if k.endswith("_scale"):
                v.fill_(-20.0)  # the Normal sites are fixed to 2e-9
            else:
                v.add_(0.3 * torch.randn_like(v))
        eng.set_noise(_fixed_noise(eng, data, family, kw))
        planes = {"X": [], "X_bcmatch": []}
        alpha = None
        for d in range(LAW_DRAWS):
            sim = eng.simulate_survival(d, seed=SEED, alphas=True)
            if alpha is None:
                alpha = sim["alpha"].clone()
            assert float(((sim["alpha"] - alpha).abs() / alpha).max()) < 1e-7
            for k in planes:
                planes[k].append(sim[k].cpu().numpy())
        torch.cuda.synchronize()
        alpha = alpha.cpu().numpy()
        keep = eng._keep["SAMPLE_MASK"].cpu().numpy() != 0
        assert not keep.all()
        rng = np.random.default_rng(7)
        ps = []
        for i, (k, slot) in enumerate((("X", "X"), ("X_bcmatch", "X_BC"))):
            n = eng._keep[slot].double().sum(1).cpu().numpy().astype(np.int64)
            got = dm.pit_marginals(np.stack(planes[k]), n, alpha[i], rng, keep=keep)
            ps += [(k, b, p) for b, p in got]
        smallest = min(p for _, _, p in ps)
        print(f"{family} {kw} {gen_kw}: {len(ps)} p-values, smallest {smallest:.3e} (threshold {P_MIN:.3e})")
        assert len(ps) == n_p
        assert smallest > P_MIN, sorted(ps, key=lambda t: t[2])[:3]
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. the fit is left alone
def test_simulate_survival_leaves_the_fit_alone(screens):
    from bean_amd import engine

    data = screens["203"].to(DEV)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(20, seed=SEED)
    torch.cuda.synchronize()
    before = _state(eng)
    hist = eng.loss_hist.clone()
    eng.simulate_survival(2, seed=7)
    torch.cuda.synchronize()
    after = _state(eng)
    for k in before:
        assert torch.equal(before[k], after[k]), k
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
            assert e.lib.bean_hip_simulate_survival(e._h, SEED + 5, 1, ctypes.c_void_p(x.data_ptr()), nb,
                                                    ctypes.c_void_p(xbc.data_ptr()), nb, None, 0, e._sptr()) == 0
        elif simulate_first:
            e.simulate_survival(1, seed=SEED + 5)
        e.run(40, seed=SEED, resume=resume)
        torch.cuda.synchronize()
        st = _state(e)
        e.close()
        return st

    plain, simulated = fit(False, False), fit(True, False)
    for k in plain:
        assert torch.equal(plain[k], simulated[k]), k
    # a resumed window after a simulate does not step on the simulator's draw: it is a plain run
    plain = fit(False, True)
    for how in (True, "raw"):
        simulated = fit(how, True)
        for k in plain:
            assert torch.equal(plain[k], simulated[k]), (how, k)


# ------------------------------------------------------------------ 5. refusals
NAME = "bean_hip_simulate_survival"
ADMIT = (NAME + ": the survival count simulator does not take this handle (bean_hip_survival_predictive_supported): "
         "survival variant Normal / MixtureNormal, unsharded, no sample covariates, one member, one particle")
FILL = -7.0


def test_refusals_are_pinned_and_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["203"]
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    n = R * B * G
    x = torch.full((n,), FILL, dtype=torch.float32, device=DEV)
    xbc = torch.full((n,), FILL, dtype=torch.float32, device=DEV)
    al = torch.full((2 * n,), FILL, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def refused(handle, stream, message, *a):
        assert lib.bean_hip_simulate_survival(handle, SEED, 0, *a, stream) < 0
        assert err() == message, err()
        torch.cuda.synchronize()
        for t in (x, xbc, al):  # nothing was launched
            assert bool((t == FILL).all())

    good = (p(x), 4 * n, p(xbc), 4 * n, p(al), 16 * n)
    refused(None, None, NAME + ": null handle", *good)
    assert lib.bean_hip_survival_predictive_supported(None) < 0
    assert err() == "bean_hip_survival_predictive_supported: null handle"

    # handles of other shapes: sorting (one fit, two members, two particles), tiling, ControlNormal
    sorting = make_sorting_variant_screen(203, 3, seed=11, depth_per_guide=DEPTH)
    assert (sorting.n_reps, sorting.n_guides) == (R, G)
    ns = R * sorting.n_condits * G
    others = [
        (engine.HipSVI("MixtureNormal", sorting.to(DEV), num_steps=10), ns),
        (engine.HipSVI("MixtureNormal", sorting.to(DEV), num_steps=10, n_members=2), ns),
        (engine.HipSVI("MixtureNormal", sorting.to(DEV), num_steps=10, n_particles=2), ns),
    ]
    til = make_survival_tiling_screen(64, 2, seed=2)
    others.append((engine.HipSVI("MultiMixtureNormal", til.to(DEV), num_steps=10),
                   til.n_reps * til.n_condits * til.n_guides))
    surv = make_survival_variant_screen(400, 3, seed=5, depth_per_guide=DEPTH)
    ctrl = surv[surv.negctrl_guide_idx]
    others.append((engine.HipSVI("ControlNormal", ctrl.to(DEV), num_steps=10), ctrl.n_reps * ctrl.n_condits * ctrl.n_guides))
    for other, size in others:
        assert size <= n
        assert not other.survival_predictive_supported
        assert lib.bean_hip_survival_predictive_supported(other._h) == 0
        refused(other._h, other._sptr(), ADMIT, p(x), 4 * size, p(xbc), 4 * size, None, 0)
        refused(other._h, other._sptr(), ADMIT, None, 0, None, 0, None, 8)  # the admission comes before the buffers
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.simulate_survival(0)
        if other.n_members > 1:
            other.run_ensemble(5, [1, 2])
        elif other.n_particles > 1:
            other.run_particles(5, SEED)
        else:
            other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(other.loss_hist[..., :5]).all())
        other.close()

    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
    assert lib.bean_hip_survival_predictive_supported(eng._h) == 1
    s = eng._sptr()
    held = f"(R, B, G) float32, {4 * n} bytes"
    x_msg = NAME + ": x_out must hold " + held
    bc_msg = NAME + ": this handle uses the barcode-matched counts: xbc_out must hold " + held
    al_msg = NAME + f": alpha_out must be null or hold (2, R, B, G) float64, {16 * n} bytes"
    refused(eng._h, s, x_msg, p(x), 4 * n - 4, p(xbc), 4 * n, None, 0)
    refused(eng._h, s, x_msg, p(x), 4 * n + 4, p(xbc), 4 * n, None, 0)
    refused(eng._h, s, x_msg, None, 0, p(xbc), 4 * n, None, 0)
    refused(eng._h, s, x_msg, None, 4 * n, p(xbc), 4 * n, None, 0)
    refused(eng._h, s, bc_msg, p(x), 4 * n, p(xbc), 4 * n + 4, None, 0)
    refused(eng._h, s, bc_msg, p(x), 4 * n, None, 0, None, 0)
    refused(eng._h, s, bc_msg, p(x), 4 * n, None, 4 * n, None, 0)
    refused(eng._h, s, al_msg, p(x), 4 * n, p(xbc), 4 * n, p(al), 8 * n)
    refused(eng._h, s, al_msg, p(x), 4 * n, p(xbc), 4 * n, p(al), 0)
    refused(eng._h, s, al_msg, p(x), 4 * n, p(xbc), 4 * n, None, 8)
    refused(eng._h, s, x_msg, p(x), 4 * n - 4, None, 0, p(al), 8)  # x_out, then xbc_out, then alpha_out
    refused(eng._h, s, bc_msg, p(x), 4 * n, None, 0, p(al), 8)
    with pytest.raises(PredictiveUnsupported, match="MixtureNormal, survival"):
        eng.simulate(0)
    assert lib.bean_hip_simulate_survival(eng._h, SEED, 0, *good, s) == 0
    torch.cuda.synchronize()
    assert float(x.sum()) == float(eng._keep["X"].sum()) and float(xbc.sum()) == float(eng._keep["X_BC"].sum())
    assert float(al.min()) >= 1e-5
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()
    x.fill_(FILL), xbc.fill_(FILL), al.fill_(FILL)

    nobc = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50, use_bcmatch=False)
    no_bc = NAME + ": xbc_out on a handle without BEAN_FLAG_USE_BCMATCH"
    refused(nobc._h, nobc._sptr(), no_bc, p(x), 4 * n, p(xbc), 4 * n, None, 0)
    refused(nobc._h, nobc._sptr(), no_bc, p(x), 4 * n, None, 4, None, 0)
    refused(nobc._h, nobc._sptr(), no_bc, p(x), 4 * n, p(xbc), 0, None, 0)
    assert set(nobc.simulate_survival(0)) == {"X"}
    # an unprepared handle of the same shape
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(nobc._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_survival_predictive_supported(h) == 1
    refused(h, None, NAME + ": call bean_hip_prepare first", p(x), 4 * n, None, 0, None, 0)
    refused(h, None, NAME + ": call bean_hip_prepare first", None, 0, p(xbc), 4, None, 0)  # ... before the buffers
    assert lib.bean_hip_destroy(h) == 0
    nobc.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(nobc.losses()).all()
    nobc.close()


# ------------------------------------------------------------------ 6. end to end
def _with_counts(data, x, x_bc):
    out = copy.copy(data)
    for name, v in (("X", x), ("X_masked", x), ("X_bcmatch", x_bc), ("X_bcmatch_masked", x_bc)):
        setattr(out, name, v.detach().cpu().clone())
    return out


@pytest.mark.parametrize("family", ["MixtureNormal", "Normal"])
def test_check_is_calibrated_on_its_own_draw_and_finds_planted_misfit(family):
    """A 300-step fit; a screen drawn by the simulator itself (seed 7, draw 0) as the observed counts of a second engine
    with the same parameters is one draw from the distribution the check draws from, so P(ppc_p_score <= 0.05) <= 0.05
    per guide; with the 128 targets as the independent units in the worst case (their guides share mu_t) the share has a
    standard deviation of at most sqrt(0.05 * 0.95 / 128) = 0.019: cap 0.05 + 5 * 0.019 = 0.15.  Then ten guides of the
    ORIGINAL screen with every read at the last timepoint: the smallest p the check can give, and z > 0."""
    import bean_amd.model.survival_model as sm
    from bean_amd.model.predictive import survival_predictive
    from bean_amd.model.run import build_engine, load_parameters, run_inference

    S = 200
    data = _screen(640, 3, seed=2, mask_fraction=0.0)
    assert data.n_targets == 128
    if family == "MixtureNormal":
        model, guide = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)
    else:
        model, guide = partial(sm.NormalModel), sm.NormalGuide
    store, _ = run_inference(model, guide, data, num_steps=300, verbose=False)

    def check(screen):
        eng = build_engine(model, guide, screen.to(DEV), num_steps=1, device=torch.device(DEV))
        try:
            load_parameters(eng, store)
            return survival_predictive(eng, n_draws=S, seed=SEED)
        finally:
            eng.close()

    first = build_engine(model, guide, data.to(DEV), num_steps=1, device=torch.device(DEV))
    try:
        load_parameters(first, store)
        sim = first.simulate_survival(0, seed=7)
        torch.cuda.synchronize()
    finally:
        first.close()
    summ = check(_with_counts(data, sim["X"], sim["X_bcmatch"]))
    assert summ["n_draws"] == S
    cap = 0.05 + 5 * np.sqrt(0.05 * 0.95 / 128)
    for key in ("ppc_p_score", "ppc_p_score_bcmatch"):
        p = summ[key].cpu()
        ok = ~torch.isnan(p)
        assert int(ok.sum()) > 600
        share = float((p[ok] <= 0.05).double().mean())
        print(f"{family} {key}: share of guides with p <= 0.05 on the simulator's own draw: {share:.4f} (cap {cap:.4f})")
        assert share <= cap, (key, share)

    picked = torch.nonzero(data.repguide_mask.all(0)).reshape(-1)[::60][:10]
    assert len(picked) == 10
    x, x_bc = data.X.clone(), data.X_bcmatch.clone()
    for v in (x, x_bc):
        tot = v[:, :, picked].sum(1)
        v[:, :, picked] = 0
        v[:, -1, picked] = tot
    assert float(data.timepoints[-1]) == float(data.timepoints.max())
    summ = check(_with_counts(data, x, x_bc))
    for sfx in ("", "_bcmatch"):
        p, z = summ["ppc_p_score" + sfx].cpu()[picked], summ["ppc_z_score" + sfx].cpu()[picked]
        assert bool((p == 2.0 / (S + 1)).all()), p
        assert bool((z > 0).all()), z


# ------------------------------------------------------------------ 7. CLI
def test_cli_survival_predictive(tmp_path, capsys):
    from bean_amd.cli.execute import main as bean_main

    base = ["survival", "variant", SURV, "--n-iter", "50", "--control-condition=D7"]
    d1 = _run(str(tmp_path / "ppc"), *base, "--survival-predictive", "20")
    d0 = _run(str(tmp_path / "plain"), *base)
    names = sorted(os.listdir(d0))
    assert "bean_element_result.MixtureNormal.csv" in names and "bean_sgRNA_result.MixtureNormal.csv" in names
    own = {"bean_predictive_guides.MixtureNormal.csv", "bean_predictive_samples.MixtureNormal.csv"}
    assert sorted(os.listdir(d1)) == sorted(set(names) | own) and not own & set(names)
    for name in names:  # every other output file is what it is without the flag
        assert open(f"{d1}/{name}", "rb").read() == open(f"{d0}/{name}", "rb").read(), name
    guides = pd.read_csv(f"{d1}/bean_predictive_guides.MixtureNormal.csv", index_col=0)
    sg = pd.read_csv(f"{d1}/bean_sgRNA_result.MixtureNormal.csv", index_col=0)
    cols = [c + s for s in ("", "_bcmatch") for c in ("ppc_p_score", "ppc_p_spread", "ppc_z_score")]
    assert list(guides.columns) == list(sg.columns) + cols and list(guides.index) == list(sg.index)
    p = guides["ppc_p_score"].dropna()
    assert len(p) and bool(((p >= 1 / 21) & (p <= 1)).all())
    samples = pd.read_csv(f"{d1}/bean_predictive_samples.MixtureNormal.csv", index_col=0)
    assert {"replicate", "condition", "masked", "frac_cells_p05", "mean_z", "frac_cells_p05_bcmatch", "mean_z_bcmatch",
            "n_draws"} <= set(samples.columns)
    assert len(samples) and bool((samples["n_draws"] == 20).all())
    with pytest.raises(SystemExit) as exc:
        bean_main(["run", "sorting", "variant", os.path.join(GOLD, "var_mini_screen.h5ad"), "--survival-predictive", "20",
                   "-o", str(tmp_path / "sorting")])
    assert exc.value.code == 2
    msg = " ".join(capsys.readouterr().err.split())
    assert "--survival-predictive" in msg and "sorting screens" in msg
