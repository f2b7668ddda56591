"""Depth study on the GPU: D x K replicate screens in one launch (bean_hip_simulate_design,
csrc/bean_predictive.hpp::k_simulate_design).  Depth 1 is the bootstrap's launch bit for bit; totals, monotonicity
across depths and batching; the law at another depth; the state the call must leave alone; its refusals;
run_inference_design batched, in several engine runs and in its fallback; and the CLI.  -m gpu."""
import copy
import ctypes
import pickle
from functools import partial

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.jackknife import design_summary
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

import design_common as dc
import dm_reference as dm
from members_common import (CONFIGS, DEV, VAR, _h5ad_reader_present, _kw_of, _mini, _run, _same_results,  # noqa: F401
                            _state, _without_columns)

pytestmark = pytest.mark.gpu
SEED = 101
FIRST, K = 7, 5
DEPTHS = (0.25, 1.0, 3.0)


# ------------------------------------------------------------------ screens and engines, built once per module
@pytest.fixture(scope="module")
def screens(tmp_path_factory):
    # 203 guides: four tiles, the last one partial; five conditions: the last gamma pair is a lone bin; masks present
    return {
        "203": make_sorting_variant_screen(203, 3, seed=11, mask_fraction=0.05, depth_per_guide=100.0),
        "203acc": make_sorting_variant_screen(203, 3, seed=11, mask_fraction=0.05, depth_per_guide=100.0,
                                              with_accessibility=True),
        "mini": _mini(tmp_path_factory.mktemp("mini")),  # 30 guides: one partial tile, the generic k_param
    }


@pytest.fixture(scope="module")
def engines(screens):
    from bean_amd import engine

    cache = {}

    def get(which, family, kw):
        key = (which, family, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in cache:
            data = screens[which]
            cache[key] = engine.HipSVI(family, data.to(DEV), num_steps=50, **_kw_of(kw, data))
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def _which(kw):
    return "203acc" if kw.get("scale_by_accessibility") else "203"


def _observed(eng):
    out = {"X": eng._keep["X"]}
    if eng.use_bcmatch:
        out["X_bcmatch"] = eng._keep["X_BC"]
    return out


def _site_noise(eng, seed):
    g = torch.Generator().manual_seed(seed)
    noise = {"eps_mu": torch.randn(eng.T, generator=g, dtype=torch.float64),
             "eps_sd": torch.randn(eng.T, generator=g, dtype=torch.float64)}
    if eng.scale_by_accessibility:
        noise["eps_noise"] = torch.randn(eng.data.n_guides, generator=g, dtype=torch.float64)
    return noise


def _totals(obs, depth):
    """floor(f n_obs + 0.5), float64 on the host, (R, G)."""
    n = obs.detach().cpu().double().sum(1).numpy()
    return torch.as_tensor(np.floor(float(depth) * n + 0.5))


# ------------------------------------------------------------------ 1. depth 1 is the bootstrap's launch
@pytest.mark.parametrize("family,kw", CONFIGS)
def test_depth_one_is_the_bootstraps_launch(engines, family, kw):
    eng = engines(_which(kw), family, kw)
    assert eng.predictive_supported
    R, B, G = eng.data.n_reps, eng.data.n_condits, eng.data.n_guides
    assert (R, B, G) == (3, 5, 203)
    keys = {"X", "X_bcmatch"} if eng.use_bcmatch else {"X"}
    for noise in (None, _site_noise(eng, 9)):
        eng.set_noise(noise)
        try:
            got = eng.simulate_design(FIRST, K, [1.0], seed=SEED)
            want = eng.simulate_members(FIRST, K, seed=SEED)
            torch.cuda.synchronize()
        finally:
            eng.set_noise(None)
        assert set(got) == set(want) == keys
        for key in keys:
            assert got[key].shape == (1, K, R, B, G) and got[key].dtype == torch.float32 and got[key].is_contiguous()
            assert torch.equal(got[key][0], want[key]), (key, noise is not None)


# ------------------------------------------------------------------ 2. planes and batching
def _check_planes(eng, k):
    obs = _observed(eng)
    a = eng.simulate_design(FIRST, k, DEPTHS, seed=SEED)
    members = eng.simulate_members(FIRST, k, seed=SEED)
    torch.cuda.synchronize()
    assert set(a) == set(obs)
    for key, x in a.items():
        assert x.shape == (len(DEPTHS), k) + tuple(obs[key].shape)
        assert torch.equal(x[1], members[key]), key  # (a)
        assert bool((x >= 0).all()) and bool((x == x.round()).all()), key
        for i, f in enumerate(DEPTHS):  # (c)
            want = _totals(obs[key], f).to(x.device)
            assert torch.equal(x[i].double().sum(2), want.expand(k, -1, -1)), (key, f)
        assert bool((x[0] <= x[1]).all()) and bool((x[1] <= x[2]).all()), key  # (b)
        assert not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2]), key
    again = eng.simulate_design(FIRST, k, DEPTHS, seed=SEED)
    alone = [eng.simulate_design(FIRST, k, [f], seed=SEED) for f in DEPTHS]
    order = [2, 0, 1]
    permuted = eng.simulate_design(FIRST, k, [DEPTHS[i] for i in order], seed=SEED)
    shifted = eng.simulate_design(FIRST + 1, k, DEPTHS, seed=SEED)
    other_seed = eng.simulate_design(FIRST, k, DEPTHS, seed=SEED + 1)
    torch.cuda.synchronize()
    eng.set_noise(_site_noise(eng, 3))  # with the shared sites injected, first_draw + 1 shifts j and nothing else
    try:
        here = eng.simulate_design(FIRST, k, DEPTHS, seed=SEED)
        there = eng.simulate_design(FIRST + 1, k, DEPTHS, seed=SEED)
        torch.cuda.synchronize()
    finally:
        eng.set_noise(None)
    for key in a:
        assert torch.equal(a[key], again[key]), key
        for i in range(len(DEPTHS)):
            assert torch.equal(alone[i][key][0], a[key][i]), (key, i)
            assert torch.equal(permuted[key][order.index(i)], a[key][i]), (key, i)
        assert torch.equal(there[key][:, :-1], here[key][:, 1:]), key
        assert not torch.equal(shifted[key], a[key]) and not torch.equal(other_seed[key], a[key]), key
    return a


@pytest.mark.parametrize("family,kw", [CONFIGS[0], CONFIGS[2], CONFIGS[3], CONFIGS[4]])
def test_planes_totals_and_batching(engines, family, kw):
    _check_planes(engines(_which(kw), family, kw), K)


@pytest.mark.parametrize("family,kw", [CONFIGS[0], CONFIGS[2]])
def test_planes_on_the_mini_screen(engines, family, kw):
    eng = engines("mini", family, kw)
    assert eng.predictive_supported and eng.data.n_guides == 30
    _check_planes(eng, 3)


def test_a_deep_pair_and_a_depth_that_rounds_to_nothing(screens):
    from bean_amd import engine

    data = copy.copy(screens["203"])
    deep = (1, 70)  # in the second tile of replicate 1
    for name in ("X", "X_masked", "X_bcmatch", "X_bcmatch_masked"):
        t = getattr(data, name).clone()
        t[deep[0], :, deep[1]] = 0
        t[deep[0], 2, deep[1]] = 5003
        setattr(data, name, t)
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
    obs = _observed(eng)
    n = obs["X"].double().sum(1)
    assert float(n[deep]) == 5003 and float(n.median()) < 1000
    out = eng.simulate_design(FIRST, 3, [0.5, 1.0, 2.0], seed=SEED)
    same = eng.simulate_members(FIRST, 3, seed=SEED)
    tiny = 0.4 / float(n.max())
    none = eng.simulate_design(FIRST, 3, [tiny], seed=SEED)
    torch.cuda.synchronize()
    for key, x in out.items():
        assert torch.equal(x[1], same[key]), key
        for i, f in enumerate((0.5, 1.0, 2.0)):
            want = _totals(obs[key], f).to(x.device)
            assert torch.equal(x[i].double().sum(2), want.expand(3, -1, -1)), (key, f)
        assert float(x[0].double().sum(2)[0][deep]) == 2502 and float(x[2].double().sum(2)[0][deep]) == 10006
        assert bool((x[0] <= x[1]).all()) and bool((x[1] <= x[2]).all()), key
        assert float(none[key].abs().sum()) == 0, key
    eng.close()


# ------------------------------------------------------------------ 3. the full grid
def test_sixty_four_members_in_one_call(engines):
    eng = engines("203", "MixtureNormal", {})
    obs = _observed(eng)
    depths = [0.5, 1.0, 1.5, 2.0, 0.75, 1.25, 3.0, 0.1]
    out = eng.simulate_design(0, 8, depths, seed=SEED)
    want = eng.simulate_members(0, 8, seed=SEED)
    torch.cuda.synchronize()
    for key, x in out.items():
        assert x.shape[:2] == (8, 8)
        assert torch.equal(x[1], want[key]), key
        for i, f in enumerate(depths):
            assert torch.equal(x[i].double().sum(2), _totals(obs[key], f).to(x.device).expand(8, -1, -1)), (key, f)
    for d, k in ((5, 13), (65, 1), (1, 65)):
        with pytest.raises(RuntimeError, match=rf"<= 64, got {d} x {k} = 65"):
            eng.simulate_design(0, k, [1.0 + 0.01 * i for i in range(d)], seed=SEED)
    assert torch.equal(eng.simulate_members(0, 8, seed=SEED)["X"], want["X"])


# ------------------------------------------------------------------ 4. the law at another depth
LABELS = []


def _law_engine(regime):
    """The regime of dm_reference.py as tests/test_gpu_simulator_law.py builds it: the Normal family, the latent sites
    fixed, the concentrations those the kernel itself exports."""
    from bean_amd import engine

    data = dm.regime_screen(regime)
    eng = engine.HipSVI("Normal", data.to(DEV), num_steps=50)
    assert eng.predictive_supported and eng.use_bcmatch
    for k in ("mu_scale", "sd_scale"):
        eng.unconstrained[k].fill_(-20.0)
    if regime != "sparse":
        g = torch.Generator().manual_seed(3)
        eng.unconstrained["mu_loc"].copy_(0.7 * torch.randn(eng.unconstrained["mu_loc"].shape, generator=g))
    return eng


@pytest.mark.parametrize("regime", ["moderate", "sparse"])
def test_the_law_at_another_depth(regime):
    eng = _law_engine(regime)
    alpha = eng.simulate(0, seed=SEED, alphas=True)["alpha"].cpu().numpy()
    n_obs = eng._keep["X"].double().sum(1).cpu().numpy().astype(np.int64)
    assert np.array_equal(n_obs, dm.regime_totals(regime)) and bool((n_obs % 2 == 1).any())
    for depth in dc.LAW_DEPTHS:
        x = eng.simulate_design(0, dc.LAW_DRAWS, [depth], seed=SEED)["X"][0].cpu().numpy()
        rep = dc.law_report(regime, depth, x, n_obs, alpha[0], np.random.default_rng(SEED))
        print(dc.describe(rep))
        LABELS.append(rep["name"])
        assert len(rep["p"]) == dc.N_PVALUES[rep["name"]]
        assert dc.failures(rep) == []
    eng.close()


def test_the_count_of_p_values():
    """The threshold was set for N_P p-values: the law tests of this file compute exactly those."""
    assert sorted(LABELS) == sorted(dc.N_PVALUES) and sum(dc.N_PVALUES[k] for k in LABELS) == dc.N_P == 95
    print(f"N_P = {dc.N_P}, threshold {dc.P_MIN:.3e}")


# ------------------------------------------------------------------ 5. state and refusals
def test_simulate_design_leaves_the_fit_alone(screens):
    from bean_amd import engine

    data = screens["203"].to(DEV)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(20, seed=SEED)
    torch.cuda.synchronize()
    before = _state(eng)
    grads = {k: v.clone() for k, v in eng.grads.items()}
    hist = eng.loss_hist.clone()
    eng.simulate_design(2, K, DEPTHS, seed=7)
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
            x = torch.empty((2, K) + tuple(e._keep["X"].shape), dtype=torch.float32, device=DEV)
            xbc = torch.empty_like(x)
            nb = x.numel() * 4
            two = (ctypes.c_double * 2)(0.5, 2.0)
            assert e.lib.bean_hip_simulate_design(e._h, SEED + 5, 1, K, two, 2, ctypes.c_void_p(x.data_ptr()), nb,
                                                  ctypes.c_void_p(xbc.data_ptr()), nb, e._sptr()) == 0
        elif simulate_first:
            e.simulate_design(1, K, [0.5, 2.0], seed=SEED + 5)
        e.run(40, seed=SEED, resume=resume)
        torch.cuda.synchronize()
        st = _state(e)
        e.close()
        return st

    plain, simulated = fit(False, False), fit(True, False)
    for k in plain:
        assert torch.equal(plain[k], simulated[k]), k
    plain = fit(False, True)
    for how in (True, "raw"):
        simulated = fit(how, True)
        for k in plain:
            assert torch.equal(plain[k], simulated[k]), (how, k)


def test_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["203"].to(DEV)
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    one = 4 * R * B * G
    x = torch.zeros(64 * R * B * G, dtype=torch.float32, device=DEV)
    xbc = torch.zeros(64 * R * B * G, dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    arr = lambda *f: (ctypes.c_double * len(f))(*f)  # noqa: E731
    D = 2
    two = arr(0.5, 2.0)
    full = D * K * one

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    before = eng.simulate_members(3, K, seed=SEED)
    sim = lambda k, f, d, *a: lib.bean_hip_simulate_design(eng._h, SEED, 0, k, f, d, *a, eng._sptr())  # noqa: E731
    assert lib.bean_hip_simulate_design(None, SEED, 0, K, two, D, p(x), full, None, 0, None) < 0 and "null handle" in err()
    assert sim(K, None, D, p(x), full, p(xbc), full) < 0 and "depths is null" in err()
    for k, d in ((0, 2), (-1, 2), (5, 0), (5, -1), (13, 5), (65, 1)):
        assert sim(k, arr(*[1.0 + i for i in range(max(d, 1))]), d, p(x), full, p(xbc), full) < 0
        assert "<= 64" in err() and f"got {d} x {k} = {d * k}" in err(), err()
    for i, bad in ((1, 0.0), (0, -1.0), (1, float("nan")), (0, float("inf")), (1, float("-inf"))):
        f = [0.5, 2.0]
        f[i] = bad
        assert sim(K, arr(*f), D, p(x), full, p(xbc), full) < 0
        assert f"depths[{i}] = " in err() and "finite factor > 0" in err(), err()
        assert ("nan" in err().lower()) if bad != bad else (("inf" in err().lower()) if abs(bad) == float("inf") else True)
    assert sim(K, two, D, p(x), full - 4, p(xbc), full) < 0 and "x_out" in err() and "D = 2, K = 5" in err()
    assert sim(K, two, D, p(x), K * one, p(xbc), full) < 0 and "x_out" in err() and "D = 2, K = 5" in err()
    assert sim(K, two, D, None, 0, p(xbc), full) < 0 and "x_out" in err()
    assert sim(K, two, D, p(x), full, p(xbc), full + one) < 0 and "xbc_out" in err() and "D = 2, K = 5" in err()
    assert sim(K, two, D, p(x), full, None, 0) < 0 and "xbc_out" in err()
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0 and float(xbc.abs().sum()) == 0  # nothing was launched
    after = eng.simulate_members(3, K, seed=SEED)  # the handle is as usable as before the refused calls
    for key in before:
        assert torch.equal(before[key], after[key]), key
    assert sim(K, two, D, p(x), full, p(xbc), full) == 0
    torch.cuda.synchronize()
    n = eng._keep["X"].double().sum(1)
    assert float(x.double().sum()) == K * float((torch.floor(0.5 * n + 0.5) + torch.floor(2.0 * n + 0.5)).sum())
    assert set(eng.simulate_design(0, 2, [0.5])) == {"X", "X_bcmatch"}
    eng.close()

    nobc = engine.HipSVI("MixtureNormal", data, num_steps=50, use_bcmatch=False)
    assert lib.bean_hip_simulate_design(nobc._h, SEED, 0, K, two, D, p(x), full, p(xbc), full, nobc._sptr()) < 0
    assert "xbc_out" in err() and "BEAN_FLAG_USE_BCMATCH" in err()
    assert set(nobc.simulate_design(0, K, [0.5, 2.0])) == {"X"}
    h = ctypes.c_void_p()  # an unprepared handle of the same shape
    assert lib.bean_hip_create(ctypes.byref(nobc._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_predictive_supported(h) == 1
    assert lib.bean_hip_simulate_design(h, SEED, 0, K, two, D, p(x), full, None, 0, None) < 0 and "bean_hip_prepare" in err()
    assert lib.bean_hip_destroy(h) == 0
    nobc.close()

    for extra in (dict(n_members=2), dict(n_particles=2)):
        many = engine.HipSVI("MixtureNormal", data, num_steps=50, **extra)
        assert lib.bean_hip_simulate_design(many._h, SEED, 0, K, two, D, p(x), full, p(xbc), full, many._sptr()) < 0
        assert "bean_hip_predictive_supported" in err()
        with pytest.raises(PredictiveUnsupported):
            many.simulate_design(0, K, [0.5, 2.0])
        many.close()

    for other in (engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10)):
        assert lib.bean_hip_simulate_design(other._h, SEED, 0, K, two, D, p(x), full, None, 0, other._sptr()) < 0
        assert "bean_hip_predictive_supported" in err()
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.simulate_design(0, K, [0.5, 2.0])
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()


def test_a_depth_that_reaches_the_categorical_window_is_refused(screens):
    from bean_amd import engine

    data = copy.copy(screens["203"])
    for name in ("X_bcmatch", "X_bcmatch_masked"):  # the barcode-matched counts alone hold the deep pair
        t = getattr(data, name).clone()
        t[2, :, 150] = 0
        t[2, 1, 150] = 5_000_000
        setattr(data, name, t)
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
    x = eng.simulate_members(0, 2, seed=SEED)["X"].clone()
    with pytest.raises(ValueError, match=r"depth 4 times the largest observed total 5000000 is 20000000 reads.*2\^24 = 16777216"):
        eng.simulate_design(0, 2, [0.5, 4.0], seed=SEED)
    assert torch.equal(eng.simulate_members(0, 2, seed=SEED)["X"], x)
    eng.close()
    nobc = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50, use_bcmatch=False)  # X alone: nothing deep
    out = nobc.simulate_design(0, 2, [0.5, 4.0], seed=SEED)
    torch.cuda.synchronize()
    assert out["X"].shape[:2] == (2, 2)
    nobc.close()


# ------------------------------------------------------------------ 6. run_inference_design
RUN_DEPTHS, N_SCREENS, STEPS, DESIGN_SEED = (0.1, 1.0, 4.0), 6, 300, 55


def _models():
    from bean_amd.model import model as m

    return partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)


@pytest.fixture(scope="module")
def design(screens, tmp_path_factory):
    """run_inference_design with its defaults, once."""
    import os

    from bean_amd.model.run import run_inference_design

    mod, gd = _models()
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("fit"))
    try:
        return run_inference_design(mod, gd, screens["203"], RUN_DEPTHS, n_screens=N_SCREENS, seed=7,
                                    design_seed=DESIGN_SEED, num_steps=STEPS, verbose=False)
    finally:
        os.chdir(cwd)


def test_run_inference_design_is_the_single_fits(screens, design, tmp_path, monkeypatch):
    """full, the depth-1 row (the bootstrap's boots), single screens, several engine runs - bit for bit - and the
    direction of the spread: the median over targets of mu_design_se at depth 0.1 exceeds that at depth 4.

    The direction on the host, before any device run (oracle CPU fits, 203 x 3, 300 steps, K = 6, one seed for all fits,
    screens from dm_reference.host_dm at floor(f n + 0.5), medians of sd_j(mu_loc) at depth 0.1 / depth 4):
      * concentrations with the a0 the screen carries and the study conditions on (fitted a0, median 162):
        0.132 / 0.067, ratio 1.98, 90 % of the targets in that direction; the likelihood's own prediction
        sqrt of (n + a0) / (n (a0 + 1)) at the median totals is 2.03;
      * concentrations with the generator's TRUE a0 (median 28, a sixth of the fitted one): 0.177 / 0.160, ratio 1.11
        (prediction 1.25) - no clear margin, and a lower depth_per_guide does not give one (20: 1.04), because the
        generator's a0 grows as n^0.79: there the spread IS the dispersion's.
    The study draws from the first, so depth_per_guide stays at the fixtures' 100.  On the device: 0.105 / 0.057."""
    from bean_amd import engine
    from bean_amd.model import run as model_run

    monkeypatch.chdir(tmp_path)
    mod, gd = _models()
    data = screens["203"]
    full, fits = design
    assert len(fits) == 3 and all(len(row) == N_SCREENS for row in fits)
    want_full = model_run.run_inference(mod, gd, data, num_steps=STEPS, seed=7, verbose=False)
    _same_results(full, want_full)
    boot_full, boots = model_run.run_inference_bootstrap(mod, gd, data, n_boot=N_SCREENS, seed=7, boot_seed=DESIGN_SEED,
                                                         num_steps=STEPS, verbose=False)
    _same_results(boot_full, full)
    for a, b in zip(fits[1], boots):
        _same_results(a, b)
    # one screen at depth 0.1 and one at depth 4: planes of one simulate_design call on an engine prepared the same way
    eng = model_run.bootstrap_engine(mod, gd, data, want_full[0])
    try:
        sim = {k: v.cpu() for k, v in eng.simulate_design(0, N_SCREENS, RUN_DEPTHS, seed=DESIGN_SEED).items()}
    finally:
        eng.close()
    for i, j in ((0, 2), (2, 5)):
        redrawn = copy.copy(data)
        redrawn.X_masked = sim["X"][i, j].to(data.X_masked.dtype)
        redrawn.X_bcmatch_masked = sim["X_bcmatch"][i, j].to(data.X_bcmatch_masked.dtype)
        _same_results(fits[i][j], model_run.run_inference(mod, gd, redrawn, num_steps=STEPS, seed=7, verbose=False))
    # several engine runs: five screens next to the screen each
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble",
                        lambda self, *a, **k: (used.append(self.n_members), real(self, *a, **k))[1])
    parts = model_run.run_inference_design(mod, gd, data, RUN_DEPTHS, n_screens=N_SCREENS, seed=7,
                                           design_seed=DESIGN_SEED, num_steps=STEPS, verbose=False, max_per_run=5)
    assert used == [6] * 9 + [4] * 3, used  # 18 screens: 5 + 5 + 5 + 3, three report windows each
    _same_results(parts[0], full)
    for row, want in zip(parts[1], fits):
        for a, b in zip(row, want):
            _same_results(a, b)
    # depth 1 put in front where it is absent
    summary = design_summary(full, fits, RUN_DEPTHS, data=data)
    assert summary["n_screens"] == N_SCREENS and summary["mu_design_se"].shape == (3, data.n_targets)
    assert bool(torch.isfinite(summary["mu_design_se"]).all()) and float(summary["se_ratio"][1]) == 1.0
    shallow, base, deep = (float(torch.quantile(summary["mu_design_se"][i], 0.5)) for i in range(3))
    print(f"median mu_design_se at depths {RUN_DEPTHS}: {shallow:.5f} {base:.5f} {deep:.5f}; se_ratio "
          f"{summary['se_ratio'].tolist()}; recovery {summary['recovery'].tolist()}; n_hits {summary['n_hits']}; "
          f"median_total {summary['median_total'].tolist()}")
    assert shallow > deep  # direction only: fewer reads, wider spread


def test_run_inference_design_fallback(screens, design, tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import run as model_run

    monkeypatch.chdir(tmp_path)
    mod, gd = _models()
    data = screens["203"]
    full, fits = design
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble", lambda self, *a, **k: (used.append(1), real(self, *a, **k))[1])
    monkeypatch.setattr(engine.HipSVI, "ensemble_supported", property(lambda self: False))
    serial = model_run.run_inference_design(mod, gd, data, [0.1, 4.0], n_screens=2, seed=7, design_seed=DESIGN_SEED,
                                            num_steps=STEPS, verbose=False)  # (depth 1 is put in front)
    assert used == []
    _same_results(serial[0], full)
    assert len(serial[1]) == 3
    for row, want in zip(serial[1], (fits[1], fits[0], fits[2])):
        for a, b in zip(row, want[:2]):
            _same_results(a, b)


# ------------------------------------------------------------------ 7. CLI
def test_cli_design(tmp_path):
    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    dd = _run(str(tmp_path / "design"), *base, "--design-depths", "0.5,2", "--design-screens", "3", "--save-raw")
    d0 = _run(str(tmp_path / "plain"), *base)
    name_el, name_sg = "bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"
    plain_el, plain_sg = open(f"{d0}/{name_el}", "rb").read(), open(f"{d0}/{name_sg}", "rb").read()
    assert open(f"{dd}/{name_sg}", "rb").read() == plain_sg
    columns = ["mu_design_se_x1", "mu_design_se_x0.5", "mu_design_se_x2"]
    assert _without_columns(f"{dd}/{name_el}", columns) == plain_el
    el, plain = pd.read_csv(f"{dd}/{name_el}"), pd.read_csv(f"{d0}/{name_el}")
    assert [c for c in el.columns if c not in plain.columns] == columns
    assert len(el) == 6 and np.isfinite(el[columns].values.astype(float)).all() and (el[columns] > 0).all().all()
    import os

    assert not os.path.exists(f"{d0}/bean_design.MixtureNormal.csv")
    table = pd.read_csv(f"{dd}/bean_design.MixtureNormal.csv")
    assert list(table.columns) == ["depth", "n_screens", "median_total", "median_mu_design_se", "se_ratio", "recovery", "n_hits"]
    assert table["depth"].tolist() == [1.0, 0.5, 2.0] and (table["n_screens"] == 3).all()
    assert table["se_ratio"][0] == 1.0 and np.isfinite(table["median_total"]).all()
    assert table["median_total"][1] < table["median_total"][0] < table["median_total"][2]
    np.testing.assert_allclose(table["median_mu_design_se"], np.median(el[columns].values, axis=0), rtol=1e-12)
    with open(f"{dd}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    entries = raw["design"]
    assert [(e["depth"], e["screen"]) for e in entries] == [(f, j) for f in (1.0, 0.5, 2.0) for j in range(3)]
    assert all(set(e) == {"depth", "screen", "params", "loss"} and len(e["loss"]) == 200 for e in entries)
    again = design_summary(raw["params"], [[e["params"] for e in entries[3 * i:3 * i + 3]] for i in range(3)], [1.0, 0.5, 2.0])
    np.testing.assert_allclose(sorted(again["mu_design_se"][1].tolist()), sorted(el["mu_design_se_x0.5"]), rtol=1e-12)
    # a tiling screen is refused with the family named
    import contextlib
    import io

    from bean_amd.cli.execute import main

    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(["run", "sorting", "tiling", VAR, "--design-depths", "0.5,2", "-o", str(tmp_path / "tiling")])
    assert exc.value.code == 2
    assert ("--design-depths simulates the counts of the sorting variant models (Normal, MixtureNormal) and is not "
            "available for tiling screens (MultiMixtureNormal).") in " ".join(err.getvalue().split())
