"""Power study on the GPU: D x K replicate screens with planted effects in one launch (bean_hip_simulate_power,
csrc/bean_predictive.hpp::k_simulate_power).  Nothing planted is the bootstrap's launch bit for bit; a planted effect is
the launch of a twin engine whose mu_loc is the effect; totals and batching; the state the call must leave alone; its
refusals; run_inference_power batched, in several engine runs and in its fallback; and the CLI.  -m gpu."""
import copy
import ctypes
import os
import pickle
from functools import partial

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.jackknife import power_summary
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

import dm_reference as dm
from members_common import (CONFIGS, DEV, VAR, _h5ad_reader_present, _kw_of, _mini, _run, _same_results,  # noqa: F401
                            _state, _without_columns)

pytestmark = pytest.mark.gpu
SEED = 101
FIRST, K = 7, 5
# (0.1 is not a float32: the twin's mu_loc holds float32(0.1), and that value is what is planted)
EFFECTS = (0.0, 0.25, -0.75, float(np.float32(0.1)))


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


def _engine_cache(screens, steps):
    from bean_amd import engine

    cache = {}

    def get(which, family, kw):
        key = (which, family, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in cache:
            data = screens[which]
            cache[key] = engine.HipSVI(family, data.to(DEV), num_steps=50, **_kw_of(kw, data))
            if steps:
                cache[key].run(steps, seed=SEED)  # the tables are not the initial ones
                torch.cuda.synchronize()
        return cache[key]

    return cache, get


@pytest.fixture(scope="module")
def engines(screens):
    cache, get = _engine_cache(screens, 50)
    yield get
    for eng in cache.values():
        eng.close()


@pytest.fixture(scope="module")
def twins(screens):
    """A second engine per configuration: it takes the first one's state and, on the planted targets, the effect."""
    cache, get = _engine_cache(screens, 0)
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


def _site_noise(eng, seed, eps_mu=True, eps_sd=True):
    g = torch.Generator().manual_seed(seed)
    draw = lambda n, on: torch.randn(n, generator=g, dtype=torch.float64) * (1.0 if on else 0.0)  # noqa: E731
    noise = {"eps_mu": draw(eng.T, eps_mu), "eps_sd": draw(eng.T, eps_sd)}
    if eng.scale_by_accessibility:
        noise["eps_noise"] = torch.randn(eng.data.n_guides, generator=g, dtype=torch.float64)
    return noise


def _guide_targets(data):
    """(G,) the target of every guide."""
    return torch.repeat_interleave(torch.arange(int(data.n_targets)), data.target_lengths.cpu())


def _copy_state(src, dst):
    for k, v in src.unconstrained.items():
        dst.unconstrained[k].copy_(v)
    for name in ("_m", "_v"):
        for k, v in getattr(src, name).items():
            getattr(dst, name)[k].copy_(v)


# ------------------------------------------------------------------ 1. nothing planted: the bootstrap's launch
@pytest.mark.parametrize("family,kw", CONFIGS)
def test_nothing_planted_is_the_bootstraps_launch(engines, family, kw):
    eng = engines(_which(kw), family, kw)
    assert eng.predictive_supported
    R, B, G = eng.data.n_reps, eng.data.n_condits, eng.data.n_guides
    assert (R, B, G) == (3, 5, 203)
    keys = {"X", "X_bcmatch"} if eng.use_bcmatch else {"X"}
    nothing = torch.zeros(eng.T, dtype=torch.bool)
    for noise in (None, _site_noise(eng, 9)):
        eng.set_noise(noise)
        try:
            got = eng.simulate_power(FIRST, K, EFFECTS, plant=nothing, seed=SEED)
            want = eng.simulate_members(FIRST, K, seed=SEED)
            torch.cuda.synchronize()
        finally:
            eng.set_noise(None)
        assert set(got) == set(want) == keys
        for key in keys:
            assert got[key].shape == (len(EFFECTS), K, R, B, G) and got[key].dtype == torch.float32
            assert got[key].is_contiguous()
            for i in range(len(EFFECTS)):
                assert torch.equal(got[key][i], want[key]), (key, i, noise is not None)


# ------------------------------------------------------------------ 2. the twin
def _check_twin(eng, twin, k, effects=EFFECTS):
    """Plane (i, j) of simulate_power is plane j of simulate_members on the twin: the same state, mu_loc = effects[i] on
    the planted targets, eps_mu = 0.  Every target planted, then every other one (the unplanted lanes are the
    bootstrap's, in every plane)."""
    T = eng.T
    _copy_state(eng, twin)
    fitted = eng.unconstrained["mu_loc"].clone()
    g2t = _guide_targets(eng.data).to(DEV)
    every_other = torch.arange(T) % 2 == 0
    try:
        for eps_sd in (False, True):
            noise = _site_noise(eng, 4, eps_mu=False, eps_sd=eps_sd)
            assert float(noise["eps_mu"].abs().sum()) == 0 and bool(noise["eps_sd"].abs().sum() > 0) == eps_sd
            eng.set_noise(noise)
            twin.set_noise(noise)
            boot = eng.simulate_members(FIRST, k, seed=SEED)
            for plant in (None, every_other):
                got = eng.simulate_power(FIRST, k, effects, plant=plant, seed=SEED)
                sel = torch.ones(T, dtype=torch.bool) if plant is None else plant
                moved = False
                for i, e in enumerate(effects):
                    mu = fitted.clone()
                    mu[sel.to(mu.device)] = e
                    twin.unconstrained["mu_loc"].copy_(mu)
                    want = twin.simulate_members(FIRST, k, seed=SEED)
                    torch.cuda.synchronize()
                    assert set(got) == set(want)
                    for key in want:
                        assert torch.equal(got[key][i], want[key]), (key, e, eps_sd, plant is None)  # (b)
                        assert torch.equal(got[key][i].double().sum(2), boot[key].double().sum(2)), key  # (c)
                        moved |= not torch.equal(got[key][i], boot[key])
                        if plant is not None:  # (d)
                            rest = ~sel.to(DEV)[g2t]
                            assert bool(rest.any()) and not bool(rest.all())
                            assert torch.equal(got[key][i][..., rest], boot[key][..., rest]), (key, e)
                assert moved  # the planted planes are not the bootstrap's
    finally:
        eng.set_noise(None)
        twin.set_noise(None)
        twin.unconstrained["mu_loc"].copy_(fitted)


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_a_planted_effect_is_the_twins_launch(engines, twins, family, kw):
    _check_twin(engines(_which(kw), family, kw), twins(_which(kw), family, kw), K)


@pytest.mark.parametrize("family,kw", [CONFIGS[0], CONFIGS[2]])
def test_the_twin_on_the_mini_screen(engines, twins, family, kw):
    eng = engines("mini", family, kw)
    assert eng.predictive_supported and eng.data.n_guides == 30
    _check_twin(eng, twins("mini", family, kw), 3)


def test_the_twin_where_pairs_are_normalised_in_logs():
    """Concentrations below 0.01 in every bin: pairs whose gammas all underflow form their concentrations again, from
    the table - there, too, a planted lane must take its own entry."""
    from bean_amd import engine

    data = dm.regime_screen("near-floor")
    eng, twin = (engine.HipSVI("Normal", data.to(DEV), num_steps=50) for _ in range(2))
    assert eng.predictive_supported and eng.use_bcmatch
    for e in (eng, twin):
        for k in ("mu_scale", "sd_scale"):
            e.unconstrained[k].fill_(-20.0)
    effects = (0.0, 0.75, -0.5)
    zeros = {"eps_mu": torch.zeros(eng.T, dtype=torch.float64), "eps_sd": torch.zeros(eng.T, dtype=torch.float64)}
    eng.set_noise(zeros)
    twin.set_noise(zeros)
    draws = 64
    got = eng.simulate_power(0, draws // 4, effects, seed=SEED)
    boot = eng.simulate_members(0, draws // 4, seed=SEED)
    differs = 0
    for i, e in enumerate(effects):
        twin.unconstrained["mu_loc"].fill_(e)
        alpha = twin.simulate(0, seed=SEED, alphas=True)["alpha"]
        assert float(alpha[0].max()) < 0.01
        want = twin.simulate_members(0, draws // 4, seed=SEED)
        torch.cuda.synchronize()
        for key in want:
            assert torch.equal(got[key][i], want[key]), (key, e)
            differs += int(not torch.equal(got[key][i], boot[key]))
    assert differs > 0
    eng.close()
    twin.close()


# ------------------------------------------------------------------ 3. planes and batching
def _check_planes(eng, k):
    obs = _observed(eng)
    a = eng.simulate_power(FIRST, k, EFFECTS, seed=SEED)
    torch.cuda.synchronize()
    assert set(a) == set(obs)
    for key, x in a.items():
        assert x.shape == (len(EFFECTS), k) + tuple(obs[key].shape) and x.dtype == torch.float32 and x.is_contiguous()
        assert bool((x >= 0).all()) and bool((x == x.round()).all()), key
        want = obs[key].double().sum(1)  # (c): every pair keeps its observed total
        assert torch.equal(x.double().sum(3), want.expand(len(EFFECTS), k, -1, -1)), key
        assert not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2]), key
    again = eng.simulate_power(FIRST, k, EFFECTS, seed=SEED)
    alone = [eng.simulate_power(FIRST, k, [e], seed=SEED) for e in EFFECTS]
    order = [2, 0, 3, 1]
    permuted = eng.simulate_power(FIRST, k, [EFFECTS[i] for i in order], seed=SEED)
    shifted = eng.simulate_power(FIRST + 1, k, EFFECTS, seed=SEED)
    other_seed = eng.simulate_power(FIRST, k, EFFECTS, seed=SEED + 1)
    # the mask as booleans, as uint8 and as a numpy array: one mask
    sel = torch.arange(eng.T) % 3 == 0
    masks = [eng.simulate_power(FIRST, k, EFFECTS, plant=m, seed=SEED)
             for m in (sel, sel.to(torch.uint8) * 7, sel.numpy(), sel.to(DEV))]
    torch.cuda.synchronize()
    eng.set_noise(_site_noise(eng, 3))  # with the shared sites injected, first_draw + 1 shifts j and nothing else
    try:
        here = eng.simulate_power(FIRST, k, EFFECTS, seed=SEED)
        there = eng.simulate_power(FIRST + 1, k, EFFECTS, seed=SEED)
        torch.cuda.synchronize()
    finally:
        eng.set_noise(None)
    for key in a:
        assert torch.equal(a[key], again[key]), key
        for i in range(len(EFFECTS)):
            assert torch.equal(alone[i][key][0], a[key][i]), (key, i)
            assert torch.equal(permuted[key][order.index(i)], a[key][i]), (key, i)
        assert torch.equal(there[key][:, :-1], here[key][:, 1:]), key
        assert not torch.equal(shifted[key], a[key]) and not torch.equal(other_seed[key], a[key]), key
        for other in masks[1:]:
            assert torch.equal(other[key], masks[0][key]), key
        assert not torch.equal(masks[0][key], a[key]), key
    for bad in (torch.zeros(eng.T + 1, dtype=torch.bool), torch.zeros(eng.T - 1, dtype=torch.uint8), np.zeros(0, dtype=bool),
                torch.zeros((eng.T, 1), dtype=torch.bool)):
        with pytest.raises(ValueError, match="plant"):
            eng.simulate_power(FIRST, k, EFFECTS, plant=bad, seed=SEED)
    return a


@pytest.mark.parametrize("family,kw", [CONFIGS[0], CONFIGS[2], CONFIGS[3], CONFIGS[4]])
def test_planes_totals_and_batching(engines, family, kw):
    _check_planes(engines(_which(kw), family, kw), K)


def test_sixty_four_members_in_one_call(engines):
    eng = engines("203", "MixtureNormal", {})
    obs = _observed(eng)
    effects = [0.0, 0.5, -0.5, 1.0, -1.0, 2.0, 0.125, -3.0]
    out = eng.simulate_power(0, 8, effects, seed=SEED)
    few = eng.simulate_power(0, 8, effects[2:5], seed=SEED)
    torch.cuda.synchronize()
    for key, x in out.items():
        assert x.shape[:2] == (8, 8)
        assert torch.equal(x.double().sum(3), obs[key].double().sum(1).expand(8, 8, -1, -1)), key
        assert torch.equal(x[2:5], few[key]), key
    for d, k in ((5, 13), (65, 1), (1, 65)):
        with pytest.raises(RuntimeError, match=rf"<= 64, got {d} x {k} = 65"):
            eng.simulate_power(0, k, [0.01 * i for i in range(d)], seed=SEED)
    assert torch.equal(eng.simulate_power(0, 8, effects[2:5], seed=SEED)["X"], few["X"])


def test_power_screens_batches_over_effects_and_draws(engines, monkeypatch):
    """power_screens: D_c * K <= 64 per call, and over j beyond 64 screens - the planes of the single calls."""
    from bean_amd import _lib as lib_mod
    from bean_amd.model import run as model_run

    eng = engines("mini", "MixtureNormal", {})
    effects = [0.0, 0.5, -1.0]
    whole = eng.simulate_power(0, 6, effects, seed=SEED)
    calls = []
    real = type(eng).simulate_power
    monkeypatch.setattr(type(eng), "simulate_power",
                        lambda self, first, k, es, **kw: (calls.append((first, k, list(es))), real(self, first, k, es, **kw))[1])
    monkeypatch.setattr(lib_mod, "MAX_MEMBERS", 8)
    x, xbc = model_run.power_screens(eng, effects, 6, SEED)  # 8 // 6 = 1 effect per call
    assert calls == [(0, 6, [e]) for e in effects]
    assert torch.equal(x, whole["X"]) and torch.equal(xbc, whole["X_bcmatch"])
    del calls[:]
    monkeypatch.setattr(lib_mod, "MAX_MEMBERS", 4)
    x, xbc = model_run.power_screens(eng, effects, 6, SEED)  # over j: draws 0 .. 3, then 4 .. 5
    assert calls == [(0, 4, [e]) for e in effects] + [(4, 2, effects[:2]), (4, 2, effects[2:])]
    assert x.shape[:2] == (3, 6)
    # (with nothing injected the shared Normal sites are those of a call's first draw: the first chunk is the call's own)
    assert torch.equal(x[:, :4], whole["X"][:, :4]) and torch.equal(xbc[:, :4], whole["X_bcmatch"][:, :4])


# ------------------------------------------------------------------ 4. state
def test_simulate_power_leaves_the_fit_alone(screens):
    from bean_amd import engine

    data = screens["203"].to(DEV)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(20, seed=SEED)
    torch.cuda.synchronize()
    before = _state(eng)
    grads = {k: v.clone() for k, v in eng.grads.items()}
    hist = eng.loss_hist.clone()
    eng.simulate_power(2, K, EFFECTS, seed=7)
    eng.simulate_power(2, K, EFFECTS, plant=torch.arange(eng.T) % 2 == 0, seed=7)
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
            two = (ctypes.c_double * 2)(0.5, -2.0)
            assert e.lib.bean_hip_simulate_power(e._h, SEED + 5, 1, K, two, 2, None, ctypes.c_void_p(x.data_ptr()), nb,
                                                 ctypes.c_void_p(xbc.data_ptr()), nb, e._sptr()) == 0
        elif simulate_first:
            e.simulate_power(1, K, [0.5, -2.0], seed=SEED + 5)
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


# ------------------------------------------------------------------ 5. refusals
def _with_covariates(n_guides, n_reps, n_cov, seed):
    data = make_sorting_variant_screen(n_guides, n_reps, seed=seed, mask_fraction=0.05)
    g = torch.Generator().manual_seed(seed)
    data.sample_covariates = [f"cov{i}" for i in range(n_cov)]
    data.n_sample_covariates = n_cov
    data.rep_by_cov = torch.randint(0, 2, (n_reps, n_cov), generator=g)
    data.rep_by_cov[0, 0], data.rep_by_cov[-1, 0] = 1, 0
    return data


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
    two = arr(0.5, -2.0)
    full = D * K * one
    NAME = "bean_hip_simulate_power: "

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    before = eng.simulate_members(3, K, seed=SEED)
    sim = lambda k, f, d, *a: lib.bean_hip_simulate_power(eng._h, SEED, 0, k, f, d, None, *a, eng._sptr())  # noqa: E731
    assert lib.bean_hip_simulate_power(None, SEED, 0, K, two, D, None, p(x), full, None, 0, None) < 0
    assert err() == NAME + "null handle"
    assert sim(K, None, D, p(x), full, p(xbc), full) < 0 and err() == NAME + "effects is null"
    for k, d in ((0, 2), (-1, 2), (5, 0), (5, -1), (13, 5), (65, 1)):
        assert sim(k, arr(*[1.0 + i for i in range(max(d, 1))]), d, p(x), full, p(xbc), full) < 0
        assert err().startswith(NAME) and "<= 64" in err() and f"got {d} x {k} = {d * k}" in err(), err()
    for i, bad in ((1, float("nan")), (0, float("inf")), (1, float("-inf"))):
        f = [0.5, -2.0]
        f[i] = bad
        assert sim(K, arr(*f), D, p(x), full, p(xbc), full) < 0
        assert err().startswith(NAME) and f"effects[{i}] = " in err() and "is not a finite number" in err(), err()
        assert ("nan" in err().lower()) if bad != bad else ("inf" in err().lower())
    assert sim(K, two, D, p(x), full - 4, p(xbc), full) < 0 and "x_out" in err() and "D = 2, K = 5" in err()
    assert sim(K, two, D, p(x), K * one, p(xbc), full) < 0 and "x_out" in err() and "D = 2, K = 5" in err()
    assert sim(K, two, D, None, 0, p(xbc), full) < 0 and "x_out" in err() and err().startswith(NAME)
    assert sim(K, two, D, p(x), full, p(xbc), full + one) < 0 and "xbc_out" in err() and "D = 2, K = 5" in err()
    assert sim(K, two, D, p(x), full, None, 0) < 0 and "xbc_out" in err() and err().startswith(NAME)
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0 and float(xbc.abs().sum()) == 0  # nothing was launched
    after = eng.simulate_members(3, K, seed=SEED)  # the handle is as usable as before the refused calls
    for key in before:
        assert torch.equal(before[key], after[key]), key
    assert sim(K, two, D, p(x), full, p(xbc), full) == 0
    torch.cuda.synchronize()
    assert float(x.double().sum()) == D * K * float(eng._keep["X"].double().sum())
    assert set(eng.simulate_power(0, 2, [0.5])) == {"X", "X_bcmatch"}
    eng.close()

    nobc = engine.HipSVI("MixtureNormal", data, num_steps=50, use_bcmatch=False)
    assert lib.bean_hip_simulate_power(nobc._h, SEED, 0, K, two, D, None, p(x), full, p(xbc), full, nobc._sptr()) < 0
    assert "xbc_out" in err() and "BEAN_FLAG_USE_BCMATCH" in err() and err().startswith(NAME)
    assert set(nobc.simulate_power(0, K, [0.5, -2.0])) == {"X"}
    h = ctypes.c_void_p()  # an unprepared handle of the same shape
    assert lib.bean_hip_create(ctypes.byref(nobc._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_predictive_supported(h) == 1
    assert lib.bean_hip_simulate_power(h, SEED, 0, K, two, D, None, p(x), full, None, 0, None) < 0
    assert err() == NAME + "call bean_hip_prepare first"
    assert lib.bean_hip_destroy(h) == 0
    nobc.close()

    for extra in (dict(n_members=2), dict(n_particles=2)):
        many = engine.HipSVI("MixtureNormal", data, num_steps=50, **extra)
        assert lib.bean_hip_simulate_power(many._h, SEED, 0, K, two, D, None, p(x), full, p(xbc), full, many._sptr()) < 0
        assert "bean_hip_predictive_supported" in err() and err().startswith(NAME)
        with pytest.raises(PredictiveUnsupported):
            many.simulate_power(0, K, [0.5, -2.0])
        many.close()

    neg = make_sorting_variant_screen(900, 3, seed=32)
    neg = neg[neg.negctrl_guide_idx]
    for other in (engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("ControlNormal", neg.to(DEV), num_steps=10),
                  engine.HipSVI("Normal", _with_covariates(200, 3, 2, seed=23).to(DEV), num_steps=10)):
        assert lib.bean_hip_simulate_power(other._h, SEED, 0, K, two, D, None, p(x), full, None, 0, other._sptr()) < 0
        assert "bean_hip_predictive_supported" in err() and err().startswith(NAME)
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.simulate_power(0, K, [0.5, -2.0])
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()


# ------------------------------------------------------------------ 6. run_inference_power
# The planted effect comes from the host check (scripts/oracle_power_direction.py): the smallest
# candidate; no candidate showed a margin in the detection rate at 300 steps, so the sign of the mean mu_loc is asserted.
RUN_EFFECTS, N_SCREENS, STEPS, POWER_SEED = (0.0, 1.0), 4, 300, 55


def _models():
    from bean_amd.model import model as m

    return partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)


@pytest.fixture(scope="module")
def power(screens, tmp_path_factory):
    """run_inference_power, once: the screen and its 8 screens in one engine run."""
    from bean_amd.model.run import run_inference_power

    mod, gd = _models()
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("fit"))
    try:
        return run_inference_power(mod, gd, screens["203"], RUN_EFFECTS[1:], n_screens=N_SCREENS, seed=7,
                                   power_seed=POWER_SEED, num_steps=STEPS, verbose=False)
    finally:
        os.chdir(cwd)


def test_run_inference_power_is_the_single_fits(screens, power, tmp_path, monkeypatch):
    """full and every fits[i][j] are run_inference's, bit for bit - in one engine run, and with three screens next to
    the screen per run - and the direction: the mean mu_loc over the planted targets has the planted effect's sign.

    The direction on the host, before any device run (scripts/oracle_power_direction.py: oracle CPU fits, 203 x 3, 300
    steps, K = 4, screens from dm_reference.host_dm with mu_t = e on every target; detection rate over (target, screen) |
    mean mu_loc | median |z| | median mu_scale):
      * effect 0:   0.000 | -0.028 | 0.111 | 0.394
      * effect 1:   0.000 | +0.622 | 1.089 | 0.573
      * effect 1.5: 0.000 | +0.782 | 1.126 | 0.698
      * effect 2:   0.000 | +0.885 | 1.127 | 0.790
    After 300 steps mu_scale has not come down far enough for any target to reach |z| = 1.96 (the screen's own fit calls
    none of its 41 targets either): no candidate of (1, 1.5, 2) gives the detection rate a margin over the null's, so the
    rates are printed and only the sign of the mean mu_loc is asserted.  Effect 1, the smallest candidate, is planted."""
    from bean_amd import engine
    from bean_amd.model import run as model_run

    monkeypatch.chdir(tmp_path)
    mod, gd = _models()
    data = screens["203"]
    full, fits = power
    assert len(fits) == len(RUN_EFFECTS) and all(len(row) == N_SCREENS for row in fits)  # (effect 0 put in front)
    want_full = model_run.run_inference(mod, gd, data, num_steps=STEPS, seed=7, verbose=False)
    _same_results(full, want_full)
    eng = model_run.bootstrap_engine(mod, gd, data, want_full[0])
    try:
        sim = {k: v.cpu() for k, v in eng.simulate_power(0, N_SCREENS, RUN_EFFECTS, seed=POWER_SEED).items()}
    finally:
        eng.close()
    for i in range(len(RUN_EFFECTS)):
        for j in range(N_SCREENS):
            redrawn = copy.copy(data)
            redrawn.X_masked = sim["X"][i, j].to(data.X_masked.dtype)
            redrawn.X_bcmatch_masked = sim["X_bcmatch"][i, j].to(data.X_bcmatch_masked.dtype)
            _same_results(fits[i][j], model_run.run_inference(mod, gd, redrawn, num_steps=STEPS, seed=7, verbose=False))
    # several engine runs: three screens next to the screen each
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble",
                        lambda self, *a, **k: (used.append(self.n_members), real(self, *a, **k))[1])
    parts = model_run.run_inference_power(mod, gd, data, RUN_EFFECTS, n_screens=N_SCREENS, seed=7, power_seed=POWER_SEED,
                                          num_steps=STEPS, verbose=False, max_per_run=3)
    assert used == [4] * 6 + [3] * 3, used  # 8 screens: 3 + 3 + 2, three report windows each
    _same_results(parts[0], full)
    for row, want in zip(parts[1], fits):
        for a, b in zip(row, want):
            _same_results(a, b)
    summary = power_summary(full, fits, RUN_EFFECTS)
    T = int(data.n_targets)
    assert summary["n_screens"] == N_SCREENS and summary["n_planted"] == T and summary["power"].shape == (2, T)
    null, at = (float(v) for v in summary["power_mean"])
    mean_m = float(summary["mu_power_mean"][1].mean())
    print(f"power_mean at effects {RUN_EFFECTS}: {null:.4f} {at:.4f}; power_median {summary['power_median'].tolist()}; "
          f"mean mu_loc at the effect {mean_m:+.4f}, at the null {float(summary['mu_power_mean'][0].mean()):+.4f}; "
          f"shrinkage {summary['shrinkage'].tolist()}")
    assert 0.0 <= null <= 1.0 and 0.0 <= at <= 1.0
    assert np.sign(mean_m) == np.sign(RUN_EFFECTS[1])  # direction only (the docstring)


def test_run_inference_power_fallback_and_mask(screens, power, tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import run as model_run

    monkeypatch.chdir(tmp_path)
    mod, gd = _models()
    data = screens["203"]
    full, fits = power
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble", lambda self, *a, **k: (used.append(1), real(self, *a, **k))[1])
    monkeypatch.setattr(engine.HipSVI, "ensemble_supported", property(lambda self: False))
    serial = model_run.run_inference_power(mod, gd, data, [RUN_EFFECTS[1]], n_screens=2, seed=7, power_seed=POWER_SEED,
                                           num_steps=STEPS, verbose=False)  # (effect 0 is put in front)
    assert used == []
    _same_results(serial[0], full)
    assert len(serial[1]) == 2
    for row, want in zip(serial[1], fits):
        for a, b in zip(row, want[:2]):
            _same_results(a, b)


# ------------------------------------------------------------------ 7. CLI
def test_cli_power(tmp_path):
    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    dd = _run(str(tmp_path / "power"), *base, "--power-effects", "0.5,-1", "--power-screens", "3", "--save-raw")
    d0 = _run(str(tmp_path / "plain"), *base)
    name_el, name_sg = "bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"
    plain_el, plain_sg = open(f"{d0}/{name_el}", "rb").read(), open(f"{d0}/{name_sg}", "rb").read()
    assert open(f"{dd}/{name_sg}", "rb").read() == plain_sg
    columns = ["power_x0", "power_x0.5", "power_x-1", "mde80", "mde80_neg"]
    assert _without_columns(f"{dd}/{name_el}", columns) == plain_el
    el, plain = pd.read_csv(f"{dd}/{name_el}"), pd.read_csv(f"{d0}/{name_el}")
    assert [c for c in el.columns if c not in plain.columns] == columns
    rates = el[columns[:3]].values.astype(float)
    assert len(el) == 6 and np.isfinite(rates).all() and (rates >= 0).all() and (rates <= 1).all()
    assert set(np.unique(rates * 3).round(9)) <= {0.0, 1.0, 2.0, 3.0}  # shares of three screens
    assert not np.isnan(el[["mde80", "mde80_neg"]].values.astype(float)).any()  # every target planted: a number or inf
    assert not os.path.exists(f"{d0}/bean_power.MixtureNormal.csv")
    table = pd.read_csv(f"{dd}/bean_power.MixtureNormal.csv")
    assert list(table.columns) == ["effect", "n_screens", "n_planted", "power_mean", "power_median", "shrinkage",
                                   "median_mu_power_se"]
    assert len(table) == 3 and table["effect"].tolist() == [0.0, 0.5, -1.0]
    assert (table["n_screens"] == 3).all() and (table["n_planted"] == 6).all()
    assert np.isnan(table["shrinkage"][0]) and np.isfinite(table["shrinkage"][1:]).all()
    np.testing.assert_allclose(table["power_mean"], rates.mean(0), rtol=1e-12)
    with open(f"{dd}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    entries = raw["power"]
    assert [(e["effect"], e["screen"]) for e in entries] == [(f, j) for f in (0.0, 0.5, -1.0) for j in range(3)]
    assert all(set(e) == {"effect", "screen", "params", "loss"} and len(e["loss"]) == 200 for e in entries)
    again = power_summary(raw["params"], [[e["params"] for e in entries[3 * i:3 * i + 3]] for i in range(3)], [0.0, 0.5, -1.0])
    np.testing.assert_allclose(sorted(again["power"][1].tolist()), sorted(el["power_x0.5"]), rtol=1e-12)
    # a tiling screen is refused with the family named
    import contextlib
    import io

    from bean_amd.cli.execute import main

    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(["run", "sorting", "tiling", VAR, "--power-effects", "0.5,2", "-o", str(tmp_path / "tiling")])
    assert exc.value.code == 2
    assert ("--power-effects simulates the counts of the sorting variant models (Normal, MixtureNormal) and is not "
            "available for tiling screens (MultiMixtureNormal).") in " ".join(err.getvalue().split())
