"""Parametric bootstrap on the GPU: K replicate screens in one launch (bean_hip_simulate_members,
csrc/bean_predictive.hpp::k_simulate_members) are, plane by plane, the screens of the single-draw simulator; their
invariants; the state the call must leave alone; its refusals; run_inference_bootstrap batched, in several engine runs
and in its fallback; and the CLI.  -m gpu."""
import ctypes
import pickle
from functools import partial

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.jackknife import bootstrap_summary
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

from members_common import (CONFIGS, DEV, VAR, _h5ad_reader_present, _kw_of, _mini, _run, _same_results,  # noqa: F401
                            _state, _without_columns)

pytestmark = pytest.mark.gpu
SEED = 101
FIRST, K = 7, 5
COLUMNS = ["mu_boot_se", "mu_boot_bias", "n_boot"]


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
    """Random draws for every per-target and per-guide Normal site the engine has (not pi: that one is per member)."""
    g = torch.Generator().manual_seed(seed)
    noise = {"eps_mu": torch.randn(eng.T, generator=g, dtype=torch.float64),
             "eps_sd": torch.randn(eng.T, generator=g, dtype=torch.float64)}
    if eng.scale_by_accessibility:
        noise["eps_noise"] = torch.randn(eng.data.n_guides, generator=g, dtype=torch.float64)
    return noise


# ------------------------------------------------------------------ 1. planes are the single draws
@pytest.mark.parametrize("family,kw", CONFIGS)
def test_planes_are_the_single_draws(engines, family, kw):
    eng = engines(_which(kw), family, kw)
    assert eng.predictive_supported
    R, B, G = eng.data.n_reps, eng.data.n_condits, eng.data.n_guides
    assert (R, B, G) == (3, 5, 203)
    assert not bool(eng._keep["REPGUIDE"].bool().all())  # masks present
    keys = {"X", "X_bcmatch"} if eng.use_bcmatch else {"X"}
    eng.set_noise(_site_noise(eng, 9))
    try:
        many = eng.simulate_members(FIRST, K, seed=SEED)
        assert set(many) == keys
        singles = [eng.simulate(FIRST + k, seed=SEED) for k in range(K)]
        torch.cuda.synchronize()
    finally:
        eng.set_noise(None)
    for key in keys:
        assert many[key].shape == (K, R, B, G) and many[key].dtype == torch.float32 and many[key].is_contiguous()
        for k in range(K):
            assert torch.equal(many[key][k], singles[k][key]), (key, k)
    # without injection the target / guide sites are draw FIRST's for every member: plane 0 alone is a single draw
    many = eng.simulate_members(FIRST, K, seed=SEED)
    one, next_one = eng.simulate(FIRST, seed=SEED), eng.simulate(FIRST + 1, seed=SEED)
    torch.cuda.synchronize()
    for key in keys:
        assert torch.equal(many[key][0], one[key]), key
        assert not torch.equal(many[key][1], next_one[key]), key


# ------------------------------------------------------------------ 2. invariants
def _check_invariants(eng, k_small, k_all):
    obs = _observed(eng)
    a = eng.simulate_members(FIRST, k_all, seed=SEED)
    torch.cuda.synchronize()
    assert set(a) == set(obs)
    for key, x in a.items():
        assert x.shape == (k_all,) + tuple(obs[key].shape)
        assert bool((x >= 0).all()) and bool((x == x.round()).all()), key
        # every (member, replicate, guide) keeps its observed total
        assert torch.equal(x.double().sum(2), obs[key].double().sum(1).expand(k_all, -1, -1)), key
        for i in range(k_all):
            for j in range(i + 1, k_all):
                assert not torch.equal(x[i], x[j]), (key, i, j)
    again = eng.simulate_members(FIRST, k_all, seed=SEED)
    fewer = eng.simulate_members(FIRST, k_small, seed=SEED)
    other_seed = eng.simulate_members(FIRST, k_all, seed=SEED + 1)
    other_first = eng.simulate_members(FIRST + 1, k_all, seed=SEED)
    torch.cuda.synchronize()
    for key in a:
        assert torch.equal(a[key], again[key]), key
        assert torch.equal(fewer[key], a[key][:k_small]), key
        assert not torch.equal(a[key], other_seed[key]), key
        assert not torch.equal(a[key], other_first[key]), key
        assert not torch.equal(a[key][1:], other_first[key][:-1]), key  # (the shared sites moved to draw FIRST + 1)
    return a


@pytest.mark.parametrize("family,kw", [CONFIGS[0], CONFIGS[2], CONFIGS[4]])
def test_invariants(engines, family, kw):
    eng = engines(_which(kw), family, kw)
    _check_invariants(eng, 3, K)


def test_sixty_four_members_in_one_call(engines):
    eng = engines("203", "MixtureNormal", {})
    obs = _observed(eng)
    out = eng.simulate_members(0, _lib.MAX_MEMBERS, seed=SEED)
    first = eng.simulate_members(0, K, seed=SEED)
    torch.cuda.synchronize()
    for key, x in out.items():
        assert x.shape[0] == 64
        assert bool((x >= 0).all()) and bool((x == x.round()).all()), key
        assert torch.equal(x.double().sum(2), obs[key].double().sum(1).expand(64, -1, -1)), key
        assert torch.equal(x[:K], first[key]) and not torch.equal(x[62], x[63]), key


@pytest.mark.parametrize("family,kw", [CONFIGS[0], CONFIGS[2]])
def test_invariants_on_the_mini_screen(engines, family, kw):
    eng = engines("mini", family, kw)
    assert eng.predictive_supported and eng.data.n_guides == 30
    a = _check_invariants(eng, 2, 3)
    one = eng.simulate(FIRST, seed=SEED)
    torch.cuda.synchronize()
    for key in a:
        assert torch.equal(a[key][0], one[key]), key


# ------------------------------------------------------------------ 3. untouched state
def test_simulate_members_leaves_the_fit_alone(screens):
    from bean_amd import engine

    data = screens["203"].to(DEV)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(20, seed=SEED)
    torch.cuda.synchronize()
    before = _state(eng)
    grads = {k: v.clone() for k, v in eng.grads.items()}
    hist = eng.loss_hist.clone()
    eng.simulate_members(2, K, seed=7)
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
            x = torch.empty((K,) + tuple(e._keep["X"].shape), dtype=torch.float32, device=DEV)
            xbc = torch.empty_like(x)
            nb = x.numel() * 4
            assert e.lib.bean_hip_simulate_members(e._h, SEED + 5, 1, K, ctypes.c_void_p(x.data_ptr()), nb,
                                                   ctypes.c_void_p(xbc.data_ptr()), nb, e._sptr()) == 0
        elif simulate_first:
            e.simulate_members(1, K, seed=SEED + 5)
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


# ------------------------------------------------------------------ 4. refusals
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

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    sim = lambda k, *a: lib.bean_hip_simulate_members(eng._h, SEED, 0, k, *a, eng._sptr())  # noqa: E731
    assert lib.bean_hip_simulate_members(None, SEED, 0, K, p(x), K * one, None, 0, None) < 0 and "null handle" in err()
    for bad in (0, -1, 65):
        assert sim(bad, p(x), max(bad, 0) * one, p(xbc), max(bad, 0) * one) < 0
        assert "n_draws" in err() and "[1, 64]" in err(), err()
    assert sim(K, p(x), K * one - 4, p(xbc), K * one) < 0 and "x_out" in err() and "K = 5" in err()
    assert sim(K, p(x), one, p(xbc), K * one) < 0 and "x_out" in err() and "K = 5" in err()
    assert sim(K, None, 0, p(xbc), K * one) < 0 and "x_out" in err()
    assert sim(K, p(x), K * one, p(xbc), (K + 1) * one) < 0 and "xbc_out" in err() and "K = 5" in err()
    assert sim(K, p(x), K * one, None, 0) < 0 and "xbc_out" in err()
    assert float(x.abs().sum()) == 0 and float(xbc.abs().sum()) == 0  # nothing was launched
    assert sim(K, p(x), K * one, p(xbc), K * one) == 0
    torch.cuda.synchronize()
    assert float(x.double().sum()) == K * float(eng._keep["X"].double().sum())
    with pytest.raises(RuntimeError, match=r"\[1, 64\]"):
        eng.simulate_members(0, 65)
    assert set(eng.simulate_members(0, 2)) == {"X", "X_bcmatch"}
    eng.close()

    nobc = engine.HipSVI("MixtureNormal", data, num_steps=50, use_bcmatch=False)
    assert lib.bean_hip_simulate_members(nobc._h, SEED, 0, K, p(x), K * one, p(xbc), K * one, nobc._sptr()) < 0
    assert "xbc_out" in err() and "BEAN_FLAG_USE_BCMATCH" in err()
    assert set(nobc.simulate_members(0, K)) == {"X"}
    # an unprepared handle of the same shape
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(nobc._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_predictive_supported(h) == 1
    assert lib.bean_hip_simulate_members(h, SEED, 0, K, p(x), K * one, None, 0, None) < 0 and "bean_hip_prepare" in err()
    assert lib.bean_hip_destroy(h) == 0
    nobc.close()

    for extra in (dict(n_members=2), dict(n_particles=2)):
        many = engine.HipSVI("MixtureNormal", data, num_steps=50, **extra)
        assert lib.bean_hip_simulate_members(many._h, SEED, 0, K, p(x), K * one, p(xbc), K * one, many._sptr()) < 0
        assert "bean_hip_predictive_supported" in err()
        with pytest.raises(PredictiveUnsupported):
            many.simulate_members(0, K)
        if "n_members" in extra:
            many.run_ensemble(5, [1, 2])
        else:
            many.run_particles(5, SEED)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(many.loss_hist[..., :5]).all())
        many.close()

    for other in (engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10)):
        assert lib.bean_hip_simulate_members(other._h, SEED, 0, K, p(x), K * one, None, 0, other._sptr()) < 0
        assert "bean_hip_predictive_supported" in err()
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.simulate_members(0, K)
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()


# ------------------------------------------------------------------ 5. run_inference_bootstrap
N_BOOT, STEPS, BOOT_SEED = 4, 300, 55


def _models(which):
    from bean_amd.model import model as m

    if which == "Normal":
        return "203", partial(m.NormalModel), m.NormalGuide
    return ("203acc", partial(m.MixtureNormalModel, scale_by_accessibility=True),
            partial(m.MixtureNormalGuide, scale_by_accessibility=True, fit_noise=True))


@pytest.fixture(scope="module")
def bootstraps(screens, tmp_path_factory):
    """run_inference_bootstrap with its defaults, once per family."""
    import os

    from bean_amd.model.run import run_inference_bootstrap

    cache = {}

    def get(which):
        if which not in cache:
            name, mod, gd = _models(which)
            cwd = os.getcwd()
            os.chdir(tmp_path_factory.mktemp("fit"))
            try:
                cache[which] = run_inference_bootstrap(mod, gd, screens[name], n_boot=N_BOOT, seed=7, boot_seed=BOOT_SEED,
                                                       num_steps=STEPS, verbose=False)
            finally:
                os.chdir(cwd)
        return cache[which]

    return get


@pytest.mark.parametrize("which", ["Normal", "MixtureNormal+Acc"])
def test_run_inference_bootstrap_is_the_single_fits(screens, bootstraps, which, tmp_path, monkeypatch):
    import copy

    from bean_amd import engine
    from bean_amd.model import run as model_run

    monkeypatch.chdir(tmp_path)
    name, mod, gd = _models(which)
    data = screens[name]
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble",
                        lambda self, *a, **k: (used.append(self.n_members), real(self, *a, **k))[1])
    full, boots = bootstraps(which)
    assert len(boots) == N_BOOT
    want_full = model_run.run_inference(mod, gd, data, num_steps=STEPS, seed=7, verbose=False)
    _same_results(full, want_full)
    # the screens: planes of one simulate_members call on an engine prepared the same way
    eng = model_run.bootstrap_engine(mod, gd, data, want_full[0])
    try:
        sim = {k: v.cpu() for k, v in eng.simulate_members(0, N_BOOT, seed=BOOT_SEED).items()}
    finally:
        eng.close()
    for j in (0, 3):
        redrawn = copy.copy(data)
        redrawn.X_masked = sim["X"][j].to(data.X_masked.dtype)
        if "X_bcmatch" in sim:
            redrawn.X_bcmatch_masked = sim["X_bcmatch"][j].to(data.X_bcmatch_masked.dtype)
        assert not torch.equal(redrawn.X_masked, data.X_masked)
        _same_results(boots[j], model_run.run_inference(mod, gd, redrawn, num_steps=STEPS, seed=7, verbose=False))
    # several engine runs: two bootstrap screens next to the screen each
    used.clear()
    parts = model_run.run_inference_bootstrap(mod, gd, data, n_boot=N_BOOT, seed=7, boot_seed=BOOT_SEED, num_steps=STEPS,
                                              verbose=False, max_per_run=2)
    assert used == [3] * 6, used
    _same_results(parts[0], full)
    for a, b in zip(parts[1], boots):
        _same_results(a, b)
    summary = bootstrap_summary(full, boots)
    assert summary["n_boot"] == N_BOOT
    se = summary["mu_boot_se"]
    assert se.shape == full[0]["mu_loc"].shape and bool(torch.isfinite(se).all()) and bool((se > 0).all())
    assert bool(torch.isfinite(summary["mu_boot_bias"]).all())


@pytest.mark.parametrize("which", ["Normal", "MixtureNormal+Acc"])
def test_run_inference_bootstrap_fallback_and_boot_seeds(screens, bootstraps, which, tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import run as model_run

    monkeypatch.chdir(tmp_path)
    name, mod, gd = _models(which)
    data = screens[name]
    full, boots = bootstraps(which)
    other = model_run.run_inference_bootstrap(mod, gd, data, n_boot=N_BOOT, seed=7, boot_seed=BOOT_SEED + 1,
                                              num_steps=STEPS, verbose=False)
    _same_results(other[0], full)
    for a, b in zip(other[1], boots):
        assert not torch.equal(a[1]["params"]["mu_loc"], b[1]["params"]["mu_loc"])
    # one fit after the other
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble", lambda self, *a, **k: (used.append(1), real(self, *a, **k))[1])
    monkeypatch.setattr(model_run, "_fit_members", lambda *a, **k: None)
    serial = model_run.run_inference_bootstrap(mod, gd, data, n_boot=N_BOOT, seed=7, boot_seed=BOOT_SEED, num_steps=STEPS,
                                               verbose=False)
    assert used == []
    _same_results(serial[0], full)
    for a, b in zip(serial[1], boots):
        _same_results(a, b)


# ------------------------------------------------------------------ 6. CLI
def test_cli_bootstrap(tmp_path):
    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    db = _run(str(tmp_path / "boot"), *base, "--bootstrap", "4", "--save-raw")
    d0 = _run(str(tmp_path / "plain"), *base)
    dz = _run(str(tmp_path / "zero"), *base, "--bootstrap", "0")
    name_el, name_sg = "bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"
    plain_el, plain_sg = open(f"{d0}/{name_el}", "rb").read(), open(f"{d0}/{name_sg}", "rb").read()
    assert open(f"{dz}/{name_el}", "rb").read() == plain_el and open(f"{dz}/{name_sg}", "rb").read() == plain_sg
    assert open(f"{db}/{name_sg}", "rb").read() == plain_sg
    assert _without_columns(f"{d0}/{name_el}", []) == plain_el  # (the cutting itself leaves a table's bytes alone)
    assert _without_columns(f"{db}/{name_el}", COLUMNS) == plain_el
    el, plain = pd.read_csv(f"{db}/{name_el}"), pd.read_csv(f"{d0}/{name_el}")
    assert [c for c in el.columns if c not in plain.columns] == COLUMNS
    assert len(el) == 6 and np.isfinite(el[COLUMNS].values.astype(float)).all()
    assert (el["mu_boot_se"] > 0).all() and (el["n_boot"] == 4).all()
    with open(f"{db}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    entries = raw["bootstrap"]
    assert len(entries) == 4 and [e["screen"] for e in entries] == [0, 1, 2, 3]
    assert all(set(e) == {"screen", "params", "loss"} and len(e["loss"]) == 200 for e in entries)
    assert not torch.equal(entries[0]["params"]["mu_loc"], raw["params"]["mu_loc"])
    again = bootstrap_summary(raw["params"], [e["params"] for e in entries])
    np.testing.assert_allclose(sorted(again["mu_boot_se"].reshape(-1).tolist()), sorted(el["mu_boot_se"]), rtol=1e-12)
