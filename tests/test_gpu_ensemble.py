"""Seed ensembles on the GPU: member k of an ensemble is, bit for bit, the single fit with seeds[k] - parameters, both
moments and the loss history - for every sorting variant family the batched kernels take; the C entry points' rejections;
the fallback for the other families; the CLI.  -m gpu."""
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
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

import members_common
from members_common import (CONFIGS, DEV, GOLD, STEPS, VAR, _assert_same, _h5ad_reader_present, _kw_of, _mini,  # noqa: F401
                            _run, _state)

pytestmark = pytest.mark.gpu
BW = os.path.join(GOLD, "accessibility_signal_chr6.bw")
SEEDS = (101, 7, 2_000_000_011)


def _single(family, data, seed, kw, steps=STEPS, **run_kw):
    return members_common._single(family, data, kw, seed=seed, steps=steps, **run_kw)


def _check_members(family, data, kw, seeds=SEEDS):
    from bean_amd import engine

    data = data.to(DEV)
    ens = engine.HipSVI(family, data, num_steps=STEPS, n_members=len(seeds), **kw)
    assert ens.ensemble_supported
    ens.run_ensemble(STEPS, seeds)
    torch.cuda.synchronize()
    losses = ens.losses()
    assert losses.shape == (len(seeds), STEPS) and np.isfinite(losses).all()
    members = [_state(ens, k) for k in range(len(seeds))]
    c1 = ens.constrained(member=1)
    assert torch.equal(c1["mu_scale"], ens.unconstrained["mu_scale"][1].exp())
    ens.close()
    for k, seed in enumerate(seeds):
        _assert_same(members[k], _single(family, data, seed, kw), f"{family} {kw} member {k} (seed {seed})")
    assert not torch.equal(members[0]["p.mu_loc"], members[1]["p.mu_loc"])


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_member_is_the_single_fit_readme_shape(family, kw):
    """3 455 guides x 6 replicates: 54 tiles, thin targets (k_param KIND 1)."""
    data = make_sorting_variant_screen(3455, 6, seed=3, with_accessibility=bool(kw.get("scale_by_accessibility")))
    _check_members(family, data, _kw_of(kw, data))


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_member_is_the_single_fit_ragged_tiles(family, kw):
    """1 003 guides (not a multiple of 64), seven guides per target: 64 = 9 * 7 + 1, so a target straddles every tile
    boundary; masked (replicate, guide) pairs and a masked sample."""
    data = make_sorting_variant_screen(1003, 3, seed=9, guides_per_target=7, mask_fraction=0.05,
                                       with_accessibility=bool(kw.get("scale_by_accessibility")))
    lengths = data.target_lengths
    off = data.target_offsets
    assert any(int(off[t]) // 64 != (int(off[t]) + int(lengths[t]) - 1) // 64 for t in range(data.n_targets))
    _check_members(family, data, _kw_of(kw, data))


@pytest.mark.parametrize("extra,family,kw", [
    ([], "MixtureNormal", {}),
    (["--uniform-edit"], "Normal", {}),
    (["--scale-by-acc", "--acc-bw-path", BW, "--repguide-mask", "None"], "MixtureNormal", dict(scale_by_accessibility=True)),
    (["--scale-by-acc", "--acc-bw-path", BW, "--repguide-mask", "None"], "MixtureNormal",
     dict(scale_by_accessibility=True, fit_noise=False)),
    ([], "MixtureNormal", dict(prior="yes")),
])
def test_member_is_the_single_fit_mini_screen(tmp_path, extra, family, kw):
    """The 30-guide fixture every reference test runs: 6 targets, i.e. the wide-target (generic) k_param."""
    data = _mini(tmp_path, *extra)
    assert (data.n_guides, data.n_targets) == (30, 6)
    _check_members(family, data, _kw_of(kw, data))


def test_supported_set():
    from bean_amd import engine

    var = make_sorting_variant_screen(640, 3, seed=2, with_accessibility=True).to(DEV)
    for family, kw in CONFIGS:
        eng = engine.HipSVI(family, var, num_steps=10, **_kw_of(kw, var))
        assert eng.ensemble_supported, (family, kw)
        eng.close()
    tiling = engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10)
    surv = engine.HipSVI("MixtureNormal", make_survival_variant_screen(300, 2, seed=2).to(DEV), num_steps=10)
    for eng in (tiling, surv):
        assert not eng.ensemble_supported
        eng.close()
    with pytest.raises(engine.EnsembleUnsupported):
        engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10, n_members=2)


def test_rejections_leave_the_handle_usable():
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2).to(DEV)
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731

    # a fresh handle, nothing bound yet: K < 1 and K above the cap are refused, a valid K is then accepted
    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(eng._shape), ctypes.byref(h)) == 0
    for bad in (0, -3, _lib.MAX_MEMBERS + 1):
        assert lib.bean_hip_set_members(h, bad) < 0 and "n_members" in err(), bad
    assert lib.bean_hip_set_members(h, 2) == 0
    assert lib.bean_hip_set_members(h, 3) == 0
    buf = torch.zeros(3 * data.n_targets, dtype=torch.float32, device=DEV)
    assert lib.bean_hip_bind(h, _lib.BUF["P"], ctypes.c_void_p(buf.data_ptr()), 4 * data.n_targets) < 0  # single-fit size
    assert "3 member" in err()
    assert lib.bean_hip_bind(h, _lib.BUF["P"], ctypes.c_void_p(buf.data_ptr()), 12 * data.n_targets) == 0
    assert lib.bean_hip_set_members(h, 2) < 0 and "before any bean_hip_bind" in err()  # after a bind
    assert lib.bean_hip_destroy(h) == 0
    eng.close()

    # a tiling shape
    til = engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10)
    assert lib.bean_hip_ensemble_supported(til._h) == 0
    assert lib.bean_hip_set_members(til._h, 2) < 0 and "do not take this shape" in err()
    til.run(5, seed=101)  # still a working single-fit handle
    torch.cuda.synchronize()
    assert np.isfinite(til.losses()).all()
    til.close()

    # run_ensemble with the wrong number of seeds / null seeds: nothing runs, the next valid call does
    ens = engine.HipSVI("MixtureNormal", data, num_steps=50, n_members=2)
    before = _state(ens, 0)
    three = (ctypes.c_uint64 * 3)(1, 2, 3)
    assert lib.bean_hip_svi_run_ensemble(ens._h, three, 3, 0, 10, 0, ens._sptr()) < 0 and "3 seeds for 2 member" in err()
    assert lib.bean_hip_svi_run_ensemble(ens._h, None, 2, 0, 10, 0, ens._sptr()) < 0 and "null seeds" in err()
    with pytest.raises(RuntimeError, match="seeds for 2 member"):
        ens.run_ensemble(10, [101])
    torch.cuda.synchronize()
    for k, v in before.items():
        if k != "loss":
            assert torch.equal(_state(ens, 0)[k], v), k
    ens.run_ensemble(10, [101, 102])
    torch.cuda.synchronize()
    assert np.isfinite(ens.losses()).all() and ens.losses().shape == (2, 10)
    ens.close()


def test_one_member_windows_and_eager_launches():
    from bean_amd import engine

    data = make_sorting_variant_screen(1003, 3, seed=9, guides_per_target=7).to(DEV)
    want = [_single("MixtureNormal", data, s, {}) for s in SEEDS]

    # an ensemble of one, on a handle that never heard of members
    one = engine.HipSVI("MixtureNormal", data, num_steps=STEPS)
    one.run_ensemble(STEPS, [SEEDS[0]])
    torch.cuda.synchronize()
    _assert_same(_state(one), want[0], "K = 1")
    one.close()

    for what, calls, chunk in (("windows", (100, 100, 100), 50), ("eager", (STEPS,), 0), ("chunk 7", (150, 150), 7)):
        ens = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=3)
        for n in calls:
            ens.run_ensemble(n, SEEDS, graph_chunk=chunk)
        torch.cuda.synchronize()
        for k in range(3):
            _assert_same(_state(ens, k), want[k], f"{what} member {k}")
        ens.close()

    # new seeds on the same handle (the graphs hold the address of the members' arguments, not the seeds)
    ens = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=2)
    tensors = list(ens.unconstrained.values()) + list(ens._m.values()) + list(ens._v.values())
    initial = [t.clone() for t in tensors]
    ens.run_ensemble(20, [5, 6], first_step=0)
    torch.cuda.synchronize()
    for t, t0 in zip(tensors, initial):
        t.copy_(t0)
    ens.run_ensemble(STEPS, SEEDS[:2], first_step=0)
    torch.cuda.synchronize()
    for k in range(2):
        _assert_same(_state(ens, k), want[k], f"reseeded member {k}")
    ens.close()


def test_members_do_not_touch_each_other():
    from bean_amd import engine

    data = make_sorting_variant_screen(1003, 3, seed=9, guides_per_target=7).to(DEV)
    ens = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=2)
    ens.run_ensemble(STEPS, [101, 101])
    torch.cuda.synchronize()
    _assert_same(_state(ens, 0), _state(ens, 1), "same seed twice")
    ens.close()
    ens = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=2)
    ens.run_ensemble(STEPS, [101, 102])
    torch.cuda.synchronize()
    assert not torch.equal(ens.unconstrained["mu_loc"][0], ens.unconstrained["mu_loc"][1])
    assert not torch.equal(ens.loss_hist[0, :STEPS], ens.loss_hist[1, :STEPS])
    ens.close()


def test_a_diverged_member_stays_alone():
    from bean_amd import engine

    data = make_sorting_variant_screen(1003, 3, seed=9, guides_per_target=7).to(DEV)
    ens = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=3)
    ens.unconstrained["mu_loc"][1, 4] = float("nan")
    ens.run_ensemble(100, SEEDS)
    torch.cuda.synchronize()
    losses = ens.losses()
    assert np.isnan(losses[1]).all()
    for k in (0, 2):
        _assert_same(_state(ens, k), _single("MixtureNormal", data, SEEDS[k], {}, steps=100), f"member {k} beside a NaN member")
    ens.close()


def test_run_inference_ensemble_batched_and_fallback(tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model import survival_model as sm
    from bean_amd.model.run import ParamStore, run_inference, run_inference_ensemble

    monkeypatch.chdir(tmp_path)
    seeds = [101, 7]

    def same(res, model, guide, data, n):
        assert isinstance(res, list) and len(res) == len(seeds)
        for (store, out), seed in zip(res, seeds):
            ref_store, ref = run_inference(model, guide, data, num_steps=n, seed=seed, verbose=False)
            assert isinstance(store, ParamStore) and set(out) == {"loss", "params"}
            assert isinstance(out["loss"], list) and len(out["loss"]) == n and out["loss"] == ref["loss"]
            assert set(out["params"]) == set(ref["params"]) == set(store.keys())
            for k, v in ref["params"].items():
                assert out["params"][k].device.type == "cpu" and torch.equal(out["params"][k], v), (seed, k)
                assert torch.equal(store[k].cpu(), ref_store[k].cpu()), (seed, k)

    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble", lambda self, *a, **k: (used.append(a[0]), real(self, *a, **k))[1])
    var = make_sorting_variant_screen(640, 3, seed=2)
    mod, gd = partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)
    same(run_inference_ensemble(mod, gd, var, seeds, num_steps=250, verbose=False), mod, gd, var, 250)
    assert used == [100, 100, 50]  # batched, in report windows
    used.clear()
    til = make_sorting_tiling_screen(200, 2, seed=2)
    mod, gd = partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide)
    same(run_inference_ensemble(mod, gd, til, seeds, num_steps=120, verbose=False), mod, gd, til, 120)
    surv = make_survival_variant_screen(300, 2, seed=2)
    mod, gd = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)
    same(run_inference_ensemble(mod, gd, surv, seeds, num_steps=120, verbose=False), mod, gd, surv, 120)
    assert used == []  # the fallback: one fit after the other


def test_run_inference_ensemble_halts_naming_the_member(tmp_path, monkeypatch):
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_ensemble

    data = make_sorting_variant_screen(2000, 3, seed=4)
    data.a0 = data.a0.clone()
    data.a0[17] = float("nan")  # shared data: every member's loss is NaN from step 0; the first one is named
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*member 0 \(seed 101\).*non-finite loss at iteration 0"):
        run_inference_ensemble(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, [101, 102],
                               num_steps=1000, verbose=False)
    with open(tmp_path / "tmp_result.member0.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert dump["member"] == 0 and dump["seed"] == 101 and "mu_loc" in dump["param"]
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


def test_cli_n_seeds(tmp_path):
    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    d3 = _run(str(tmp_path / "k3"), *base, "--n-seeds", "3", "--save-raw")
    el = pd.read_csv(f"{d3}/bean_element_result.MixtureNormal.csv")
    sg = pd.read_csv(f"{d3}/bean_sgRNA_result.MixtureNormal.csv")
    assert len(el) == 6 and len(sg) == 30
    assert (el["n_seeds"] == 3).all() and (el["mu_seed_sd"] >= 0).all() and (el["mu_seed_sd"] > 0).any()
    assert np.isfinite(el[["mu", "mu_sd", "mu_z", "sd"]].values).all()
    with open(f"{d3}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    assert len(raw["ensemble"]) == 3 and all(set(e) == {"params", "loss"} for e in raw["ensemble"])
    mus = torch.stack([e["params"]["mu_loc"].double() for e in raw["ensemble"]])
    assert torch.allclose(raw["params"]["mu_loc"].double(), mus.mean(0), rtol=0, atol=1e-12)
    d1 = _run(str(tmp_path / "k1"), *base, "--n-seeds", "1")
    d0 = _run(str(tmp_path / "k0"), *base)
    for name in ("bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"):
        assert open(f"{d1}/{name}", "rb").read() == open(f"{d0}/{name}", "rb").read(), name
    plain = pd.read_csv(f"{d0}/bean_element_result.MixtureNormal.csv")
    assert "mu_seed_sd" not in plain.columns and "n_seeds" not in plain.columns
    # member 0 of the ensemble is the fit a run without the flag does
    one = plain.sort_values("target")["mu"].values
    mu0 = raw["ensemble"][0]["params"]["mu_loc"].reshape(-1).numpy()
    np.testing.assert_allclose(np.sort(one), np.sort(mu0), rtol=1e-6)
