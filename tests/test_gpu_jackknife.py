"""Replicate jackknife on the GPU: a member with its own masks is, bit for bit, the single fit of the screen with those
masks - parameters, both moments and the loss history - for every sorting variant family the batched kernels take, in
windows, eagerly and across a second prepare; the per-member loss constants; the C entry point's rejections; the
fallback for the other families; the CLI.  -m gpu."""
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
from bean_amd.model.jackknife import candidate_replicates, leave_out, member_masks
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

from members_common import (CONFIGS, DEV, SEED, STEPS, VAR, _assert_same, _h5ad_reader_present, _kw_of, _run,  # noqa: F401
                            _same_results, _single, _state, _without_columns)

pytestmark = pytest.mark.gpu
COLUMNS = ["mu_jk_se", "mu_jk_max_shift", "mu_jk_max_shift_rep", "n_jk"]


def _screens(data):
    """The full screen and its leave-one-replicate-out copies, in member order."""
    left_out = candidate_replicates(data)
    return [data] + [leave_out(data, r) for r in left_out], left_out


def _jackknife_engine(family, data, kw, **extra):
    from bean_amd import engine

    screens, left_out = _screens(data)
    eng = engine.HipSVI(family, data, num_steps=STEPS, n_members=len(screens), member_masks=member_masks(data, left_out),
                        **kw, **extra)
    assert eng.ensemble_supported and eng.member_masks
    return eng, screens


def _check_members(family, data, kw):
    data = data.to(DEV)
    ens, screens = _jackknife_engine(family, data, kw)
    n = len(screens)
    assert n == data.n_reps + 1
    ens.run_ensemble(STEPS, [SEED] * n)
    torch.cuda.synchronize()
    losses = ens.losses()
    assert losses.shape == (n, STEPS) and np.isfinite(losses).all()
    members = [_state(ens, k) for k in range(n)]
    ens.close()
    for k, screen in enumerate(screens):
        what = "the plain fit" if k == 0 else f"replicate {k - 1} left out"
        _assert_same(members[k], _single(family, screen, kw), f"{family} {kw} member {k} ({what})")
    # same seed, other data: the members differ from the full fit and from each other
    assert not torch.equal(members[0]["p.mu_loc"], members[1]["p.mu_loc"])
    assert not torch.equal(members[1]["p.mu_loc"], members[2]["p.mu_loc"])


def _ragged(**kw):
    return make_sorting_variant_screen(1003, 3, seed=9, guides_per_target=7, mask_fraction=0.05, **kw)


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_member_is_the_masked_single_fit_readme_shape(family, kw):
    """3 455 guides x 6 replicates: seven members (the screen and six leave-one-out copies)."""
    data = make_sorting_variant_screen(3455, 6, seed=3, with_accessibility=bool(kw.get("scale_by_accessibility")))
    _check_members(family, data, _kw_of(kw, data))


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_member_is_the_masked_single_fit_ragged_tiles(family, kw):
    """1 003 guides, seven per target, with masked (replicate, guide) pairs and a masked sample already in the screen:
    the members' masks are the screen's own with one more replicate zeroed."""
    data = _ragged(with_accessibility=bool(kw.get("scale_by_accessibility")))
    assert not bool(data.repguide_mask.all()) and not bool((data.sample_mask != 0).all())
    _check_members(family, data, _kw_of(kw, data))


def test_windows_and_graph_chunks():
    data = _ragged().to(DEV)
    screens, _ = _screens(data)
    want = [_single("MixtureNormal", s, {}) for s in screens]
    for what, calls, chunk in (("windows", (100, 100, 100), 50), ("eager windows", (100, 100, 100), 0),
                               ("eager, one call", (STEPS,), 0), ("chunk 7", (100, 100, 100), 7)):
        ens, _ = _jackknife_engine("MixtureNormal", data, {})
        for n in calls:
            ens.run_ensemble(n, [SEED] * len(screens), graph_chunk=chunk)
        torch.cuda.synchronize()
        for k in range(len(screens)):
            _assert_same(_state(ens, k), want[k], f"{what} member {k}")
        ens.close()


def test_second_prepare_keeps_the_constants_and_null_masks_give_the_seed_ensemble_back():
    from bean_amd import engine

    data = _ragged().to(DEV)
    screens, _ = _screens(data)
    n = len(screens)
    want = [_single("MixtureNormal", s, {}) for s in screens]
    ens, _ = _jackknife_engine("MixtureNormal", data, {})
    initial = {id(t): t.clone() for d in (ens.unconstrained, ens._m, ens._v) for t in d.values()}

    def rewind():
        for d in (ens.unconstrained, ens._m, ens._v):
            for t in d.values():
                t.copy_(initial[id(t)])

    with ens._on_stream():
        ens._check(ens.lib.bean_hip_prepare(ens._h, ens._sptr()), "prepare")  # a second prepare
    ens.run_ensemble(STEPS, [SEED] * n, first_step=0)
    torch.cuda.synchronize()
    for k in range(n):
        _assert_same(_state(ens, k), want[k], f"after a second prepare, member {k}")
    # null for both: shared masks again, i.e. the seed ensemble (here with one seed for all: n times the plain fit)
    assert ens.lib.bean_hip_bind_member_masks(ens._h, None, 0, None, 0) == 0
    rewind()
    with pytest.raises(RuntimeError, match="prepare"):  # a bind of masks leaves the handle unprepared
        ens.run_ensemble(10, [SEED] * n, first_step=0)
    with ens._on_stream():
        ens._check(ens.lib.bean_hip_prepare(ens._h, ens._sptr()), "prepare")
    ens.run_ensemble(STEPS, [SEED] * n, first_step=0)
    torch.cuda.synchronize()
    for k in range(n):
        _assert_same(_state(ens, k), want[0], f"shared masks again, member {k}")
    ens.close()
    # and with seeds of their own: what an engine that never heard of member masks gives
    seeds = [SEED + k for k in range(n)]
    plain = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=n)
    plain.run_ensemble(STEPS, seeds)
    back, _ = _jackknife_engine("MixtureNormal", data, {})
    assert back.lib.bean_hip_bind_member_masks(back._h, None, 0, None, 0) == 0
    with back._on_stream():
        back._check(back.lib.bean_hip_prepare(back._h, back._sptr()), "prepare")
    back.run_ensemble(STEPS, seeds)
    torch.cuda.synchronize()
    for k in range(n):
        _assert_same(_state(back, k), _state(plain, k), f"seed ensemble after unbinding, member {k}")
    plain.close()
    back.close()


@pytest.mark.parametrize("family,kw", [("MixtureNormal", {}), ("Normal", {})])
def test_member_loss_constants(family, kw):
    """The members' losses of step 0 - same seed, same initial parameters, same draws - differ by what the masks take out
    of the loss, data-only constant included.  Against the float64 oracle on the draws of that step: each difference
    to 1e-9 of the loss, the loss tolerance of the parity tests (each member's loss is within that of its oracle)."""
    from bean_amd import engine
    from oracle import elbo, svi

    data = _ragged()
    screens, _ = _screens(data)
    one = engine.HipSVI(family, data.to(DEV), dump_noise=True, num_steps=STEPS, **kw)
    one.elbo_grad(step=0, seed=SEED)
    noise = {k: v.cpu() for k, v in one.drawn_noise().items()}
    params0 = {k: v.detach().cpu().double() for k, v in one.unconstrained.items()}
    one.close()
    ref = []
    for s in screens:
        params = {k: v.clone().requires_grad_(True) for k, v in params0.items()}
        ref.append(svi.loss_and_grads(elbo.LOSSES[family], elbo.as_float64(s), params, noise=noise, **kw)[0])
    ens, _ = _jackknife_engine(family, data.to(DEV), kw)
    ens.run_ensemble(1, [SEED] * len(screens))
    torch.cuda.synchronize()
    got = ens.losses()[:, 0]
    ens.close()
    print(f"{family}: step-0 losses {got.tolist()}, oracle {ref}")
    assert abs(got[0] - ref[0]) <= 1e-9 * abs(ref[0])
    assert len(set(got.tolist())) == len(got)  # every member has a loss of its own
    for k in range(1, len(screens)):
        d_got, d_ref = got[k] - got[0], ref[k] - ref[0]
        print(f"  member {k}: difference {d_got!r}, oracle {d_ref!r}, off by {abs(d_got - d_ref):.3e}")
        assert abs(d_ref) > 1e-3 * abs(ref[0])
        assert abs(d_got - d_ref) <= 1e-9 * min(abs(ref[k]), abs(ref[0])), (k, d_got, d_ref)


def test_engine_refuses_bad_member_masks_before_the_library():
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2).to(DEV)
    rg, sm = member_masks(data, [0, 1, 2])
    created = []
    lib = _lib.load()
    real = lib.bean_hip_create
    try:
        lib.bean_hip_create = lambda *a: (created.append(1), real(*a))[1]
        with pytest.raises(ValueError, match="n_members > 1"):
            engine.HipSVI("MixtureNormal", data, num_steps=10, member_masks=(rg[:1], sm[:1]))
        for bad in ((rg[:3], sm), (rg, sm[:, :, :-1]), (rg[:, :, :-1], sm), (rg.reshape(4, -1), sm)):
            with pytest.raises(ValueError, match="member_masks"):
                engine.HipSVI("MixtureNormal", data, num_steps=10, n_members=4, member_masks=bad)
        with pytest.raises(ValueError, match="pair"):
            engine.HipSVI("MixtureNormal", data, num_steps=10, n_members=4, member_masks=rg)
        assert created == []
    finally:
        lib.bean_hip_create = real
    # member_masks=None is the engine as it was
    eng = engine.HipSVI("MixtureNormal", data, num_steps=10, n_members=2)
    assert eng.member_masks is False
    eng.close()


def test_rejections_leave_the_handle_usable():
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2).to(DEV)
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    K = 4
    rg = torch.ones(K * R * G, dtype=torch.uint8, device=DEV)
    sm = torch.ones(K * R * B, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    # before bean_hip_set_members
    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    assert lib.bean_hip_bind_member_masks(eng._h, p(rg), R * G, p(sm), 8 * R * B) < 0 and "bean_hip_set_members first" in err()
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()

    # wrong byte counts, one mask without the other: refused naming K, nothing changes, the next valid calls work
    ens, screens = _jackknife_engine("MixtureNormal", data, {})
    assert len(screens) == K
    h = ens._h
    assert lib.bean_hip_bind_member_masks(h, p(rg), R * G, p(sm), 8 * K * R * B) < 0
    assert "repguide" in err() and "4 member" in err()
    assert lib.bean_hip_bind_member_masks(h, p(rg), K * R * G, p(sm), 8 * R * B) < 0
    assert "sample_mask" in err() and "4 member" in err()
    assert lib.bean_hip_bind_member_masks(h, p(rg), K * R * G, None, 0) < 0 and "go together" in err()
    ens.run_ensemble(50, [SEED] * K)  # still prepared, still on its own masks
    torch.cuda.synchronize()
    for k, s in enumerate(screens):
        _assert_same(_state(ens, k), _single("MixtureNormal", s, {}, steps=50), f"after refused binds, member {k}")
    ens.close()

    # a tiling handle
    til = engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10)
    assert lib.bean_hip_bind_member_masks(til._h, p(rg), K * R * G, p(sm), 8 * K * R * B) < 0
    assert "do not take this shape" in err()
    til.run(5, seed=SEED)  # still a working single-fit handle
    torch.cuda.synchronize()
    assert np.isfinite(til.losses()).all()
    til.close()


def test_run_inference_jackknife_batched_and_fallback(tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model import survival_model as sm
    from bean_amd.model.run import run_inference, run_inference_jackknife

    monkeypatch.chdir(tmp_path)

    def same(res, model, guide, data, n):
        full, loo, left_out = res
        assert left_out == list(range(data.n_reps)) and len(loo) == len(left_out)
        _same_results(full, run_inference(model, guide, data, num_steps=n, seed=7, verbose=False))
        for fit, r in zip(loo, left_out):
            _same_results(fit, run_inference(model, guide, leave_out(data, r), num_steps=n, seed=7, verbose=False))

    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble", lambda self, *a, **k: (used.append(a[0]), real(self, *a, **k))[1])
    var = make_sorting_variant_screen(640, 3, seed=2)
    mod, gd = partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)
    same(run_inference_jackknife(mod, gd, var, seed=7, num_steps=250, verbose=False), mod, gd, var, 250)
    assert used == [100, 100, 50]  # batched, in report windows
    used.clear()
    til = make_sorting_tiling_screen(200, 2, seed=2)
    mod, gd = partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide)
    same(run_inference_jackknife(mod, gd, til, seed=7, num_steps=120, verbose=False), mod, gd, til, 120)
    surv = make_survival_variant_screen(300, 2, seed=2)
    mod, gd = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)
    same(run_inference_jackknife(mod, gd, surv, seed=7, num_steps=120, verbose=False), mod, gd, surv, 120)
    assert used == []  # the fallback: one fit after the other
    # fewer than two candidates
    with pytest.raises(ValueError, match="found 1"):
        run_inference_jackknife(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide),
                                leave_out(leave_out(var, 0), 1), num_steps=10, verbose=False)


def test_run_inference_jackknife_halts_naming_the_replicate(tmp_path, monkeypatch):
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_jackknife

    data = make_sorting_variant_screen(2000, 3, seed=4)
    data.a0 = data.a0.clone()
    # a NaN the masks of replicates 1 and 2 do not hide: every member is NaN from step 0, the first one is named
    data.a0[17] = float("nan")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*the full screen \(seed 101\).*non-finite loss at iteration 0"):
        run_inference_jackknife(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, num_steps=1000,
                                verbose=False)
    with open(tmp_path / "tmp_result.full.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert dump["left_out"] is None and dump["seed"] == 101 and "mu_loc" in dump["param"]
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


def test_run_inference_jackknife_halts_naming_the_left_out_replicate(tmp_path, monkeypatch):
    """A member other than the full fit goes NaN (its parameters are poisoned behind the window's snapshot): message,
    file name and the dump's ``left_out`` carry the REPLICATE that member leaves out - here replicate 0 is masked from
    the start, so member 2 leaves out replicate 2 (not 1, its index among the left-out fits, and not 3)."""
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_jackknife

    data = leave_out(make_sorting_variant_screen(640, 4, seed=4), 0)
    assert candidate_replicates(data) == [1, 2, 3]
    real = engine.HipSVI.run_ensemble

    def poisoned(self, *a, **k):
        if self.steps_done == 0:
            self.unconstrained["mu_loc"][2, 4] = float("nan")
        return real(self, *a, **k)

    monkeypatch.setattr(engine.HipSVI, "run_ensemble", poisoned)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*replicate 2 left out \(seed 101\).*non-finite loss at iteration 0"):
        run_inference_jackknife(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, num_steps=300,
                                verbose=False)
    assert sorted(os.listdir(tmp_path)) == ["tmp_result.without_replicate2.pkl"]
    with open(tmp_path / "tmp_result.without_replicate2.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert dump["left_out"] == 2 and dump["seed"] == 101 and "mu_loc" in dump["param"]
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


def test_cli_jackknife_replicates(tmp_path):
    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    dj = _run(str(tmp_path / "jk"), *base, "--jackknife-replicates", "--save-raw")
    d0 = _run(str(tmp_path / "plain"), *base)
    name_el, name_sg = "bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"
    assert open(f"{dj}/{name_sg}", "rb").read() == open(f"{d0}/{name_sg}", "rb").read()
    plain_bytes = open(f"{d0}/{name_el}", "rb").read()
    assert _without_columns(f"{d0}/{name_el}", []) == plain_bytes  # (the cutting itself leaves a table's bytes alone)
    assert _without_columns(f"{dj}/{name_el}", COLUMNS) == plain_bytes
    el = pd.read_csv(f"{dj}/{name_el}")
    plain = pd.read_csv(f"{d0}/{name_el}")
    assert not set(COLUMNS) & set(plain.columns)
    assert [c for c in el.columns if c not in plain.columns] == COLUMNS
    assert len(el) == 6 and (el["mu_jk_se"] >= 0).all() and (el["mu_jk_se"] > 0).any()
    assert (el["mu_jk_max_shift"] >= 0).all() and np.isfinite(el[["mu_jk_se", "mu_jk_max_shift"]].values).all()
    with open(f"{dj}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    reps = [str(r) for r in dict.fromkeys(raw["data"].screen.samples["replicate"].astype(str))]
    assert len(reps) == raw["data"].n_reps >= 2
    assert set(el["mu_jk_max_shift_rep"].astype(str)) <= set(reps)
    assert (el["n_jk"] == len(reps)).all()
    assert [e["left_out"] for e in raw["jackknife"]] == reps  # one entry per replicate
    assert all(set(e) == {"left_out", "params", "loss"} and len(e["loss"]) == 200 for e in raw["jackknife"])
    # the pickle's main entries are the plain fit's; the left-out fits differ from it
    one = plain.sort_values("target")["mu"].values
    np.testing.assert_allclose(np.sort(one), np.sort(raw["params"]["mu_loc"].reshape(-1).numpy()), rtol=1e-6)
    assert not torch.equal(raw["jackknife"][0]["params"]["mu_loc"], raw["params"]["mu_loc"])
