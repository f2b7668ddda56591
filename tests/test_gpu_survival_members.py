"""Survival member fits on the GPU: K fits of one survival variant screen in the same launches (csrc/bean_survival_ensemble.hpp,
bean_hip_survival_members_supported) against single fits - seeds, windows, members with counts and masks of their own, a
diverged member, the admission and its refusals, and run_survival_bootstrap's batched refits.  Every comparison is
torch.equal on the parameters, both Adam moments and the loss history.  The screens: 130 guides (3 tiles, the last with 2
valid lanes, in a grid padded to 8; one gamma block), 300 guides (5 tiles, 2 gamma blocks: the last-arrival hand-over has
a partner) and 130 guides at 3 timepoints (the two-per-pass loop has a lone last timepoint).  -m gpu."""
import copy
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.preprocessing.synthetic import make_survival_tiling_screen, make_survival_variant_screen

from members_common import DEV, _assert_same, _h5ad_reader_present, _same_results, _state  # noqa: F401

pytestmark = pytest.mark.gpu
DEPTH = 17.0
K = 3
SEEDS = (101, 7, 55)
STEPS = 60
CAP = 80
T3 = (0.0, 7.0, 14.0)

FAMILIES = [("Normal", dict()), ("MixtureNormal", dict()),
            ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True))]
IDS = ["Normal", "MixtureNormal", "MixtureNormal+Acc"]
SHAPE_REFUSAL = ("bean_hip_set_members: the batched kernels do not take this shape (bean_hip_ensemble_supported): "
                 "fit its seeds one after the other")


@pytest.fixture(scope="module")
def screens():
    def make(n, acc, **kw):
        return make_survival_variant_screen(n, 2, depth_per_guide=DEPTH, mask_fraction=0.05, seed=11,
                                            with_accessibility=acc, **kw)

    out = {}
    for acc in (False, True):
        tag = "acc" if acc else ""
        out["130" + tag] = make(130, acc)
        out["300" + tag] = make(300, acc)
    out["130t3"] = make(130, False, times=T3)
    assert out["130t3"].n_condits == 3 and out["130"].n_condits == 6
    return out


def _pick(screens, size, kw):
    return screens[size + ("acc" if kw.get("scale_by_accessibility") else "")]


def _engine(family, data, kw, **more):
    from bean_amd import engine

    return engine.HipSVI(family, data.to(DEV), num_steps=CAP, **kw, **more)


_singles = {}


def _single(family, which, data, kw, seed, calls=(STEPS,), **run_kw):
    """The single fit a member is compared with: computed once per (screen, family, seed, windows), never modified."""
    key = (family, which, tuple(sorted(kw.items())), seed, tuple(calls), tuple(sorted(run_kw.items())))
    if key not in _singles:
        eng = _engine(family, data, kw)
        for i, n in enumerate(calls):
            eng.run(n, seed=seed, resume=i > 0, **run_kw)
        torch.cuda.synchronize()
        _singles[key] = _state(eng)
        eng.close()
    return _singles[key]


# ------------------------------------------------------------------ 1. seeds
CASES = [(f, kw, s) for f, kw in FAMILIES for s in ("130", "300")] + [("MixtureNormal", dict(), "130t3")]
CASE_IDS = [f"{i}-{s}" for i in IDS for s in ("130", "300")] + ["MixtureNormal-130t3"]


@pytest.mark.parametrize("family,kw,size", CASES, ids=CASE_IDS)
def test_member_is_the_single_fit(screens, family, kw, size):
    data = screens[size] if size == "130t3" else _pick(screens, size, kw)
    want = [_single(family, size, data, kw, s) for s in SEEDS]
    for chunk in (25, 0):  # the graph ladder (25 + 25 + eager rest), and eager launches
        ens = _engine(family, data, kw, n_members=K)
        assert ens.survival_members_supported and not ens.ensemble_supported
        ens.run_ensemble(STEPS, SEEDS, graph_chunk=chunk)
        torch.cuda.synchronize()
        assert ens.losses().shape == (K, STEPS) and np.isfinite(ens.losses()).all()
        for k in range(K):
            _assert_same(_state(ens, k), want[k], f"chunk {chunk} member {k}")
        assert not torch.equal(ens.unconstrained["mu_loc"][0], ens.unconstrained["mu_loc"][1])
        ens.close()


# ------------------------------------------------------------------ 2. windows
@pytest.mark.parametrize("family,kw", FAMILIES, ids=IDS)
def test_windows_give_the_bits_of_one_call(screens, family, kw):
    data = _pick(screens, "130", kw)
    ens = _engine(family, data, kw, n_members=K)
    ens.run_ensemble(25, SEEDS, graph_chunk=25)
    ens.run_ensemble(15, SEEDS, graph_chunk=25)
    one = _engine(family, data, kw, n_members=K)
    one.run_ensemble(40, SEEDS, graph_chunk=25)
    torch.cuda.synchronize()
    for k in range(K):
        _assert_same(_state(ens, k), _state(one, k), f"windows against one call, member {k}")
        _assert_same(_state(ens, k), _single(family, "130", data, kw, SEEDS[k], calls=(25, 15)),
                     f"windows against the single fit's resumed windows, member {k}")
    ens.close()
    one.close()


# ------------------------------------------------------------------ 3. counts of their own
@pytest.mark.parametrize("use_bc", [True, False], ids=["bcmatch", "no-bcmatch"])
@pytest.mark.parametrize("family,kw", FAMILIES, ids=IDS)
def test_members_with_their_own_counts(screens, family, kw, use_bc):
    data = _pick(screens, "130", kw)
    kw = dict(kw, use_bcmatch=use_bc)
    src = _engine(family, data, kw)
    torch.manual_seed(3)
    for v in src.unconstrained.values():  # parameters a fit could have reached, not the initial ones
        v.add_(0.3 * torch.randn_like(v))
    sim = src.simulate_survival_members(0, 3)
    torch.cuda.synchronize()
    planes = {k: v.clone() for k, v in sim.items()}
    src.close()
    assert set(planes) == ({"X", "X_bcmatch"} if use_bc else {"X"})
    x = torch.cat([data.X_masked.to(DEV, torch.float32)[None], planes["X"]])
    x_bc = torch.cat([data.X_bcmatch_masked.to(DEV, torch.float32)[None], planes["X_bcmatch"]]) if use_bc else None
    seeds = (101, 7, 55, 101)
    ens = _engine(family, data, kw, n_members=4, member_counts=(x, x_bc))
    ens.run_ensemble(STEPS, seeds, graph_chunk=25)
    torch.cuda.synchronize()
    for k in range(4):
        screen = data
        if k:
            screen = copy.copy(data)
            screen.X_masked = planes["X"][k - 1].cpu()
            if use_bc:
                screen.X_bcmatch_masked = planes["X_bcmatch"][k - 1].cpu()
        one = _engine(family, screen, kw)
        one.run(STEPS, seed=seeds[k])
        torch.cuda.synchronize()
        _assert_same(_state(ens, k), _state(one), f"member {k} with its own counts")
        one.close()
    assert not torch.equal(ens.loss_hist[0, :STEPS], ens.loss_hist[3, :STEPS])  # same seed, other counts
    ens.close()


# ------------------------------------------------------------------ 4. masks of their own
def test_a_member_with_its_own_masks(screens):
    from bean_amd.model.jackknife import leave_out, member_masks

    data = screens["130"]
    ens = _engine("MixtureNormal", data, {}, n_members=2, member_masks=member_masks(data, [1]))
    ens.run_ensemble(STEPS, (101, 101), graph_chunk=25)
    torch.cuda.synchronize()
    _assert_same(_state(ens, 0), _single("MixtureNormal", "130", data, {}, 101), "the screen itself")
    one = _engine("MixtureNormal", leave_out(data, 1), {})
    one.run(STEPS, seed=101)
    torch.cuda.synchronize()
    _assert_same(_state(ens, 1), _state(one), "replicate 1 masked")
    assert not torch.equal(ens.loss_hist[0, :STEPS], ens.loss_hist[1, :STEPS])
    one.close()
    ens.close()


# ------------------------------------------------------------------ 5. a diverged member stays alone
@pytest.mark.parametrize("family,kw", FAMILIES[:2], ids=IDS[:2])
def test_a_diverged_member_stays_alone(screens, family, kw):
    data = screens["300"]
    ens = _engine(family, data, kw, n_members=K)
    ens.unconstrained["mu_loc"][1, 4] = float("nan")
    ens.run_ensemble(STEPS, SEEDS, graph_chunk=25)
    torch.cuda.synchronize()
    assert np.isnan(ens.losses()[1]).all()
    for k in (0, 2):
        _assert_same(_state(ens, k), _single(family, "300", data, kw, SEEDS[k]), f"member {k} beside a NaN member")
    ens.close()


# ------------------------------------------------------------------ 6. admission and refusals
def test_admission_and_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine, parallel
    from bean_amd.engine import EnsembleUnsupported, PredictiveUnsupported

    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731

    def still_fits(eng):
        eng.run(5, seed=101)
        torch.cuda.synchronize()
        assert np.isfinite(np.asarray(eng.losses())).all()

    for family, kw in FAMILIES:
        eng = _engine(family, _pick(screens, "130", kw), kw)
        assert eng.survival_members_supported and lib.bean_hip_survival_members_supported(eng._h) == 1
        assert not eng.ensemble_supported and lib.bean_hip_ensemble_supported(eng._h) == 0
        assert not eng._particles_native
        assert lib.bean_hip_set_particles(eng._h, 2) < 0
        assert err() == ("bean_hip_set_particles: the batched kernels do not take this shape (bean_hip_ensemble_supported): "
                         "step its particles one after the other"), err()
        still_fits(eng)
        eng.close()

    # shapes the survival member kernels do not take: tiling, the negative-control model, a guide shard
    surv = make_survival_variant_screen(400, 2, seed=5, depth_per_guide=DEPTH)
    ctrl = surv[surv.negctrl_guide_idx]
    tiling = make_survival_tiling_screen(200, 2, seed=2)
    shard = parallel.plan_shards(surv.target_lengths.numpy(), 2)[1]
    assert shard[0] > 0
    others = [("MultiMixtureNormal", tiling, {}), ("ControlNormal", ctrl, {}),
              ("Normal", parallel.shard_screen(surv, shard),
               dict(guide_offset=shard[0], target_offset=shard[2], n_guides_total=surv.n_guides))]
    for family, data, kw in others:
        eng = engine.HipSVI(family, data.to(DEV), num_steps=10, **kw)
        assert eng.survival and not eng.survival_members_supported and not eng.ensemble_supported
        assert lib.bean_hip_set_members(eng._h, 2) < 0
        assert err() == SHAPE_REFUSAL, err()
        with pytest.raises(EnsembleUnsupported, match=family):
            engine.HipSVI(family, data.to(DEV), num_steps=10, n_members=2, **kw)
        still_fits(eng)
        eng.close()

    # an exchange buffer would be one buffer for all members
    data = screens["130"]
    ens = _engine("MixtureNormal", data, {}, n_members=2)
    ens.exchange_buffers()
    assert "XCHG_GSUM" in ens._keep
    two = (ctypes.c_uint64 * 2)(101, 7)
    assert lib.bean_hip_svi_run_ensemble(ens._h, two, 2, 0, 5, 0, ens._sptr()) < 0
    assert err().startswith("bean_hip_svi_run_ensemble: BEAN_BUF_XCHG_GSUM is bound: 2 survival members would share"), err()
    with pytest.raises(RuntimeError, match="BEAN_BUF_XCHG_GSUM is bound"):
        ens.run_ensemble(5, (101, 7))
    torch.cuda.synchronize()
    assert ens.steps_done == 0 and bool((ens.loss_hist == 0).all())  # nothing was launched
    # the count simulator still wants one member
    with pytest.raises(PredictiveUnsupported, match="one member"):
        ens.simulate_survival(0)
    with pytest.raises(PredictiveUnsupported, match="one member"):
        ens.simulate_survival_members(0, 2)
    ens._bind_slot(_lib.BUF["XCHG_GSUM"], None, "XCHG_GSUM")
    ens.run_ensemble(5, (101, 7))
    torch.cuda.synchronize()
    assert ens.losses().shape == (2, 5) and np.isfinite(ens.losses()).all()
    want = _engine("MixtureNormal", data, {})
    want.run(5, seed=7)
    torch.cuda.synchronize()
    _assert_same(_state(ens, 1), _state(want), "after the refusals")
    want.close()
    ens.close()


# ------------------------------------------------------------------ 7. the run layer
@pytest.mark.parametrize("family", ["MixtureNormal", "Normal"])
def test_run_survival_bootstrap_refits_as_members(family, tmp_path, monkeypatch):
    import bean_amd.model.survival_model as sm
    from bean_amd import engine
    from bean_amd.model.run import (run_inference, run_inference_ensemble, run_survival_bootstrap,
                                    survival_bootstrap_engine, survival_bootstrap_screens)

    monkeypatch.chdir(tmp_path)
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble",
                        lambda self, *a, **k: (used.append((self.n_members, a[0])), real(self, *a, **k))[1])
    data = make_survival_variant_screen(128, 2, depth_per_guide=DEPTH, seed=2, mask_fraction=0.05)
    if family == "MixtureNormal":
        model, guide = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)
    else:
        model, guide = partial(sm.NormalModel), sm.NormalGuide
    full, boots = run_survival_bootstrap(model, guide, data, n_boot=K, seed=101, boot_seed=7, num_steps=40, verbose=False)
    assert used == [(K + 1, 40)]  # the screen as member 0 and the K refits, one report window
    used.clear()
    _same_results(full, run_inference(model, guide, data, seed=101, num_steps=40, verbose=False))
    eng = survival_bootstrap_engine(model, guide, data, full[0])
    try:
        x, x_bc = survival_bootstrap_screens(eng, K, boot_seed=7)
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert len(boots) == K
    for j in range(K):
        screen = copy.copy(data)
        screen.X_masked = x[j].cpu()
        screen.X_bcmatch_masked = x_bc[j].cpu()
        _same_results(boots[j], run_inference(model, guide, screen, seed=101, num_steps=40, verbose=False))
    # the seed ensemble of a survival screen still goes one fit after the other
    res = run_inference_ensemble(model, guide, data, [101, 7], num_steps=40, verbose=False)
    assert used == [] and len(res) == 2
    _same_results(res[0], full)
