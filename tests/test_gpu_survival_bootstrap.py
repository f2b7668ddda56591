"""The survival bootstrap on the GPU: K screens of a survival fit in one launch (bean_hip_simulate_survival_members,
csrc/bean_survival_predictive.hpp) against the single draws of bean_hip_simulate_survival - which draw is whose - their
batching, totals, odd and large numbers of timepoints, the state the call must leave alone, its refusals, and
run_survival_bootstrap and `bean run --survival-bootstrap` end to end.  The screens have depth_per_guide = 17: totals
near 100.  -m gpu."""
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
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen, make_survival_variant_screen

from members_common import DEV, GOLD, _h5ad_reader_present, _run, _same_results, _state, _without_columns  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = 101
DEPTH = 17.0
BIG = 5003   # one pair's total inside a wave of totals near 100
G_BIG, G_ZERO, R_EDIT = 70, 75, 1  # both in the second tile of replicate 1
K = 3
SURV = os.path.join(GOLD, "survival_var_mini_screen.h5ad")
T3 = (0.0, 7.0, 14.0)
T36 = tuple(0.5 * t for t in range(36))
NAME = "bean_hip_simulate_survival_members"

FAMILIES = [("Normal", dict()), ("MixtureNormal", dict()),
            ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True))]
IDS = ["Normal", "MixtureNormal", "MixtureNormal+Acc"]


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
def screens():
    # 130 guides: the last of the three tiles has 2 valid lanes
    make = lambda acc: make_survival_variant_screen(130, 2, depth_per_guide=DEPTH, with_accessibility=acc, seed=11,  # noqa: E731
                                                    mask_fraction=0.05)
    return {"130": _edited(make(False)), "130acc": _edited(make(True))}


def _which(kw):
    return "130acc" if kw.get("scale_by_accessibility") else "130"


def _observed(eng):
    out = {"X": eng._keep["X"]}
    if eng.use_bcmatch:
        out["X_bcmatch"] = eng._keep["X_BC"]
    return out


def _engine(family, data, kw, steps=50, move=True, **more):
    from bean_amd import engine

    eng = engine.HipSVI(family, data.to(DEV), num_steps=steps, **kw, **more)
    if move:  # parameters a fit could have reached, not the initial ones
        torch.manual_seed(3)
        for v in eng.unconstrained.values():
            v.add_(0.3 * torch.randn_like(v))
    return eng


def _plug_in(eng, data):
    """The sites survival_bootstrap_engine injects: zeros into the Normal sites (mu and the guide noise: survival has no sd site), q_0 at the mean of its Dirichlet."""
    zeros = lambda n: torch.zeros(int(n), dtype=torch.float64, device=DEV)  # noqa: E731
    noise = {"eps_mu": zeros(eng.T)}
    if eng.scale_by_accessibility:
        noise["eps_noise"] = zeros(data.n_guides)
    if eng.surv_normal:
        ia = eng.constrained()["initial_abundance"].double().reshape(-1)
        noise["q_0"] = (ia / ia.sum()).expand(data.n_reps, data.n_guides).contiguous()
    return noise


def _same_planes(many, singles, what):
    """Plane k of ``many`` is ``singles[k]``, bit for bit, in every likelihood."""
    for k, one in enumerate(singles):
        assert set(one) == set(many), what
        for key in one:
            assert many[key].shape[1:] == one[key].shape
            assert torch.equal(many[key][k], one[key]), (what, key, k, int((many[key][k] != one[key]).sum()))


def _check_totals(eng, many):
    obs = _observed(eng)
    assert set(many) == set(obs)
    for key, x in many.items():
        assert x.dtype == torch.float32 and x.shape[1:] == obs[key].shape
        assert bool((x >= 0).all()) and bool((x == x.round()).all()), key
        want = obs[key].double().sum(1)
        for k in range(x.shape[0]):  # every pair keeps its observed total, in every member
            assert torch.equal(x[k].double().sum(1), want), (key, k)


# ------------------------------------------------------------------ 1. planes are the single draws
@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("family,kw", FAMILIES, ids=IDS)
def test_planes_are_the_single_draws(screens, family, kw, first):
    data = screens[_which(kw)]
    eng = _engine(family, data, kw)
    try:
        assert eng.survival_predictive_supported
        # nothing injected: plane 0 is the single draw; the shared sites of the other planes are draw `first`'s
        many = eng.simulate_survival_members(first, K, seed=SEED)
        single = [eng.simulate_survival(first + k, seed=SEED) for k in range(K)]
        torch.cuda.synchronize()
        assert set(many) == {"X", "X_bcmatch"} and many["X"].shape == (K,) + tuple(single[0]["X"].shape)
        _same_planes(many, single[:1], "nothing injected")
        for key in many:
            assert not torch.equal(many[key][1], single[1][key])  # mu_t of plane 1 is draw `first`'s, not first + 1's
            assert not torch.equal(many[key][1], many[key][0]) and not torch.equal(many[key][2], many[key][1])
        # the plug-in's sites injected, eps_u not: every plane is the single draw - the baseline u_g of member k is the
        # one PREP draws at step first + k
        eng.set_noise(_plug_in(eng, data))
        many = eng.simulate_survival_members(first, K, seed=SEED)
        single = [eng.simulate_survival(first + k, seed=SEED) for k in range(K)]
        torch.cuda.synchronize()
        _same_planes(many, single, "plug-in")
        _check_totals(eng, many)
        for key in many:
            assert not torch.equal(many[key][1], many[key][0]), key
        if family == "MixtureNormal":
            # an injected baseline is every member's
            g = torch.Generator().manual_seed(9)
            eps_u = torch.randn(data.n_guides, generator=g, dtype=torch.float64)
            eng.set_noise({**_plug_in(eng, data), "eps_u": eps_u})
            given = eng.simulate_survival_members(first, K, seed=SEED)
            single = [eng.simulate_survival(first + k, seed=SEED) for k in range(K)]
            torch.cuda.synchronize()
            _same_planes(given, single, "plug-in + eps_u")
            for key in many:
                for k in range(K):
                    assert not torch.equal(given[key][k], many[key][k]), (key, k)
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. batching, totals
@pytest.mark.parametrize("family,kw", FAMILIES, ids=IDS)
def test_batching_and_totals(screens, family, kw):
    data = screens[_which(kw)]
    eng = _engine(family, data, kw)
    try:
        obs = _observed(eng)
        n = obs["X"].double().sum(1)
        assert float(n[R_EDIT, G_BIG]) == BIG and float(n[R_EDIT, G_ZERO]) == 0 and bool((n % 4 != 0).any())
        assert 50 < float(n[R_EDIT, 64:128].median()) < 200  # the deep pair sits in a wave of totals near 100
        masked = ~eng._keep["REPGUIDE"].bool()
        assert bool(masked.any()) and float(eng._keep["SAMPLE_MASK"].min()) == 0  # masks present
        eng.set_noise(_plug_in(eng, data))
        five = eng.simulate_survival_members(0, 5, seed=SEED)
        three = eng.simulate_survival_members(2, 3, seed=SEED)
        again = eng.simulate_survival_members(0, 5, seed=SEED)
        other_seed = eng.simulate_survival_members(0, 5, seed=SEED + 1)
        torch.cuda.synchronize()
        _check_totals(eng, five)
        for key in five:
            assert torch.equal(five[key][2:5], three[key]), key  # screen j is draw j whatever the batching
            assert torch.equal(five[key], again[key]), key
            assert not torch.equal(five[key], other_seed[key]), key
            assert float(five[key][:, R_EDIT, :, G_ZERO].abs().sum()) == 0, key
            # masked pairs are drawn like any other
            drawn = five[key].double().sum(2)[:, masked.reshape(n.shape)]
            assert drawn.numel() and float(drawn.sum()) > 0, key
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. odd B, large B
@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
@pytest.mark.parametrize("gen_kw,k", [
    (dict(n_guides=90, n_reps=2, times=T3), 3),    # odd B: the lone last bin of the gamma pairs
    (dict(n_guides=64, n_reps=1, times=T36), 2),   # 36 timepoints: the smallest B whose columns take more than 64 KB of LDS
], ids=["3-timepoints", "36-timepoints"])
def test_planes_at_other_numbers_of_timepoints(family, gen_kw, k):
    lds = lambda b: (4 * b + 3 * b * 64) * 8 + b * 64 * 4  # noqa: E731  simulate_survival_lds (bean_survival_predictive.hpp)
    data = make_survival_variant_screen(seed=4, depth_per_guide=DEPTH, mask_fraction=0.05 if gen_kw["n_reps"] > 1 else 0.0,
                                        **gen_kw)
    B = len(gen_kw["times"])
    assert data.n_condits == B
    if B == 36:
        assert lds(35) <= 65536 < lds(36)
    eng = _engine(family, data, dict())
    try:
        eng.set_noise(_plug_in(eng, data))
        many = eng.simulate_survival_members(1, k, seed=SEED)
        single = [eng.simulate_survival(1 + j, seed=SEED) for j in range(k)]
        torch.cuda.synchronize()
        _same_planes(many, single, f"{B} timepoints")
        _check_totals(eng, many)
        assert not torch.equal(many["X"][0], many["X"][1])
    finally:
        eng.close()


# ------------------------------------------------------------------ 4. the fit is left alone
def test_simulate_survival_members_leaves_the_fit_alone(screens):
    from bean_amd import engine

    data = screens["130"].to(DEV)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(20, seed=SEED)
    torch.cuda.synchronize()
    before = _state(eng)
    hist = eng.loss_hist.clone()
    eng.simulate_survival_members(2, K, seed=7)
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
            x = torch.empty((K,) + tuple(e._keep["X"].shape), dtype=torch.float32, device=DEV)
            xbc = torch.empty_like(x)
            nb = x.numel() * 4
            assert e.lib.bean_hip_simulate_survival_members(e._h, SEED + 5, 1, K, ctypes.c_void_p(x.data_ptr()), nb,
                                                            ctypes.c_void_p(xbc.data_ptr()), nb, e._sptr()) == 0
        elif simulate_first:
            e.simulate_survival_members(1, K, seed=SEED + 5)
        e.run(40, seed=SEED, resume=resume)
        torch.cuda.synchronize()
        st = _state(e)
        e.close()
        return st

    plain, simulated = fit(False, False), fit(True, False)
    for k in plain:
        assert torch.equal(plain[k], simulated[k]), k
    # a resumed window after the call does not step on the simulator's draw: it is a plain run
    plain = fit(False, True)
    for how in (True, "raw"):
        simulated = fit(how, True)
        for k in plain:
            assert torch.equal(plain[k], simulated[k]), (how, k)


# ------------------------------------------------------------------ 5. refusals
ADMIT = (NAME + ": the survival count simulator does not take this handle (bean_hip_survival_predictive_supported): "
         "survival variant Normal / MixtureNormal, unsharded, no sample covariates, one member, one particle")
FILL = -7.0


def test_refusals_are_pinned_and_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["130"]
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    n = K * R * B * G
    x = torch.full((n,), FILL, dtype=torch.float32, device=DEV)
    xbc = torch.full((n,), FILL, dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def refused(handle, stream, message, k, *a):
        assert lib.bean_hip_simulate_survival_members(handle, SEED, 0, k, *a, stream) < 0
        assert err() == message, err()
        torch.cuda.synchronize()
        for t in (x, xbc):  # nothing was launched
            assert bool((t == FILL).all())

    good = (p(x), 4 * n, p(xbc), 4 * n)
    refused(None, None, NAME + ": null handle", K, *good)

    # handles of other shapes: a sorting screen, the negative-control model of a survival screen
    sorting = make_sorting_variant_screen(130, 2, seed=11, depth_per_guide=DEPTH)
    surv = make_survival_variant_screen(400, 2, seed=5, depth_per_guide=DEPTH)
    ctrl = surv[surv.negctrl_guide_idx]
    others = [(engine.HipSVI("MixtureNormal", sorting.to(DEV), num_steps=10), sorting),
              (engine.HipSVI("ControlNormal", ctrl.to(DEV), num_steps=10), ctrl)]
    for other, scr in others:
        size = K * scr.n_reps * scr.n_condits * scr.n_guides
        assert size <= n and not other.survival_predictive_supported
        refused(other._h, other._sptr(), ADMIT, K, p(x), 4 * size, p(xbc), 4 * size)
        refused(other._h, other._sptr(), ADMIT, 0, None, 0, None, 0)  # the admission comes before range and buffers
        with pytest.raises(PredictiveUnsupported, match=other.family) as exc:
            other.simulate_survival_members(0, K)
        with pytest.raises(PredictiveUnsupported) as exc1:
            other.simulate_survival(0)
        assert str(exc.value) == str(exc1.value)  # simulate_survival's own sentence
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(other.loss_hist[:5]).all())
        other.close()

    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
    s = eng._sptr()
    for bad in (0, -1, 65):
        refused(eng._h, s, NAME + f": n_draws must be in [1, 64], got {bad}", bad, *good)
        refused(eng._h, s, NAME + f": n_draws must be in [1, 64], got {bad}", bad, None, 0, None, 0)  # ... before the buffers
    held = f"(K, R, B, G) float32 with K = {K}, {4 * n} bytes"
    x_msg = NAME + ": x_out must hold " + held
    bc_msg = NAME + ": this handle uses the barcode-matched counts: xbc_out must hold " + held
    refused(eng._h, s, x_msg, K, p(x), 4 * n - 4, p(xbc), 4 * n)
    refused(eng._h, s, x_msg, K, p(x), 4 * n + 4, p(xbc), 4 * n)
    refused(eng._h, s, x_msg, K, None, 0, p(xbc), 4 * n)
    refused(eng._h, s, x_msg, K, None, 4 * n, p(xbc), 4 * n)
    refused(eng._h, s, bc_msg, K, p(x), 4 * n, p(xbc), 4 * n + 4)
    refused(eng._h, s, bc_msg, K, p(x), 4 * n, None, 0)
    refused(eng._h, s, bc_msg, K, p(x), 4 * n, None, 4 * n)
    two = 4 * 2 * R * B * G  # the byte count follows K
    refused(eng._h, s, NAME + f": x_out must hold (K, R, B, G) float32 with K = 2, {two} bytes", 2, *good)
    with pytest.raises(RuntimeError, match=r"n_draws must be in \[1, 64\], got 65"):
        eng.simulate_survival_members(0, 65)
    assert lib.bean_hip_simulate_survival_members(eng._h, SEED, 0, K, *good, s) == 0
    torch.cuda.synchronize()
    assert float(x.sum()) == K * float(eng._keep["X"].sum()) and float(xbc.sum()) == K * float(eng._keep["X_BC"].sum())
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()
    x.fill_(FILL), xbc.fill_(FILL)

    nobc = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50, use_bcmatch=False)
    no_bc = NAME + ": xbc_out on a handle without BEAN_FLAG_USE_BCMATCH"
    refused(nobc._h, nobc._sptr(), no_bc, K, p(x), 4 * n, p(xbc), 4 * n)
    refused(nobc._h, nobc._sptr(), no_bc, K, p(x), 4 * n, None, 4)
    refused(nobc._h, nobc._sptr(), no_bc, K, p(x), 4 * n, p(xbc), 0)
    assert set(nobc.simulate_survival_members(0, K)) == {"X"}
    # an unprepared handle of the same shape
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(nobc._shape), ctypes.byref(h)) == 0
    refused(h, None, NAME + ": call bean_hip_prepare first", K, p(x), 4 * n, None, 0)
    refused(h, None, NAME + ": call bean_hip_prepare first", 0, None, 0, p(xbc), 4)  # ... before range and buffers
    assert lib.bean_hip_destroy(h) == 0
    nobc.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(nobc.losses()).all()
    nobc.close()


# ------------------------------------------------------------------ 6. the run layer
@pytest.mark.parametrize("family", ["MixtureNormal", "Normal"])
def test_run_survival_bootstrap(family):
    import bean_amd.model.survival_model as sm
    from bean_amd.model.jackknife import bootstrap_summary
    from bean_amd.model.run import (run_inference, run_survival_bootstrap, survival_bootstrap_engine,
                                    survival_bootstrap_screens)

    data = make_survival_variant_screen(128, 2, depth_per_guide=DEPTH, seed=2, mask_fraction=0.05)
    if family == "MixtureNormal":
        model, guide = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)
    else:
        model, guide = partial(sm.NormalModel), sm.NormalGuide
    kept = {k: getattr(data, k).clone() for k in ("X", "X_masked", "X_bcmatch", "X_bcmatch_masked")}
    full, boots = run_survival_bootstrap(model, guide, data, n_boot=K, seed=SEED, boot_seed=7, num_steps=40, verbose=False)
    for k, v in kept.items():  # the screen is not modified
        assert torch.equal(getattr(data, k), v), k
    want_full = run_inference(model, guide, data, seed=SEED, num_steps=40, verbose=False)
    _same_results(full, want_full)
    eng = survival_bootstrap_engine(model, guide, data, full[0])
    try:
        assert "EPS_MU_IN" in eng._keep and "EPS_U_IN" not in eng._keep  # the baseline is left to the kernel
        x, x_bc = survival_bootstrap_screens(eng, K, boot_seed=7)
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert len(boots) == K
    for j in range(K):
        screen = copy.copy(data)
        screen.X_masked = x[j].cpu()
        screen.X_bcmatch_masked = x_bc[j].cpu()
        _same_results(boots[j], run_inference(model, guide, screen, seed=SEED, num_steps=40, verbose=False))
    assert not torch.equal(boots[0][0]["mu_loc"].cpu(), boots[1][0]["mu_loc"].cpu())
    summ = bootstrap_summary(full, boots)
    se = summ["mu_boot_se"].reshape(-1).cpu()
    assert summ["n_boot"] == K and se.shape == (data.n_targets,)
    # a target with an edited guide: one of its guides shows edited reads at the control timepoint and enters the
    # likelihood with mu (the NormalModel forces mu of negative-control guides to 0: their mu_loc follows the prior alone
    # and is the same in every refit)
    edited = data.allele_counts_control[..., 1].sum((0, 1)) > 0
    if family == "Normal" and data.negctrl_guide_idx is not None:
        edited[torch.as_tensor(data.negctrl_guide_idx, dtype=torch.long)] = False
    has = torch.zeros(data.n_targets, dtype=torch.bool)
    has[data.guide_to_target.long()[edited]] = True
    print(f"{family}: {int(has.sum())} of {data.n_targets} targets with an edited guide; mu_boot_se "
          f"min {float(se[has].min()):.3e} max {float(se[has].max()):.3e}")
    assert int(has.sum()) > data.n_targets // 2
    assert bool(torch.isfinite(se[has]).all()) and bool((se[has] > 0).all())


# ------------------------------------------------------------------ 7. CLI
COLUMNS = ["mu_boot_se", "mu_boot_bias", "n_boot"]


def test_cli_survival_bootstrap(tmp_path, capsys):
    from bean_amd.cli.execute import main as bean_main

    base = ["survival", "variant", SURV, "--n-iter", "50", "--control-condition=D7"]
    db = _run(str(tmp_path / "boot"), *base, "--survival-bootstrap", "3", "--save-raw")
    d0 = _run(str(tmp_path / "plain"), *base, "--save-raw")
    dz = _run(str(tmp_path / "zero"), *base, "--survival-bootstrap", "0", "--save-raw")
    name_el, name_raw = "bean_element_result.MixtureNormal.csv", "MixtureNormal.result.pkl"
    names = sorted(os.listdir(d0))
    assert name_el in names and name_raw in names and "bean_sgRNA_result.MixtureNormal.csv" in names
    assert sorted(os.listdir(db)) == names == sorted(os.listdir(dz))
    load = lambda path: pickle.load(open(path, "rb"))  # noqa: E731
    for name in names:
        plain = open(f"{d0}/{name}", "rb").read()
        if name == "bean_run.log":  # (time stamps)
            continue
        if name in (name_raw, "ndata.pkl"):
            continue
        assert open(f"{dz}/{name}", "rb").read() == plain, name  # 0 is off
        if name == name_el:
            assert _without_columns(f"{db}/{name}", COLUMNS) == plain
        else:  # every other file is what it is without the flag
            assert open(f"{db}/{name}", "rb").read() == plain, name
    el, plain = pd.read_csv(f"{db}/{name_el}"), pd.read_csv(f"{d0}/{name_el}")
    assert [c for c in el.columns if c not in plain.columns] == COLUMNS
    # (this screen lists var_1 under two groups: its target table has one row more than the fit has targets, whose fitted
    # columns are empty with and without the flag)
    fitted = el["mu"].notna()
    assert int(fitted.sum()) == len(el) - 1 == 13 and plain["mu"].notna().equals(fitted)
    assert np.isfinite(el.loc[fitted, COLUMNS].values.astype(float)).all() and (el["n_boot"] == 3).all()
    assert el.loc[~fitted, ["mu_boot_se", "mu_boot_bias"]].isna().all().all()
    assert (el.loc[fitted, "mu_boot_se"] >= 0).all() and (el.loc[fitted, "mu_boot_se"] > 0).any()
    raw, raw0, rawz = load(f"{db}/{name_raw}"), load(f"{d0}/{name_raw}"), load(f"{dz}/{name_raw}")
    assert set(raw) == set(raw0) | {"bootstrap"} and set(rawz) == set(raw0) and "bootstrap" not in raw0
    for k in raw0["params"]:
        assert torch.equal(raw["params"][k], raw0["params"][k]) and torch.equal(rawz["params"][k], raw0["params"][k]), k
    assert raw["loss"] == raw0["loss"] == rawz["loss"]
    entries = raw["bootstrap"]
    assert len(entries) == 3 and [e["screen"] for e in entries] == [0, 1, 2]
    assert all(set(e) == {"screen", "params", "loss"} and len(e["loss"]) == 50 for e in entries)
    assert not torch.equal(entries[0]["params"]["mu_loc"], raw["params"]["mu_loc"])
    with pytest.raises(SystemExit) as exc:
        bean_main(["run", "sorting", "variant", os.path.join(GOLD, "var_mini_screen.h5ad"), "--survival-bootstrap", "3",
                   "-o", str(tmp_path / "sorting")])
    assert exc.value.code == 2
    msg = " ".join(capsys.readouterr().err.split())
    assert "--survival-bootstrap" in msg and "sorting screens (--bootstrap serves them)" in msg
