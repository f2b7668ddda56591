"""Multi-particle SVI on the GPU.  A particle step is defined in include/bean_hip.h: every particle's
bean_hip_elbo_grad at the shared parameters, the float64 mean of the gradients in particle order, one bean_hip_adam.
Every comparison here is bitwise against that loop, written out below and driven on a single-fit engine through the
elbo_grad / adam entry points: parameters, both moments, the loss history and the bound gradients.  -m gpu."""
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
from bean_amd.model.jackknife import particle_seeds
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

from members_common import (CONFIGS, DEV, GOLD, VAR, _h5ad_reader_present, _kw_of, _mini, _run, _same_results)  # noqa: F401

pytestmark = pytest.mark.gpu
BW = os.path.join(GOLD, "accessibility_signal_chr6.bw")
ACC_ARGS = ["--scale-by-acc", "--acc-bw-path", BW, "--repguide-mask", "None"]
SEED = 101
STEPS = 300  # the schedule's length (lrd), not the number of steps a test runs


# ------------------------------------------------------------------ the definition
def _state(eng, first, n, grads=True):
    torch.cuda.synchronize()
    out = {f"{tag}.{k}": v.detach().clone() for tag, d in (("p", eng.unconstrained), ("m", eng._m), ("v", eng._v))
           for k, v in d.items()}
    if grads:
        out.update({f"g.{k}": v.detach().clone() for k, v in eng.grads.items()})
    out["loss"] = eng.loss_hist[first:first + n].clone()
    return out


def _load(eng, start):
    for tag, d in (("p", eng.unconstrained), ("m", eng._m), ("v", eng._v)):
        for k, v in d.items():
            v.copy_(start[f"{tag}.{k}"])


def _assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k, (got[k].double() - want[k].double()).abs().max().item())


def _defining_loop(eng, P, n, seed=SEED, first=0):
    """n particle steps on a SINGLE-FIT engine: what every path is compared with.  Leaves the mean losses in
    loss_hist[first : first + n]; the particles' own losses pass through the last slot."""
    seeds = particle_seeds(seed, P)
    spare = eng.loss_hist.numel() - 1
    assert first + n <= spare
    for s in range(first, first + n):
        grads, losses = [], []
        for sd in seeds:
            eng.elbo_grad(step=s, seed=sd, loss_index=spare)
            grads.append({k: v.clone() for k, v in eng.grads.items()})
            losses.append(eng.loss_hist[spare].clone())
        for k, dst in eng.grads.items():
            acc = grads[0][k].to(torch.float64)
            for g in grads[1:]:
                acc = acc + g[k].to(torch.float64)
            dst.copy_((acc * (1.0 / P)).to(torch.float32))
        eng.adam(s + 1)
        acc = losses[0]
        for l in losses[1:]:
            acc = acc + l
        eng.loss_hist[s] = acc * (1.0 / P)
    return _state(eng, first, n)


def _reference(family, data, kw, P, n, **loop_kw):
    from bean_amd import engine

    eng = engine.HipSVI(family, data, num_steps=STEPS, **kw)
    assert eng.n_particles == 1
    want = _defining_loop(eng, P, n, **loop_kw)
    eng.close()
    assert all(torch.isfinite(v).all() for v in want.values())
    return want


def _particles(family, data, kw, P, calls, chunk=50, native=True, **run_kw):
    from bean_amd import engine

    eng = engine.HipSVI(family, data, num_steps=STEPS, n_particles=P, **kw)
    assert eng._particles_native == native
    for name in eng.unconstrained:  # every tensor keeps its single-fit shape
        assert eng.grads[name].shape == eng.unconstrained[name].shape == eng._m[name].shape
    assert eng.loss_hist.dim() == 1
    first = run_kw.get("first_step", 0)
    for i, n in enumerate(calls):
        eng.run_particles(n, SEED, graph_chunk=chunk, **(run_kw if i == 0 else {}))
    assert eng.steps_done == first + sum(calls)
    got = _state(eng, first, sum(calls))
    eng.close()
    return got


# ------------------------------------------------------------------ screens
FAMILIES = [
    ("Normal", dict(), []),
    ("MixtureNormal", dict(), []),
    ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True), ACC_ARGS),
    ("MixtureNormal", dict(prior="yes"), []),
]
FAMILY_IDS = ["Normal", "MixtureNormal", "MixtureNormal+Acc+noise", "MixtureNormal+priors"]


def _screen(which, kw, tmp_path, cli_extra):
    acc = bool(kw.get("scale_by_accessibility"))
    if which == "ten tiles":
        data = make_sorting_variant_screen(640, 3, seed=2, with_accessibility=True)
    elif which == "ragged":
        # seven guides per target: targets cut by a tile end, a partial last tile, a short last target
        data = make_sorting_variant_screen(130, 2, guides_per_target=7, seed=3, with_accessibility=acc)
        assert data.n_guides % 64 and data.n_guides % 7 and int(data.target_lengths[-1]) < 7
    else:
        data = _mini(tmp_path, *cli_extra)
        assert (data.n_guides, data.n_targets) == (30, 6)
    return data.to(DEV)


# ------------------------------------------------------------------ 1. one particle is the single fit
@pytest.mark.parametrize("family,kw", CONFIGS)
def test_one_particle_is_the_single_fit(family, kw):
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2, with_accessibility=True).to(DEV)
    kw = _kw_of(kw, data)
    n = 70
    got = _particles(family, data, kw, 1, (n,), chunk=8)
    eng = engine.HipSVI(family, data, num_steps=STEPS, **kw)
    eng.run(n, seed=SEED)
    want = _state(eng, 0, n, grads=False)
    eng.close()
    got = {k: v for k, v in got.items() if not k.startswith("g.")}  # (run() leaves no gradients behind)
    _assert_same(got, want, (family, kw))


# ------------------------------------------------------------------ 2. P particles are the defining loop
@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("which", ["ten tiles", "ragged", "mini"])
@pytest.mark.parametrize("family,kw,cli_extra", FAMILIES, ids=FAMILY_IDS)
def test_particles_are_the_defining_loop(tmp_path, family, kw, cli_extra, which, P):
    data = _screen(which, kw, tmp_path, cli_extra)
    kw = _kw_of(kw, data)
    n = 40
    want = _reference(family, data, kw, P, n)
    got = _particles(family, data, kw, P, (n,))
    _assert_same(got, want, (family, which, P))
    # the particles are different draws: one particle alone gives another fit
    assert not torch.equal(want["p.mu_loc"], _particles(family, data, kw, 1, (n,))["p.mu_loc"])


# ------------------------------------------------------------------ 3. step counts and windows
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 33])
def test_step_counts_against_eager_launches(n):
    data = make_sorting_variant_screen(130, 2, guides_per_target=7, seed=3).to(DEV)
    want = _particles("MixtureNormal", data, {}, 3, (n,), chunk=1)
    assert torch.isfinite(want["loss"]).all() and want["loss"].numel() == n
    for chunk in (0, 4, 50):  # (0: no graph at all; 1 above: a graph per step)
        _assert_same(_particles("MixtureNormal", data, {}, 3, (n,), chunk=chunk), want, (n, chunk))
    if n == 5:
        _assert_same(want, _reference("MixtureNormal", data, {}, 3, n), "graph_chunk 1 against the loop")


def test_windows_are_one_call_and_the_slot_behind_stays():
    from bean_amd import engine

    data = make_sorting_variant_screen(130, 2, guides_per_target=7, seed=3).to(DEV)
    one = _particles("MixtureNormal", data, {}, 3, (40,))
    two = _particles("MixtureNormal", data, {}, 3, (25, 15))
    _assert_same(two, one, "25 + 15 steps against 40")
    _assert_same(one, _reference("MixtureNormal", data, {}, 3, 40), "40 steps against the loop")
    eng = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_particles=3)
    eng.loss_hist.fill_(-7.25)
    eng.run_particles(25, SEED)
    torch.cuda.synchronize()
    assert torch.equal(eng.loss_hist[:25], one["loss"][:25])
    assert bool((eng.loss_hist[25:] == -7.25).all())
    eng.run_particles(15, SEED)
    torch.cuda.synchronize()
    assert torch.equal(eng.loss_hist[:40], one["loss"]) and bool((eng.loss_hist[40:] == -7.25).all())
    assert eng.losses() == one["loss"].cpu().tolist()
    eng.close()


def test_particles_members_and_single_fit_share_one_handle():
    """The particles' arguments and the members' are both live on a particle handle: run_ensemble takes it as an ensemble
    of one, run as the single fit.  Five calls on ONE engine, each from step 0 and from the initial parameters and
    moments, each a ladder of its own (graph_chunk 4, 23 steps): every call gives the bits a fresh engine gives that
    makes that call alone, and the ensemble of one and the run are the single fit of their seed."""
    from bean_amd import engine

    data = make_sorting_variant_screen(130, 2, guides_per_target=7, seed=3).to(DEV)
    n, chunk = 23, 4
    calls = [
        ("particles", None, lambda e: e.run_particles(n, SEED, graph_chunk=chunk, first_step=0)),
        ("ensemble of one", SEED, lambda e: e.run_ensemble(n, [SEED], graph_chunk=chunk, first_step=0)),
        ("run", SEED, lambda e: e.run(n, seed=SEED, graph_chunk=chunk, first_step=0)),
        ("particles again", None, lambda e: e.run_particles(n, SEED, graph_chunk=chunk, first_step=0)),
        ("ensemble of one, another seed", 7, lambda e: e.run_ensemble(n, [7], graph_chunk=chunk, first_step=0)),
    ]

    def alone(call, **kw):
        eng = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, **kw)
        call(eng)
        out = _state(eng, 0, n, grads=False)
        eng.close()
        assert all(torch.isfinite(v).all() for v in out.values())
        return out

    fresh = [alone(call, n_particles=3) for _, _, call in calls]
    single = {seed: alone(lambda e, s=seed: e.run(n, seed=s, graph_chunk=chunk, first_step=0)) for seed in (SEED, 7)}

    eng = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_particles=3)
    assert eng._particles_native
    start = _state(eng, 0, 0, grads=False)
    got = []
    for what, seed, call in calls:
        _load(eng, start)
        call(eng)
        got.append(_state(eng, 0, n, grads=False))
        _assert_same(got[-1], fresh[len(got) - 1], f"{what}: on the shared handle against a fresh engine")
        if seed is not None:
            _assert_same(got[-1], single[seed], f"{what}: against the single fit of seed {seed}")
    eng.close()
    _assert_same(got[3], got[0], "the particles after the members' calls")
    assert not torch.equal(got[4]["p.mu_loc"], got[1]["p.mu_loc"]) and not torch.equal(got[4]["loss"], got[1]["loss"])
    assert not torch.equal(got[0]["p.mu_loc"], got[2]["p.mu_loc"])  # (three particles are not the single fit)


# ------------------------------------------------------------------ 4. started late in the schedule
def test_late_first_step_equals_the_defining_loop():
    """6 steps from first_step = 1500 of a 2000-step schedule, from the state a 5-step run leaves: the step size of
    update s + 1 comes from the device step counter k_particle_adam reads."""
    from bean_amd import engine

    data = make_sorting_variant_screen(600, 3, seed=73, mask_fraction=0.05).to(DEV)
    make = lambda **kw: engine.HipSVI("MixtureNormal", data, num_steps=2000, **kw)  # noqa: E731
    eng = make()
    eng.run(5, seed=9, graph_chunk=0)
    start = _state(eng, 0, 0, grads=False)
    eng.close()
    ref = make()
    _load(ref, start)
    want = _defining_loop(ref, 4, 6, first=1500)
    ref.close()
    assert any(not torch.equal(want[k], start[k]) for k in want if k.startswith("p."))
    for chunk in (0, 4):
        eng = make(n_particles=4)
        assert eng._particles_native
        _load(eng, start)
        eng.run_particles(6, SEED, graph_chunk=chunk, first_step=1500)
        _assert_same(_state(eng, 1500, 6), want, f"graph_chunk {chunk}")
        eng.close()


# ------------------------------------------------------------------ 5. the host loop gives the bits of the C entry point
def test_fallback_equals_batched(monkeypatch):
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2, with_accessibility=True).to(DEV)
    kw = dict(scale_by_accessibility=True, fit_noise=True)
    batched = _particles("MixtureNormal", data, kw, 3, (30,))
    monkeypatch.setattr(engine.HipSVI, "ensemble_supported", property(lambda self: False))
    looped = _particles("MixtureNormal", data, kw, 3, (30,), native=False)
    windows = _particles("MixtureNormal", data, kw, 3, (20, 10), native=False)
    _assert_same(looped, batched, "host loop against bean_hip_svi_run_particles")
    _assert_same(windows, batched, "host loop in windows")


# ------------------------------------------------------------------ 6. the other families go through the host loop
def _spy_on_entry_point(monkeypatch):
    called = []
    for build in _lib.ALL_BUILDS:
        lib = _lib.load(build)
        real = lib.bean_hip_svi_run_particles
        monkeypatch.setattr(lib, "bean_hip_svi_run_particles",
                            lambda *a, _real=real: (called.append(int(a[4])), _real(*a))[1])
    return called


def _models(which):
    from bean_amd.model import model as m
    from bean_amd.model import survival_model as sm

    if which == "tiling":
        return (partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide),
                make_sorting_tiling_screen(200, 2, seed=2))
    if which == "survival":
        return (partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide),
                make_survival_variant_screen(300, 2, seed=2))
    return partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), make_sorting_variant_screen(640, 3, seed=2)


@pytest.mark.parametrize("which", ["tiling", "survival", "sorting variant"])
def test_run_inference_particles(tmp_path, monkeypatch, which):
    from bean_amd.model import run as model_run

    monkeypatch.chdir(tmp_path)
    model, guide, data = _models(which)
    n = 20
    plain = model_run.run_inference(model, guide, data, num_steps=n, verbose=False)
    _same_results(model_run.run_inference(model, guide, data, num_steps=n, verbose=False, num_particles=1), plain)

    built = []
    real_build = model_run.build_engine
    monkeypatch.setattr(model_run, "build_engine", lambda *a, **k: (built.append((a, k)), real_build(*a, **k))[1])
    called = _spy_on_entry_point(monkeypatch)
    store, out = model_run.run_inference(model, guide, data, num_steps=n, verbose=False, num_particles=2)
    assert called == ([n] if which == "sorting variant" else [])
    (args, kwargs), = built
    assert kwargs.pop("n_particles") == 2
    ref = real_build(*args, **kwargs)  # the engine run_inference builds, as a single fit
    assert ref.n_particles == 1 and ref.ensemble_supported == (which == "sorting variant")
    want = _defining_loop(ref, 2, n)
    assert out["loss"] == want["loss"].cpu().tolist() and out["loss"] != plain[1]["loss"]
    constrained = ref.constrained()
    ref.close()
    assert set(out["params"]) == set(constrained) == set(store.keys())
    for k, v in constrained.items():
        assert torch.equal(out["params"][k], v.cpu()) and torch.equal(store[k].cpu(), v.cpu()), (which, k)
    assert not torch.equal(out["params"]["mu_loc"], plain[1]["params"]["mu_loc"])


def test_member_entry_points_do_not_take_the_argument():
    from bean_amd.model import run as model_run

    for fn in (model_run.run_inference_ensemble, model_run.run_inference_jackknife,
               model_run.run_inference_guide_jackknife, model_run.run_inference_sample_jackknife):
        with pytest.raises(TypeError, match="num_particles"):
            fn(None, None, None, num_particles=2)


# ------------------------------------------------------------------ 7. halt
def test_halt_on_a_non_finite_window(tmp_path, monkeypatch):
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference

    data = make_sorting_variant_screen(2000, 3, seed=4)
    data.a0 = data.a0.clone()
    data.a0[17] = float("nan")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*non-finite loss at iteration 0"):
        run_inference(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, num_steps=1000, verbose=False,
                      num_particles=2)
    with open(tmp_path / "tmp_result.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert set(dump) == {"param"} and "mu_loc" in dump["param"]
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


# ------------------------------------------------------------------ 8. rejections
def test_rejections_leave_the_handle_usable():
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2).to(DEV)
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)

    def fresh():
        h = ctypes.c_void_p()
        assert lib.bean_hip_create(ctypes.byref(eng._shape), ctypes.byref(h)) == 0
        return h

    # a fresh handle, nothing bound yet: P < 1 and P above the cap are refused, a valid P is then accepted
    h = fresh()
    for bad in (0, -3, _lib.MAX_MEMBERS + 1):
        assert lib.bean_hip_set_particles(h, bad) < 0 and "n_particles" in err(), bad
    assert lib.bean_hip_set_particles(h, 2) == 0
    assert lib.bean_hip_set_particles(h, _lib.MAX_MEMBERS) == 0
    assert lib.bean_hip_set_particles(h, 3) == 0
    # ... the caller's buffers keep their single-fit sizes
    buf = torch.zeros(3 * data.n_targets, dtype=torch.float32, device=DEV)
    assert lib.bean_hip_bind(h, _lib.BUF["P"], ctypes.c_void_p(buf.data_ptr()), 12 * data.n_targets) < 0
    assert "1 member" in err()
    assert lib.bean_hip_bind(h, _lib.BUF["P"], ctypes.c_void_p(buf.data_ptr()), 4 * data.n_targets) == 0
    assert lib.bean_hip_set_particles(h, 2) < 0 and "before any bean_hip_bind" in err()  # after a bind
    assert lib.bean_hip_destroy(h) == 0

    # members and particles: whichever comes second is refused
    h = fresh()
    assert lib.bean_hip_set_members(h, 2) == 0
    assert lib.bean_hip_set_particles(h, 2) < 0 and "bean_hip_set_members" in err()
    assert lib.bean_hip_set_members(h, 1) == 0
    assert lib.bean_hip_set_particles(h, 3) == 0
    assert lib.bean_hip_set_members(h, 2) < 0 and "bean_hip_set_particles" in err()
    assert lib.bean_hip_set_members(h, 1) == 0  # (an ensemble of one is the fit itself)
    assert lib.bean_hip_set_particles(h, 1) == 0
    assert lib.bean_hip_set_members(h, 2) == 0
    assert lib.bean_hip_destroy(h) == 0
    eng.close()
    with pytest.raises(ValueError, match="n_members == 1"):
        engine.HipSVI("MixtureNormal", data, num_steps=50, n_members=2, n_particles=2)
    for bad in (0, -3, _lib.MAX_MEMBERS + 1):
        with pytest.raises(ValueError, match="n_particles must be in"):
            engine.HipSVI("MixtureNormal", data, num_steps=50, n_particles=bad)

    # a tiling shape
    til = engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10)
    assert lib.bean_hip_set_particles(til._h, 2) < 0 and "do not take this shape" in err()
    seeds = (ctypes.c_uint64 * 2)(1, 2)
    assert lib.bean_hip_svi_run_particles(til._h, seeds, 2, 0, 5, 0, til._sptr()) < 0 and "bean_hip_set_particles first" in err()
    til.run(5, seed=101)  # still a working single-fit handle
    torch.cuda.synchronize()
    assert np.isfinite(til.losses()).all()
    til.close()

    # the wrong number of seeds, null seeds, injected noise: nothing runs, the next valid call does
    par = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_particles=2)
    before = _state(par, 0, 0)
    three = (ctypes.c_uint64 * 3)(1, 2, 3)
    assert lib.bean_hip_svi_run_particles(par._h, three, 3, 0, 10, 0, par._sptr()) < 0 and "3 seeds for 2 particle" in err()
    assert lib.bean_hip_svi_run_particles(par._h, None, 2, 0, 10, 0, par._sptr()) < 0 and "null seeds" in err()
    par.set_noise({"eps_mu": torch.zeros(data.n_targets)})
    assert lib.bean_hip_svi_run_particles(par._h, seeds, 2, 0, 10, 0, par._sptr()) < 0 and "noise" in err()
    with pytest.raises(RuntimeError, match="injected or dumped noise"):
        par.run_particles(10, SEED)
    _assert_same(_state(par, 0, 0), before, "after the refusals")
    par.set_noise(None)
    par.run_particles(10, SEED)
    _assert_same(_state(par, 0, 10), _reference("MixtureNormal", data, {}, 2, 10), "after the refusals, a valid call")
    par.close()


# ------------------------------------------------------------------ 9. the particles are independent draws
def test_gradient_noise_falls_as_one_over_p():
    """One step's mu_loc gradient at the initial parameters, over 64 base seeds: the per-target sample variances at
    P = 8, summed, are 1/8 of those at P = 1 in expectation.  Each sum is a chi-square estimate over 63 x 128 degrees
    of freedom (about 2 % under Gaussian tails), so a factor of two either way is more than ten standard deviations;
    particles that share a stream give a ratio of 1, a sum in place of the mean gives 8."""
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2, with_accessibility=True).to(DEV)
    assert data.n_targets == 128
    var = {}
    for P in (1, 8):
        eng = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_particles=P)
        assert eng._particles_native
        start = _state(eng, 0, 0, grads=False)
        grads = []
        for base in range(64):
            _load(eng, start)
            eng.run_particles(1, 5000 + base, first_step=0)
            torch.cuda.synchronize()
            grads.append(eng.grads["mu_loc"].reshape(-1).double().clone())
        eng.close()
        var[P] = float(torch.stack(grads).var(0, unbiased=True).sum())
    ratio = var[8] / var[1]
    print(f"summed per-target variance of d loss / d mu_loc: P = 1 {var[1]:.6g}, P = 8 {var[8]:.6g}, ratio {ratio:.4f}")
    assert 0.06 < ratio < 0.25, ratio


# ------------------------------------------------------------------ 10. CLI
def test_cli_num_particles(tmp_path, monkeypatch):
    from bean_amd.cli.execute import get_parser
    from bean_amd.model.run import identify_model_guide, run_inference

    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    d4 = _run(str(tmp_path / "p4"), *base, "--num-particles", "4", "--save-raw")
    d1 = _run(str(tmp_path / "p1"), *base)
    for name in ("bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"):
        got, plain = pd.read_csv(f"{d4}/{name}"), pd.read_csv(f"{d1}/{name}")
        assert list(got.columns) == list(plain.columns) and len(got) == len(plain), name
    el = pd.read_csv(f"{d4}/bean_element_result.MixtureNormal.csv")
    assert len(el) == 6 and np.isfinite(el[["mu", "mu_sd", "mu_z", "sd"]].values).all()
    assert not np.array_equal(el.sort_values("target")["mu"].values,
                              pd.read_csv(f"{d1}/bean_element_result.MixtureNormal.csv").sort_values("target")["mu"].values)
    with open(f"{d4}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    assert set(raw) == {"data", "params", "loss"}  # the layout of a run without the flag
    args = get_parser().parse_args(["run", *base, "--num-particles", "4"])
    _, model, guide = identify_model_guide(args)
    monkeypatch.chdir(tmp_path)
    _, want = run_inference(model, guide, _mini(tmp_path / "data"), num_steps=200, verbose=False, num_particles=4)
    assert raw["loss"] == want["loss"] and len(raw["loss"]) == 200
    assert set(raw["params"]) == set(want["params"])
    for k, v in want["params"].items():
        assert torch.equal(raw["params"][k], v), k
