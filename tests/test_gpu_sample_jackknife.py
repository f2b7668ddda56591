"""Sample jackknife on the GPU: a member with its own sample mask AND its own counts is, bit for bit, the single fit of the
screen with that sample left out - parameters, both moments and the loss history - for every sorting variant family the
batched kernels take; the masks alone do not give that fit; windows, eager launches, a second prepare, the return to
shared counts; the C entry point's rejections; run_inference_sample_jackknife batched, in several runs and in its
fallback; the CLI; and a planted bad sample that the influence table puts first.  -m gpu."""
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
from bean_amd.model.jackknife import (leave_out_samples, sample_groups, sample_jackknife_summary, sample_member_counts,
                                      sample_member_masks)
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

from members_common import (CONFIGS, DEV, SEED, STEPS, VAR, _assert_same, _h5ad_reader_present, _kw_of, _mini,  # noqa: F401
                            _run, _same_results, _single, _state, _without_columns)

pytestmark = pytest.mark.gpu
COLUMNS = ["mu_sjk_max_shift", "mu_sjk_max_shift_sample", "n_sjk"]


def _same(got, want):
    return set(got) == set(want) and all(got[k].shape == want[k].shape and torch.equal(got[k], want[k]) for k in want)


def _counts(data, groups, kw):
    x, xbc = sample_member_counts(data, groups)
    return x, (xbc if kw.get("use_bcmatch", True) else None)


def _engine(family, data, groups, kw, counts=True, **extra):
    from bean_amd import engine

    if counts:
        extra["member_counts"] = _counts(data, groups, kw)
    eng = engine.HipSVI(family, data, num_steps=STEPS, n_members=1 + len(groups),
                        member_masks=sample_member_masks(data, groups), **kw, **extra)
    assert eng.ensemble_supported and eng.member_masks and eng.member_counts is bool(counts)
    return eng


def _check_members(family, data, kw, by):
    data = data.to(DEV)
    groups, _ = sample_groups(data, by)
    screens = [data] + [leave_out_samples(data, g) for g in groups]
    n = len(screens)
    ens = _engine(family, data, groups, kw)
    ens.run_ensemble(STEPS, [SEED] * n)
    torch.cuda.synchronize()
    losses = ens.losses()
    assert losses.shape == (n, STEPS) and np.isfinite(losses).all()
    members = [_state(ens, k) for k in range(n)]
    ens.close()
    for k, screen in enumerate(screens):
        what = "the plain fit" if k == 0 else f"{groups[k - 1]} left out"
        _assert_same(members[k], _single(family, screen, kw), f"{family} {kw} member {k} ({what})")
    for k in range(1, n):
        # masking a sample really changes the fit ...
        assert not torch.equal(members[k]["p.mu_loc"], members[0]["p.mu_loc"]), k
        # ... and its loss from step 0 on, far beyond rounding: the member's own data-only constant (the log-factorials of
        # the sample's counts leave it) next to the likelihood terms that go
        l0, lk = float(members[0]["loss"][0]), float(members[k]["loss"][0])
        assert abs(lk - l0) > 1e-6 * abs(l0), (k, l0, lk)
    return n


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_member_is_the_single_fit_by_sample(family, kw):
    """640 guides x 3 replicates x 5 conditions: sixteen members (the screen and fifteen leave-one-sample-out copies)."""
    data = make_sorting_variant_screen(640, 3, seed=2, with_accessibility=bool(kw.get("scale_by_accessibility")))
    assert _check_members(family, data, _kw_of(kw, data), "sample") == 1 + data.n_reps * data.n_condits


@pytest.mark.parametrize("family,kw", CONFIGS)
def test_member_is_the_single_fit_by_condition_ragged_tiles(family, kw):
    """1 003 guides, seven per target (a tile boundary inside a target, a partial last tile): six members, each
    leaving one condition of every replicate out."""
    data = make_sorting_variant_screen(1003, 3, seed=9, guides_per_target=7,
                                       with_accessibility=bool(kw.get("scale_by_accessibility")))
    assert _check_members(family, data, _kw_of(kw, data), "condition") == 1 + data.n_condits


@pytest.mark.parametrize("extra,family", [([], "MixtureNormal"), (["--uniform-edit"], "Normal")])
def test_member_is_the_single_fit_mini_screen(tmp_path, extra, family):
    """The 30-guide fixture every reference test runs: 6 targets, i.e. the wide-target (generic) k_param."""
    data = _mini(tmp_path, *extra)
    assert data.n_guides == 30 and data.n_targets == 6
    _check_members(family, data, {}, "sample")


def test_the_masks_alone_are_not_the_left_out_fit():
    """Why the counts are needed: with the member masks but shared counts, the member that masks sample (1, 2) is not the
    single fit of the screen with that sample left out (the guide kernel sums every bin's count whatever sample_mask
    says, and the loss constant keeps the sample's log-factorials); with its own counts it is."""
    data = make_sorting_variant_screen(640, 3, seed=2).to(DEV)
    groups = [[(1, 2)], [(0, 0)]]
    want = _single("MixtureNormal", leave_out_samples(data, groups[0]), {})
    masks_only = _engine("MixtureNormal", data, groups, {}, counts=False)
    masks_only.run_ensemble(STEPS, [SEED] * 3)
    torch.cuda.synchronize()
    got = _state(masks_only, 1)
    masks_only.close()
    assert np.isfinite(got["loss"].cpu().numpy()).all()
    assert not _same(got, want)
    assert not torch.equal(got["p.mu_loc"], want["p.mu_loc"]) and not torch.equal(got["loss"], want["loss"])
    both = _engine("MixtureNormal", data, groups, {})
    both.run_ensemble(STEPS, [SEED] * 3)
    torch.cuda.synchronize()
    _assert_same(_state(both, 1), want, "with member counts")
    both.close()


def test_run_modes_second_prepare_and_the_return_to_shared_counts():
    data = make_sorting_variant_screen(1003, 3, seed=9, guides_per_target=7).to(DEV)
    groups, _ = sample_groups(data, "condition")
    screens = [data] + [leave_out_samples(data, g) for g in groups]
    n = len(screens)
    want = [_single("MixtureNormal", s, {}) for s in screens]
    for what, calls, chunk in (("windows", (100, 100, 100), 50), ("eager windows", (100, 100, 100), 0),
                               ("eager, one call", (STEPS,), 0), ("chunk 7", (100, 100, 100), 7)):
        ens = _engine("MixtureNormal", data, groups, {})
        for steps in calls:
            ens.run_ensemble(steps, [SEED] * n, graph_chunk=chunk)
        torch.cuda.synchronize()
        for k in range(n):
            _assert_same(_state(ens, k), want[k], f"{what} member {k}")
        ens.close()

    ens = _engine("MixtureNormal", data, groups, {})
    initial = {id(t): t.clone() for d in (ens.unconstrained, ens._m, ens._v) for t in d.values()}

    def rewind():
        for d in (ens.unconstrained, ens._m, ens._v):
            for t in d.values():
                t.copy_(initial[id(t)])

    def prepare():
        with ens._on_stream():
            ens._check(ens.lib.bean_hip_prepare(ens._h, ens._sptr()), "prepare")

    # the counts bound again, then a second prepare
    x, xbc = ens._keep["MEMBER_X"], ens._keep["MEMBER_X_BC"]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert ens.lib.bean_hip_bind_member_counts(ens._h, p(x), x.numel() * 4, p(xbc), xbc.numel() * 4) == 0
    with pytest.raises(RuntimeError, match="prepare"):  # a bind of counts leaves the handle unprepared
        ens.run_ensemble(10, [SEED] * n, first_step=0)
    prepare()
    ens.run_ensemble(STEPS, [SEED] * n, first_step=0)
    torch.cuda.synchronize()
    for k in range(n):
        _assert_same(_state(ens, k), want[k], f"after rebinding and a second prepare, member {k}")
    # null / null: shared counts again; with the masks unbound too every member is the plain fit
    assert ens.lib.bean_hip_bind_member_counts(ens._h, None, 0, None, 0) == 0
    assert ens.lib.bean_hip_bind_member_masks(ens._h, None, 0, None, 0) == 0
    rewind()
    with pytest.raises(RuntimeError, match="prepare"):
        ens.run_ensemble(10, [SEED] * n, first_step=0)
    prepare()
    ens.run_ensemble(STEPS, [SEED] * n, first_step=0)
    torch.cuda.synchronize()
    for k in range(n):
        _assert_same(_state(ens, k), want[0], f"shared counts and masks again, member {k}")
    ens.close()


def test_counts_without_masks():
    """Either may be bound: members with their own counts and the shared masks are the single fits of the screen with
    those counts (here: member 1 has the counts of replicate 0 and 1 swapped)."""
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2).to(DEV)
    other = copy.copy(data)
    other.X_masked = data.X_masked[[1, 0, 2]].contiguous()
    other.X_bcmatch_masked = data.X_bcmatch_masked[[1, 0, 2]].contiguous()
    counts = (torch.stack([data.X_masked, other.X_masked]), torch.stack([data.X_bcmatch_masked, other.X_bcmatch_masked]))
    ens = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=2, member_counts=counts)
    assert ens.member_counts and not ens.member_masks
    ens.run_ensemble(STEPS, [SEED] * 2)
    torch.cuda.synchronize()
    _assert_same(_state(ens, 0), _single("MixtureNormal", data, {}), "member 0")
    _assert_same(_state(ens, 1), _single("MixtureNormal", other, {}), "member 1")
    ens.close()


def test_rejections_leave_the_handle_usable():
    from bean_amd import engine

    data = make_sorting_variant_screen(640, 3, seed=2).to(DEV)
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    lib = _lib.load()
    bind = lib.bean_hip_bind_member_counts
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    groups = [[(1, 2)], [(0, 0)], [(2, 4)]]
    K = 4
    one = 4 * R * B * G
    x = torch.ones(K * R * B * G, dtype=torch.float32, device=DEV)
    xbc = torch.ones(K * R * B * G, dtype=torch.float32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    assert bind(None, p(x), K * one, p(xbc), K * one) < 0 and "null handle" in err()

    # before bean_hip_set_members
    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    assert bind(eng._h, p(x), one, p(xbc), one) < 0 and "bean_hip_set_members first" in err()
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()

    # wrong byte counts, x_bcmatch missing, x missing: refused naming K, nothing changes, the next valid calls work
    ens = _engine("MixtureNormal", data, groups, {})
    h = ens._h
    assert bind(h, p(x), one, p(xbc), K * one) < 0 and "x expects" in err() and "4 member" in err()
    assert bind(h, p(x), K * one, p(xbc), one) < 0 and "x_bcmatch expects" in err() and "4 member" in err()
    assert bind(h, p(x), K * one, None, 0) < 0 and "x_bcmatch is required" in err()
    assert bind(h, None, 0, p(xbc), K * one) < 0 and "x_bcmatch without x" in err()
    ens.run_ensemble(50, [SEED] * K)  # still prepared, still on its own counts
    torch.cuda.synchronize()
    for k, s in enumerate([data] + [leave_out_samples(data, g) for g in groups]):
        _assert_same(_state(ens, k), _single("MixtureNormal", s, {}, steps=50), f"after refused binds, member {k}")
    ens.close()

    # a handle that does not use the barcode-matched counts
    kw = {"use_bcmatch": False}
    ens = _engine("MixtureNormal", data, groups, kw)
    assert bind(ens._h, p(x), K * one, p(xbc), K * one) < 0 and "x_bcmatch must be null" in err()
    ens.run_ensemble(50, [SEED] * K)
    torch.cuda.synchronize()
    _assert_same(_state(ens, 1), _single("MixtureNormal", leave_out_samples(data, groups[0]), kw, steps=50), "no bcmatch")
    ens.close()

    # a tiling handle
    til = engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10)
    assert bind(til._h, p(x), K * one, p(xbc), K * one) < 0 and "do not take this shape" in err()
    til.run(5, seed=SEED)  # still a working single-fit handle
    torch.cuda.synchronize()
    assert np.isfinite(til.losses()).all()
    til.close()


# ---------------------------------------------------------------- run_inference_sample_jackknife


def _as_run_inference(res, model, guide, data, n, by):
    from bean_amd.model.run import run_inference

    full, loo, groups, names = res
    want_groups, want_names = sample_groups(data, by)
    assert groups == want_groups and names == want_names and len(loo) == len(groups)
    _same_results(full, run_inference(model, guide, data, num_steps=n, seed=7, verbose=False))
    for fit, g in zip(loo, groups):
        _same_results(fit, run_inference(model, guide, leave_out_samples(data, g), num_steps=n, seed=7, verbose=False))


def test_run_inference_sample_jackknife_batched_and_in_several_runs(tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_sample_jackknife

    monkeypatch.chdir(tmp_path)
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble",
                        lambda self, *a, **k: (used.append((self.n_members, a[0])), real(self, *a, **k))[1])
    var = make_sorting_variant_screen(640, 3, seed=2)
    mod, gd = partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)
    one = run_inference_sample_jackknife(mod, gd, var, seed=7, num_steps=250, verbose=False)
    assert used == [(16, 100), (16, 100), (16, 50)]  # batched, one engine, in report windows
    _as_run_inference(one, mod, gd, var, 250, "sample")
    used.clear()
    parts = run_inference_sample_jackknife(mod, gd, var, seed=7, num_steps=250, verbose=False, max_groups_per_run=5)
    assert [k for k, _ in used] == [6] * 9  # three runs of five groups next to the full screen
    assert parts[2] == one[2] and parts[3] == one[3]
    _same_results(parts[0], one[0])
    for a, b in zip(parts[1], one[1]):
        _same_results(a, b)
    by_condition = run_inference_sample_jackknife(mod, gd, var, by="condition", seed=7, num_steps=250, verbose=False)
    assert len(by_condition[1]) == var.n_condits and by_condition[3] == [f"c{b}" for b in range(var.n_condits)]
    _same_results(by_condition[0], one[0])
    with pytest.raises(ValueError, match="max_groups_per_run"):
        run_inference_sample_jackknife(mod, gd, var, num_steps=10, verbose=False, max_groups_per_run=64)


def test_run_inference_sample_jackknife_fallback(tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model import survival_model as sm
    from bean_amd.model.run import run_inference_sample_jackknife

    monkeypatch.chdir(tmp_path)
    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble", lambda self, *a, **k: (used.append(a[0]), real(self, *a, **k))[1])
    til = make_sorting_tiling_screen(200, 2, seed=2)
    mod, gd = partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide)
    _as_run_inference(run_inference_sample_jackknife(mod, gd, til, by="condition", seed=7, num_steps=120, verbose=False),
                      mod, gd, til, 120, "condition")
    surv = make_survival_variant_screen(300, 2, seed=2)
    mod, gd = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)
    _as_run_inference(run_inference_sample_jackknife(mod, gd, surv, by="condition", seed=7, num_steps=120, verbose=False),
                      mod, gd, surv, 120, "condition")
    assert used == []  # the fallback: one fit after the other


def test_run_inference_sample_jackknife_halts_naming_the_full_screen(tmp_path, monkeypatch):
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_sample_jackknife

    data = make_sorting_variant_screen(640, 3, seed=2)
    data.a0 = data.a0.clone()
    data.a0[17] = float("nan")  # a NaN no left-out sample hides: every member is NaN from step 0, the first one is named
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*the full screen \(seed 101\).*non-finite loss at iteration 0"):
        run_inference_sample_jackknife(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, num_steps=300,
                                       verbose=False)
    assert sorted(os.listdir(tmp_path)) == ["tmp_result.full.pkl"]
    with open(tmp_path / "tmp_result.full.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert dump["left_out"] is None and dump["seed"] == 101 and "mu_loc" in dump["param"]
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


def test_run_inference_sample_jackknife_halts_naming_the_left_out_sample(tmp_path, monkeypatch):
    """A member other than the full fit goes NaN (its parameters are poisoned behind the window's snapshot): message, file
    name and the dump's ``left_out`` carry the sample that member leaves out."""
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_sample_jackknife

    data = make_sorting_variant_screen(640, 3, seed=2)
    real = engine.HipSVI.run_ensemble

    def poisoned(self, *a, **k):
        if self.steps_done == 0:
            self.unconstrained["mu_loc"][8, 4] = float("nan")  # member 8 leaves out group 7 = (1, 2)
        return real(self, *a, **k)

    monkeypatch.setattr(engine.HipSVI, "run_ensemble", poisoned)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*sample r1_c2 left out \(seed 101\).*non-finite loss at iteration 0"):
        run_inference_sample_jackknife(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, num_steps=300,
                                       verbose=False)
    assert sorted(os.listdir(tmp_path)) == ["tmp_result.without_r1_c2.pkl"]
    with open(tmp_path / "tmp_result.without_r1_c2.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert dump["left_out"] == [[1, 2]] and dump["seed"] == 101
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


# ---------------------------------------------------------------- CLI


def test_cli_jackknife_samples(tmp_path):
    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    dj = _run(str(tmp_path / "sjk"), *base, "--jackknife-samples", "--save-raw")
    d0 = _run(str(tmp_path / "plain"), *base)
    name_el, name_sg = "bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"
    name_inf = "bean_sample_influence.MixtureNormal.csv"
    assert open(f"{dj}/{name_sg}", "rb").read() == open(f"{d0}/{name_sg}", "rb").read()
    plain_bytes = open(f"{d0}/{name_el}", "rb").read()
    assert _without_columns(f"{d0}/{name_el}", []) == plain_bytes  # (the cutting itself leaves a table's bytes alone)
    assert _without_columns(f"{dj}/{name_el}", COLUMNS) == plain_bytes
    assert not os.path.exists(f"{d0}/{name_inf}")
    el = pd.read_csv(f"{dj}/{name_el}")
    plain = pd.read_csv(f"{d0}/{name_el}")
    assert [c for c in el.columns if c not in plain.columns] == COLUMNS
    with open(f"{dj}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    ndata = raw["data"]
    R, B = ndata.n_reps, ndata.n_condits
    sample_names = [str(s) for s in ndata.screen.samples.index]
    assert len(sample_names) == R * B
    assert len(el) == 6 and (el["mu_sjk_max_shift"] > 0).all() and np.isfinite(el["mu_sjk_max_shift"].values).all()
    assert (el["n_sjk"] == R * B).all() and set(el["mu_sjk_max_shift_sample"].astype(str)) <= set(sample_names)
    inf = pd.read_csv(f"{dj}/{name_inf}")
    assert list(inf.columns) == ["left_out", "n_samples", "influence_median", "influence_max", "n_targets_moved"]
    assert inf["left_out"].astype(str).tolist() == sample_names  # the row the tensor builder put at (r, b), in (r, b) order
    assert (inf["n_samples"] == 1).all() and (inf["influence_max"] >= inf["influence_median"]).all()
    assert (inf["influence_median"] >= 0).all() and (inf["n_targets_moved"].between(0, 6)).all()
    entries = raw["sample_jackknife"]
    assert [e["left_out"] for e in entries] == sample_names
    assert [e["pairs"] for e in entries] == [[[r, b]] for r in range(R) for b in range(B)]
    assert all(set(e) == {"left_out", "pairs", "params", "loss"} and len(e["loss"]) == 200 for e in entries)
    assert not torch.equal(entries[0]["params"]["mu_loc"], raw["params"]["mu_loc"])
    # the summary the tables hold is that of the stored fits
    again = sample_jackknife_summary(raw["params"], [e["params"] for e in entries], [e["pairs"] for e in entries], sample_names)
    np.testing.assert_allclose(sorted(again["mu_sjk_max_shift"].reshape(-1).tolist()), sorted(el["mu_sjk_max_shift"]), rtol=1e-12)
    np.testing.assert_allclose(again["influence"]["influence_median"], inf["influence_median"].values, rtol=1e-12)


def test_cli_jackknife_conditions(tmp_path):
    dj = _run(str(tmp_path / "cjk"), "sorting", "variant", VAR, "--n-iter", "100", "--jackknife-conditions")
    el = pd.read_csv(f"{dj}/bean_element_result.MixtureNormal.csv")
    inf = pd.read_csv(f"{dj}/bean_sample_influence.MixtureNormal.csv")
    assert set(COLUMNS) <= set(el.columns) and (el["n_sjk"] == len(inf)).all() and len(inf) >= 2
    assert (inf["n_samples"] >= 2).all()  # a condition over all replicates
    assert set(el["mu_sjk_max_shift_sample"].astype(str)) <= set(inf["left_out"].astype(str))


# ---------------------------------------------------------------- a planted bad sample
def test_a_planted_bad_sample_is_the_most_influential():
    """The counts of sample (1, 2) permuted across guides by a fixed permutation - its signal is destroyed - and multiplied
    by 8: an over-amplified sample whose depth the screen's size factors (the whole screen's, from before) do not describe.
    Leaving that sample out moves the targets more than leaving out any other one: it has the largest influence_median.
    The float64 CPU oracle ranks it first too, 0.760 against 0.535 for the runner-up; with the permutation alone (depth
    kept) it does NOT - at 300 steps the samples of the outermost bins lead - which is why the corruption was made stronger
    and not the assertion weaker (scripts/oracle_planted_sample.py, figures in DESIGN.md §12)."""
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_sample_jackknife

    data = make_sorting_variant_screen(640, 3, seed=2)
    perm = torch.randperm(data.n_guides, generator=torch.Generator().manual_seed(12345))
    planted = copy.copy(data)
    for name in ("X", "X_masked", "X_bcmatch", "X_bcmatch_masked"):
        v = getattr(data, name).clone()
        v[1, 2] = v[1, 2][perm] * 8
        setattr(planted, name, v)
    assert torch.equal(planted.X_masked[1, 2].sort().values, 8 * data.X_masked[1, 2].sort().values)
    full, loo, groups, names = run_inference_sample_jackknife(
        partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), planted, num_steps=STEPS, verbose=False)
    inf = sample_jackknife_summary(full, loo, groups, names)["influence"]
    order = sorted(range(len(groups)), key=lambda j: -inf["influence_median"][j])
    print("influence_median, largest first:", [(names[j], inf["influence_median"][j]) for j in order])
    assert groups[order[0]] == [(1, 2)] and names[order[0]] == "r1_c2"
    assert inf["influence_median"][order[0]] > inf["influence_median"][order[1]]
