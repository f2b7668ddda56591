"""Guide jackknife on the GPU.  A member that masks position j of every target is, bit for bit, the single fit of the
screen with those guides masked; on target t's slices it is also, bit for bit, the single fit with ONLY guide (t, j)
masked - the kernels couple no two targets - and a target without a guide at that position keeps the full fit's bits.
Then run_inference_guide_jackknife (batched, fallback, refusals, halts) and the CLI.  -m gpu."""
import functools
import os
import pickle
from functools import partial

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.model.jackknife import guides_at_position, guide_member_masks, guide_positions, leave_out_guides
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

from members_common import (DEV, SEED, STEPS, VAR, _assert_same, _h5ad_reader_present, _kw_of, _mini, _run,  # noqa: F401
                            _same_results, _single, _state)

pytestmark = pytest.mark.gpu
ELEMENT_COLUMNS = ["mu_gjk_se", "mu_gjk_max_shift", "mu_gjk_max_shift_guide", "n_gjk"]
PER_TARGET = ("mu_loc", "mu_scale", "sd_loc", "sd_scale")
PER_GUIDE = ("alpha_pi", "noise_loc", "noise_scale")


CONFIGS = {
    "Normal": ("Normal", dict()),
    "MixtureNormal": ("MixtureNormal", dict()),
    "MixtureNormal+Acc+noise": ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True)),
    "MixtureNormal+Acc": ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=False)),
    "MixtureNormal+prior": ("MixtureNormal", dict(prior="yes")),
}


@functools.lru_cache(maxsize=None)
def _screen(with_accessibility):
    """200 guides x 3 replicates, seven per target: 28 targets of 7 and a last one of 4, i.e. 8 members; 64 = 9 * 7 + 1,
    so a target straddles every tile boundary; masked (replicate, guide) pairs and a masked sample.  Never modified."""
    data = make_sorting_variant_screen(200, 3, seed=9, guides_per_target=7, mask_fraction=0.05,
                                       with_accessibility=with_accessibility)
    assert data.target_lengths.tolist() == [7] * 28 + [4]
    assert not bool(data.repguide_mask.all()) and not bool((data.sample_mask != 0).all())
    off = data.target_offsets
    for edge in (64, 128, 192):
        assert any(int(off[t]) < edge < int(off[t + 1]) for t in range(28)), edge
    return data.to(DEV)


@functools.lru_cache(maxsize=None)
def _members(config):
    """The 8 members' final states of one configuration on the screen above: computed once, shared, never modified."""
    from bean_amd import engine

    family, kw = CONFIGS[config]
    data = _screen(bool(kw.get("scale_by_accessibility")))
    kw = _kw_of(kw, data)
    positions, included = guide_positions(data)
    assert positions == list(range(7)) and int(included.sum()) == 200
    n = 1 + len(positions)
    ens = engine.HipSVI(family, data, num_steps=STEPS, n_members=n, member_masks=guide_member_masks(data, positions), **kw)
    assert ens.ensemble_supported and ens.member_masks
    ens.run_ensemble(STEPS, [SEED] * n)
    torch.cuda.synchronize()
    losses = ens.losses()
    assert losses.shape == (n, STEPS) and np.isfinite(losses).all()
    states = [_state(ens, k) for k in range(n)]
    ens.close()
    return family, kw, data, states


def _slices(state, data, t):
    """Target t's part of a fit's state: its row of the per-target parameters and moments, its guides' rows of the
    per-guide ones (alpha_pi and, where fitted, the noise)."""
    off = data.target_offsets
    rows = {"target": slice(t, t + 1), "guide": slice(int(off[t]), int(off[t + 1]))}
    out = {}
    for k, v in state.items():
        if k == "loss":  # the loss sums over all targets
            continue
        name = k.split(".", 1)[1]
        assert name in PER_TARGET or name in PER_GUIDE, f"{k}: a parameter that belongs to no target"
        assert v.shape[0] == (data.n_targets if name in PER_TARGET else data.n_guides), k
        out[k] = v[rows["target" if name in PER_TARGET else "guide"]]
    return out


# ---------------------------------------------------------------- member == the single fit with the same masks
@pytest.mark.parametrize("config", list(CONFIGS))
def test_member_is_the_single_fit_with_its_masks(config):
    family, kw, data, states = _members(config)
    for k, st in enumerate(states):
        screen = data if k == 0 else leave_out_guides(data, guides_at_position(data, k - 1))
        what = "the plain fit" if k == 0 else f"position {k - 1} left out"
        _assert_same(st, _single(family, screen, kw), f"{config} member {k} ({what})")
    # same seed, other data: the members differ from the full fit and from each other
    assert not torch.equal(states[0]["p.mu_loc"], states[1]["p.mu_loc"])
    assert not torch.equal(states[1]["p.mu_loc"], states[2]["p.mu_loc"])


@pytest.mark.parametrize("extra,family", [([], "MixtureNormal"), (["--uniform-edit"], "Normal")])
def test_member_is_the_single_fit_mini_screen(tmp_path, extra, family):
    """The 30-guide fixture every reference test runs: 6 targets, i.e. the wide-target (generic) k_param."""
    from bean_amd import engine

    data = _mini(tmp_path, *extra).to(DEV)
    assert (data.n_guides, data.n_targets) == (30, 6)
    positions, included = guide_positions(data)
    n = 1 + len(positions)
    assert positions == list(range(5)) and included.shape == (6, 5)
    ens = engine.HipSVI(family, data, num_steps=STEPS, n_members=n, member_masks=guide_member_masks(data, positions))
    ens.run_ensemble(STEPS, [SEED] * n)
    torch.cuda.synchronize()
    states = [_state(ens, k) for k in range(n)]
    ens.close()
    for k, st in enumerate(states):
        screen = data if k == 0 else leave_out_guides(data, guides_at_position(data, k - 1))
        _assert_same(st, _single(family, screen, {}), f"{family} mini screen, member {k}")
    # and one member serves every target here too: target 2 without its guide 3 alone
    one = _single(family, leave_out_guides(data, int(data.target_offsets[2]) + 3), {})
    _assert_same(_slices(states[4], data, 2), _slices(one, data, 2), f"{family} mini screen, target 2 position 3")


# ---------------------------------------------------------------- one member serves every target
# the first target; target 9 = guides 63 .. 69, on both sides of the first tile boundary (its guide on the far side, its
# last guide, and - position 0 - the one on the near side); the short last target (guides 196 .. 199)
PAIRS = [(0, 2), (9, 0), (9, 1), (9, 6), (28, 3)]


@pytest.mark.parametrize("config", ["Normal", "MixtureNormal", "MixtureNormal+Acc+noise"])
def test_one_member_serves_every_target(config):
    family, kw, data, states = _members(config)
    off = data.target_offsets
    assert int(off[9]) == 63 and int(off[10]) == 70 and int(off[28]) == 196
    moved = 0
    for t, j in PAIRS:
        g = int(off[t]) + j
        assert bool(data.repguide_mask[:, g].any()), (t, j)
        one = _single(family, leave_out_guides(data, g), kw)  # only guide (t, j) masked
        got, want = _slices(states[1 + j], data, t), _slices(one, data, t)
        if family == "MixtureNormal":
            assert {"p.alpha_pi", "m.alpha_pi", "v.alpha_pi"} <= set(want)
        if kw.get("fit_noise"):
            assert {"p.noise_loc", "v.noise_scale"} <= set(want)
        _assert_same(got, want, f"{config}: target {t} in the member for position {j} against guide {g} masked alone")
        # the single fit leaves another target as the full fit has it
        u = 5 if t != 5 else 6
        _assert_same(_slices(one, data, u), _slices(states[0], data, u), f"{config}: target {u} with guide {g} masked")
        full = _slices(states[0], data, t)
        differs = sorted(k for k in want if not torch.equal(want[k], full[k]))
        print(f"{config}: guide {g} = (target {t}, position {j}) masked alone moves {len(differs)} of {len(want)} slices of its target")
        moved += bool(differs)
    # not vacuous: a guide matters to its target.  (Not asserted pair by pair: ClippedAdam clips every gradient entry to
    # +-10, and where an entry stays beyond that in both fits at every step the two take the same steps.)
    assert moved >= 1


@pytest.mark.parametrize("config", list(CONFIGS))
def test_untouched_targets_keep_the_full_fits_bits(config):
    """The last target has guides at positions 0 .. 3 only: in the members for positions 4, 5 and 6 nothing of it is
    masked, and its slices are member 0's."""
    _, _, data, states = _members(config)
    want = _slices(states[0], data, 28)
    for j in (4, 5, 6):
        _assert_same(_slices(states[1 + j], data, 28), want, f"{config}: the last target in the member for position {j}")
        assert not torch.equal(states[1 + j]["p.mu_loc"][:28], states[0]["p.mu_loc"][:28])  # (the other targets do move)


# ---------------------------------------------------------------- run_inference_guide_jackknife


def test_run_inference_guide_jackknife_batched_fallback_and_tiling(tmp_path, monkeypatch):
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model import survival_model as sm
    from bean_amd.model.run import run_inference, run_inference_guide_jackknife

    monkeypatch.chdir(tmp_path)

    def same(res, model, guide, data, n, lengths):
        full, loo, positions, included = res
        assert positions == list(range(max(lengths))) and len(loo) == len(positions)
        assert included.shape == (data.n_targets, len(positions))
        assert int(included.sum()) == int(data.repguide_mask.any(0).sum()) >= data.n_guides - 2
        _same_results(full, run_inference(model, guide, data, num_steps=n, seed=7, verbose=False))
        for fit, j in zip(loo, positions):
            masked = leave_out_guides(data, guides_at_position(data, j))
            _same_results(fit, run_inference(model, guide, masked, num_steps=n, seed=7, verbose=False))

    used = []
    real = engine.HipSVI.run_ensemble
    monkeypatch.setattr(engine.HipSVI, "run_ensemble", lambda self, *a, **k: (used.append(a[0]), real(self, *a, **k))[1])
    var = make_sorting_variant_screen(200, 3, seed=9, guides_per_target=7)
    mod, gd = partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)
    same(run_inference_guide_jackknife(mod, gd, var, seed=7, num_steps=250, verbose=False), mod, gd, var, 250, [7, 4])
    assert used == [100, 100, 50]  # batched, in report windows
    used.clear()
    # the cap: only the short last target takes part, four positions
    full, loo, positions, included = run_inference_guide_jackknife(mod, gd, var, seed=7, num_steps=20, verbose=False,
                                                                   max_positions=4)
    assert positions == [0, 1, 2, 3] and len(loo) == 4 and int(included.sum()) == 4 and bool(included[-1].all())
    used.clear()
    surv = make_survival_variant_screen(300, 2, seed=2)
    mod, gd = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)
    same(run_inference_guide_jackknife(mod, gd, surv, seed=7, num_steps=120, verbose=False), mod, gd, surv, 120, [5])
    assert used == []  # the fallback: one fit after the other
    til = make_sorting_tiling_screen(200, 2, seed=2)
    with pytest.raises(ValueError, match="tiling"):
        run_inference_guide_jackknife(partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide), til,
                                      num_steps=10, verbose=False)
    assert used == [] and os.listdir(tmp_path) == []


def test_halt_on_nan_in_a0_writes_the_dump(tmp_path, monkeypatch):
    """A NaN in the data reaches the full screen first (a member only ever masks more), so the member named is the
    full screen; the dump says that no position was left out."""
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_guide_jackknife

    data = make_sorting_variant_screen(640, 3, seed=4)
    data.a0 = data.a0.clone()
    data.a0[17] = float("nan")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*the full screen \(seed 101\).*non-finite loss at iteration 0"):
        run_inference_guide_jackknife(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, num_steps=300,
                                      verbose=False)
    assert sorted(os.listdir(tmp_path)) == ["tmp_result.full.pkl"]
    with open(tmp_path / "tmp_result.full.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert dump["left_out_position"] is None and dump["seed"] == 101 and "mu_loc" in dump["param"]
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


def test_halt_names_the_position(tmp_path, monkeypatch):
    """A member other than the full fit goes NaN (its parameters are poisoned behind the window's snapshot): message,
    file name and the dump carry the POSITION that member leaves out - member 2 leaves out position 1 (the screen has
    5 guides per target and a last target of 3)."""
    from bean_amd import engine
    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference_guide_jackknife

    data = make_sorting_variant_screen(638, 3, seed=4)
    real = engine.HipSVI.run_ensemble

    def poisoned(self, *a, **k):
        if self.steps_done == 0:
            self.unconstrained["mu_loc"][2, 4] = float("nan")
        return real(self, *a, **k)

    monkeypatch.setattr(engine.HipSVI, "run_ensemble", poisoned)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match=r"(?s)Fitting halted.*guides at position 1 of their targets left out "
                                         r"\(seed 101\).*non-finite loss at iteration 0"):
        run_inference_guide_jackknife(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), data, num_steps=300,
                                      verbose=False)
    assert sorted(os.listdir(tmp_path)) == ["tmp_result.without_guide_position1.pkl"]
    with open(tmp_path / "tmp_result.without_guide_position1.pkl", "rb") as fh:
        dump = pickle.load(fh)
    assert dump["left_out_position"] == 1 and dump["seed"] == 101 and "mu_loc" in dump["param"]
    for k, v in dump["param"].items():
        assert torch.isfinite(v).all(), k


# ---------------------------------------------------------------- CLI


def test_cli_jackknife_guides(tmp_path):
    base = ["sorting", "variant", VAR, "--n-iter", str(STEPS)]
    dj = _run(str(tmp_path / "gjk"), *base, "--jackknife-guides", "--save-raw")
    d0 = _run(str(tmp_path / "plain"), *base)
    name_el, name_sg = "bean_element_result.MixtureNormal.csv", "bean_sgRNA_result.MixtureNormal.csv"
    read = lambda path: pd.read_csv(path, float_precision="round_trip")  # noqa: E731
    el, plain = read(f"{dj}/{name_el}"), read(f"{d0}/{name_el}")
    assert not set(ELEMENT_COLUMNS) & set(plain.columns)
    assert [c for c in el.columns if c not in plain.columns] == ELEMENT_COLUMNS
    pd.testing.assert_frame_equal(el.drop(columns=ELEMENT_COLUMNS), plain, check_exact=True)
    assert len(el) == 6 and (el["n_gjk"] == 5).all()
    assert np.isfinite(el[["mu_gjk_se", "mu_gjk_max_shift"]].values).all()
    assert (el["mu_gjk_se"] >= 0).all() and (el["mu_gjk_se"] > 0).any()
    assert (el["mu_gjk_max_shift"] >= 0).all() and (el["mu_gjk_max_shift"] > 0).any()
    sg, plain_sg = read(f"{dj}/{name_sg}"), read(f"{d0}/{name_sg}")
    assert list(sg.columns) == list(plain_sg.columns) + ["mu_shift_left_out"]
    pd.testing.assert_frame_equal(sg.drop(columns=["mu_shift_left_out"]), plain_sg, check_exact=True)
    assert len(sg) == 30 and np.isfinite(sg["mu_shift_left_out"]).all()
    with open(f"{dj}/MixtureNormal.result.pkl", "rb") as fh:
        raw = pickle.load(fh)
    # the guide named for a target is one of its own, and the one with the largest |shift| among them
    guides = raw["data"].screen.guides
    name_col = sg.columns[0]
    for _, row in el.iterrows():
        own = sg[sg[name_col].isin(guides.index[guides["target"].astype(str) == str(row["target"])])]
        assert len(own) == 5 and row["mu_gjk_max_shift_guide"] in set(own[name_col])
        worst = own.loc[own["mu_shift_left_out"].abs().idxmax()]
        assert worst[name_col] == row["mu_gjk_max_shift_guide"]
        assert abs(worst["mu_shift_left_out"]) == row["mu_gjk_max_shift"]
    gj = raw["guide_jackknife"]
    assert set(gj) == {"included", "positions"} and gj["included"].shape == (6, 5) and bool(gj["included"].all())
    assert [e["position"] for e in gj["positions"]] == [0, 1, 2, 3, 4]
    assert all(set(e) == {"position", "params", "loss"} and len(e["loss"]) == STEPS for e in gj["positions"])
    # the pickle's main entries are the plain fit's; the members differ from it
    np.testing.assert_allclose(np.sort(plain["mu"].values), np.sort(raw["params"]["mu_loc"].reshape(-1).numpy()), rtol=1e-6)
    assert not torch.equal(gj["positions"][0]["params"]["mu_loc"], raw["params"]["mu_loc"])
