"""Sample jackknife, the parts that need no GPU: leave_out_samples, the groups of both modes, the members' masks and
counts, sample_jackknife_summary on hand-computed numbers, the two flags and their refusals, the three added columns of
the element table with the influence table, and the C entry point (declared, exported, listed, null handle rejected)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model import readwrite
from bean_amd.model.jackknife import (leave_out, leave_out_samples, sample_groups, sample_jackknife_summary,
                                      sample_member_counts, sample_member_masks)
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ["mu_sjk_max_shift", "mu_sjk_max_shift_sample", "n_sjk"]
CHANGED = ("sample_mask", "X_masked", "X_bcmatch_masked")


# ---------------------------------------------------------------- leave_out_samples
@pytest.mark.parametrize("make", [lambda: make_sorting_variant_screen(200, 3, seed=5, mask_fraction=0.05),
                                  lambda: make_sorting_tiling_screen(60, 2, seed=2),
                                  lambda: make_survival_variant_screen(80, 3, seed=2)],
                         ids=["sorting variant", "sorting tiling", "survival variant"])
def test_leave_out_samples_zeroes_the_named_rows_and_nothing_else(make):
    data = make()
    R, B = data.n_reps, data.n_condits
    before = {k: v.clone() for k, v in data.tensor_items()}
    pairs = [(1, 2), (0, B - 1)]
    out = leave_out_samples(data, pairs)
    for k, v in data.tensor_items():  # the original is not modified
        assert torch.equal(v, before[k]), k
    assert set(vars(out)) == set(vars(data))
    for k, v in vars(data).items():
        if k in CHANGED:
            continue
        w = getattr(out, k)
        assert w is v or (isinstance(v, torch.Tensor) and torch.equal(v, w)), k
    assert getattr(data, "X_bcmatch_masked", None) is not None
    keep = torch.ones(R, B, dtype=torch.bool)
    for r, b in pairs:
        keep[r, b] = False
    for name in CHANGED:
        a, b_ = getattr(data, name), getattr(out, name)
        assert a.dtype == b_.dtype and a.shape == b_.shape and a.data_ptr() != b_.data_ptr(), name
        assert torch.equal(a[keep], b_[keep]), name  # every other sample as it was
        assert not bool(b_[~keep].any()), name  # the named ones zero
    assert bool(data.X_masked[~keep].any()) and bool(data.sample_mask[~keep].all())
    # the unmasked counts are the screen's: X is not X_masked
    assert torch.equal(out.X, data.X)
    for bad in ([(R, 0)], [(0, B)], [(-1, 0)], [(0, -1)]):
        with pytest.raises(ValueError, match="sample"):
            leave_out_samples(data, bad)
    with pytest.raises(ValueError, match="pair"):
        leave_out_samples(data, [3])
    assert torch.equal(leave_out_samples(data, []).sample_mask, data.sample_mask)


def test_leave_out_samples_without_barcode_matched_counts():
    data = make_sorting_variant_screen(50, 2, seed=5)
    data.X_bcmatch_masked = None
    out = leave_out_samples(data, [(1, 0)])
    assert out.X_bcmatch_masked is None and not bool(out.X_masked[1, 0].any()) and int(out.sample_mask[1, 0]) == 0


# ---------------------------------------------------------------- sample_groups
def test_sample_groups_both_modes():
    data = make_sorting_variant_screen(120, 3, seed=5)
    R, B = data.n_reps, data.n_condits
    groups, names = sample_groups(data, "sample")
    assert groups == [[(r, b)] for r in range(R) for b in range(B)]
    assert names == [f"r{r}_c{b}" for r in range(R) for b in range(B)]
    groups, names = sample_groups(data, "condition")
    assert groups == [[(r, b) for r in range(R)] for b in range(B)] and names == [f"c{b}" for b in range(B)]
    with pytest.raises(ValueError, match="by must be"):
        sample_groups(data, "replicate")


def test_masked_samples_and_masked_replicates_are_no_candidates():
    data = make_sorting_variant_screen(120, 3, seed=5, mask_fraction=0.05)  # sample (2, 0) is masked in the screen
    R, B = data.n_reps, data.n_condits
    assert int(data.sample_mask[R - 1, 0]) == 0
    groups, names = sample_groups(data, "sample")
    assert [(R - 1, 0)] not in groups and len(groups) == R * B - 1 and "r2_c0" not in names
    groups, _ = sample_groups(data, "condition")
    assert groups[0] == [(r, 0) for r in range(R - 1)] and len(groups) == B
    # a replicate whose repguide_mask row is zero throughout: none of its samples is a candidate
    gone = leave_out(data, 1)
    gone.sample_mask = data.sample_mask  # (only the repguide row masks it)
    groups, _ = sample_groups(gone, "sample")
    assert all(r != 1 for g in groups for r, _ in g) and len(groups) == (R - 1) * B - 1
    # fewer than two groups
    one = leave_out_samples(data, [(r, b) for r in range(R) for b in range(B) if (r, b) != (0, 1)])
    with pytest.raises(ValueError, match="found 1"):
        sample_groups(one, "sample")
    with pytest.raises(ValueError, match="found 1"):
        sample_groups(one, "condition")


# ---------------------------------------------------------------- members
def test_member_masks_and_counts_are_the_left_out_screens():
    data = make_sorting_variant_screen(90, 3, seed=5, mask_fraction=0.05)
    groups, _ = sample_groups(data, "condition")
    groups = groups + [[(1, 2)]]
    K = 1 + len(groups)
    rg, sm = sample_member_masks(data, groups)
    x, xbc = sample_member_counts(data, groups)
    assert rg.shape == (K, data.n_reps, data.n_guides) and rg.dtype == torch.bool
    assert sm.shape == (K, data.n_reps, data.n_condits) and sm.dtype == data.sample_mask.dtype
    assert x.shape == xbc.shape == (K, data.n_reps, data.n_condits, data.n_guides)
    assert x.dtype == xbc.dtype == torch.float32
    for k, screen in enumerate([data] + [leave_out_samples(data, g) for g in groups]):
        assert torch.equal(rg[k], data.repguide_mask != 0) and torch.equal(sm[k], screen.sample_mask), k
        assert torch.equal(x[k], screen.X_masked) and torch.equal(xbc[k], screen.X_bcmatch_masked), k
    assert not torch.equal(x[1], x[0]) and not torch.equal(sm[1], sm[0])
    data.X_bcmatch_masked = None
    assert sample_member_counts(data, groups)[1] is None


# ---------------------------------------------------------------- summary
def _fit(mu, scale=None):
    out = {"mu_loc": torch.tensor(mu, dtype=torch.float32).reshape(-1, 1)}
    if scale is not None:
        out["mu_scale"] = torch.tensor(scale, dtype=torch.float32).reshape(-1, 1)
    return out


def test_summary_matches_hand_computed_numbers():
    """Three targets, four groups; c = (1, 0, -2), s = (0.5, 1, 0.25).

    group a: m = (1.5, 0, -2)      |m - c| = (0.5, 0, 0)     / s = (1, 0, 0)    median 0, max 1, moved 0 (0.5 > 0.5 is false)
    group b: m = (1, 2, -2.5)      |m - c| = (0, 2, 0.5)     / s = (0, 2, 2)    median 2, max 2, moved 2
    group c: m = (0.5, -2, -1.75)  |m - c| = (0.5, 2, 0.25)  / s = (1, 2, 1)    median 1, max 2, moved 1 (target 1 only)
    group d: m = (1.25, 1, -1)     |m - c| = (0.25, 1, 1)    / s = (0.5, 1, 4)  median 1, max 4, moved 1 (target 2 only)

    Per target: 0.5 (a and c tie: a), 2 (b and c tie: b), 1 (d)."""
    full = _fit([1.0, 0.0, -2.0], [0.5, 1.0, 0.25])
    loo = [_fit([1.5, 0.0, -2.0]), _fit([1.0, 2.0, -2.5]), (_fit([0.5, -2.0, -1.75]), {"loss": [], "params": {}}),
           _fit([1.25, 1.0, -1.0])]
    groups = [[(0, 0)], [(0, 1)], [(1, 0), (1, 1)], [(2, 2)]]
    out = sample_jackknife_summary(full, loo, groups, ["a", "b", "c", "d"])
    assert set(out) == set(COLUMNS) | {"influence"}
    assert out["mu_sjk_max_shift"].dtype == torch.float64
    assert out["mu_sjk_max_shift"].reshape(-1).tolist() == [0.5, 2.0, 1.0]
    assert out["mu_sjk_max_shift_sample"] == ["a", "b", "d"] and out["n_sjk"] == 4
    inf = out["influence"]
    assert inf["left_out"] == ["a", "b", "c", "d"] and inf["n_samples"] == [1, 1, 2, 1]
    assert inf["influence_median"] == [0.0, 2.0, 1.0, 1.0]
    assert inf["influence_max"] == [1.0, 2.0, 2.0, 4.0]
    assert inf["n_targets_moved"] == [0, 2, 1, 1]
    assert not any("se" in k.split("_") for k in out)  # no standard error: samples are not exchangeable
    with pytest.raises(ValueError, match="at least two"):
        sample_jackknife_summary(full, loo[:1], groups[:1], ["a"])
    with pytest.raises(ValueError, match="at least two"):
        sample_jackknife_summary(full, loo, groups[:3], ["a", "b", "c", "d"])


# ---------------------------------------------------------------- flags
RUN = ["run", "sorting", "variant", "screen.h5ad"]


@pytest.mark.parametrize("flag,attr", [("--jackknife-samples", "jackknife_samples"),
                                       ("--jackknife-conditions", "jackknife_conditions")])
def test_flags_are_accepted_and_refused_in_combination(flag, attr, capsys):
    from bean_amd.cli.execute import get_parser
    from bean_amd.cli.execute import main as bean_main
    from bean_amd.cli.run import check_sample_jackknife_switches
    from bean_amd.model.parser import parse_args as reference_table

    parser = get_parser()
    assert getattr(parser.parse_args(RUN), attr) is False
    assert getattr(parser.parse_args(RUN + [flag]), attr) is True
    assert parser.parse_args(RUN + [flag, "--n-seeds", "1"]).n_seeds == 1
    other = "--jackknife-conditions" if flag == "--jackknife-samples" else "--jackknife-samples"
    for extra, word in (([other], other), (["--jackknife-replicates"], "--jackknife-replicates"),
                        (["--jackknife-guides"], "--jackknife-guides"), (["--n-seeds", "2"], "--n-seeds"),
                        (["--load-existing"], "--load-existing")):
        with pytest.raises(SystemExit) as exc:
            bean_main(RUN + [flag] + extra)  # refused before anything is read or fitted
        assert exc.value.code == 2, extra
        msg = capsys.readouterr().err
        assert word in msg and "--jackknife-" in msg, (extra, msg)
        # ... and by the run itself, for callers that bypass the parser
        args = parser.parse_args(RUN + [flag] + extra)
        with pytest.raises(ValueError, match=re.escape(word)):
            check_sample_jackknife_switches(args)
    assert check_sample_jackknife_switches(parser.parse_args(RUN)) is None
    assert check_sample_jackknife_switches(parser.parse_args(RUN + [flag])) == ("sample" if "samples" in flag else "condition")
    with pytest.raises(SystemExit):
        reference_table().parse_args(RUN[1:] + [flag])  # not in the reference's flag table


def test_group_names_come_from_the_sample_table():
    from bean_amd.cli.run import _sample_group_names

    R, B = 2, 3
    samples = pd.DataFrame({"condition": ["bot", "bulk", "top"] * R},
                           index=[f"rep{r}_{c}" for r in range(R) for c in ("bot", "bulk", "top")])
    ndata = SimpleNamespace(n_reps=R, n_condits=B, screen=SimpleNamespace(samples=samples))
    groups = [[(0, 2)], [(1, 0)]]
    assert _sample_group_names(ndata, groups, ["r0_c2", "r1_c0"], "sample", "condition") == ["rep0_top", "rep1_bot"]
    groups = [[(0, 0), (1, 0)], [(0, 2), (1, 2)]]
    assert _sample_group_names(ndata, groups, ["c0", "c2"], "condition", "condition") == ["bot", "top"]
    assert _sample_group_names(ndata, groups, ["c0", "c2"], "condition", "no_such_column") == ["c0", "c2"]
    bare = SimpleNamespace(n_reps=R, n_condits=B)  # a screen without a sample table
    assert _sample_group_names(bare, groups, ["c0", "c2"], "condition", "condition") == ["c0", "c2"]


# ---------------------------------------------------------------- table
def _write(tmp_path, name, **kw):
    n = 40
    g = torch.Generator().manual_seed(3)
    target_info = pd.DataFrame({"n_guides": 3}, index=pd.Index([f"t{i}" for i in range(n)], name="target"))
    guide_info = pd.DataFrame({"edit_rate": 0.5}, index=pd.Index([f"g{i}" for i in range(3 * n)], name="name"))
    P = {"mu_loc": torch.randn(n, 1, generator=g), "mu_scale": 0.1 + torch.rand(n, 1, generator=g),
         "sd_loc": 0.1 * torch.randn(n, 1, generator=g), "sd_scale": 0.1 + torch.rand(n, 1, generator=g)}
    prefix = str(tmp_path / name) + "."
    readwrite.write_result_table(target_info, guide_info, P, model_label="Normal", prefix=prefix,
                                 adjust_confidence_by_negative_control=False, **kw)
    return prefix, n


def test_element_table_gains_exactly_the_three_columns_and_the_influence_table(tmp_path):
    ref_prefix, n = _write(tmp_path, "plain")
    again, _ = _write(tmp_path, "again", sample_jackknife=None)
    influence = {"left_out": ["s0", "s1", "s2"], "n_samples": [1, 1, 1], "influence_median": [0.25, 0.5, 3.0],
                 "influence_max": [1.0, 2.0, 8.0], "n_targets_moved": [0, 1, 30]}
    sjk = {"mu_sjk_max_shift": torch.linspace(1, 2, n, dtype=torch.float64).reshape(n, 1),
           "mu_sjk_max_shift_sample": [f"s{i % 3}" for i in range(n)], "n_sjk": 3, "influence": influence}
    prefix, _ = _write(tmp_path, "sjk", sample_jackknife=sjk)
    el, sg, inf = "bean_element_result.Normal.csv", "bean_sgRNA_result.Normal.csv", "bean_sample_influence.Normal.csv"
    # without the argument: the two tables as they were, and no third one
    assert open(again + el, "rb").read() == open(ref_prefix + el, "rb").read()
    assert open(again + sg, "rb").read() == open(ref_prefix + sg, "rb").read()
    assert not os.path.exists(ref_prefix + inf) and not os.path.exists(again + inf)
    ref = pd.read_csv(ref_prefix + el, float_precision="round_trip")
    got = pd.read_csv(prefix + el, float_precision="round_trip")
    assert not set(COLUMNS) & set(ref.columns)
    assert [c for c in got.columns if c not in ref.columns] == COLUMNS
    assert [c for c in got.columns if c not in COLUMNS] == list(ref.columns)
    pd.testing.assert_frame_equal(got.drop(columns=COLUMNS), ref, check_exact=True)
    by_target = got.set_index("target")
    for i in (0, 7, n - 1):
        row = by_target.loc[f"t{i}"]
        assert row["mu_sjk_max_shift"] == float(sjk["mu_sjk_max_shift"][i])
        assert row["mu_sjk_max_shift_sample"] == f"s{i % 3}" and row["n_sjk"] == 3
    assert open(prefix + sg, "rb").read() == open(ref_prefix + sg, "rb").read()
    table = pd.read_csv(prefix + inf, float_precision="round_trip")
    assert list(table.columns) == list(influence) and len(table) == 3
    for k, v in influence.items():
        assert table[k].tolist() == v, k
    with pytest.raises(ValueError, match="entries for"):
        _write(tmp_path, "bad", sample_jackknife=dict(sjk, mu_sjk_max_shift=sjk["mu_sjk_max_shift"][:-1]))


# ---------------------------------------------------------------- C entry point
def test_entry_point_declared_exported_listed_and_null_handle_rejected():
    _lib.build_library()
    lib = _lib.load()
    name = "bean_hip_bind_member_counts"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in bean_hip.h"
    assert hasattr(lib, name) and name in {s[0] for s in _lib.SYMBOLS} and name in _lib.ENSEMBLE_SYMBOLS
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.bean_hip_bind_member_counts(None, None, 0, None, 0) < 0
    msg = lib.bean_hip_last_error().decode()
    assert "bind_member_counts" in msg and "null handle" in msg


def test_engine_refuses_bad_member_counts_before_the_library(monkeypatch):
    """Shape, dtype and the presence of X_bcmatch are checked in front of everything that needs a GPU."""
    from bean_amd import engine

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # whatever the machine: the engine stops right behind the checks
    data = make_sorting_variant_screen(64, 2, seed=5)
    groups, _ = sample_groups(data, "sample")
    K = 1 + len(groups)
    x, xbc = sample_member_counts(data, groups)
    new = lambda **kw: engine.HipSVI("MixtureNormal", data, num_steps=10, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="n_members > 1"):
        new(member_counts=(x[:1], xbc[:1]))
    with pytest.raises(ValueError, match="pair"):
        new(n_members=K, member_counts=x)
    for bad in ((x[:-1], xbc), (x, xbc[:, :, :-1]), (x[..., :-1], xbc[..., :-1]), (x.reshape(K, -1), xbc)):
        with pytest.raises(ValueError, match="member_counts: X"):
            new(n_members=K, member_counts=bad)
    with pytest.raises(ValueError, match="float32"):
        new(n_members=K, member_counts=(x.double(), xbc))
    with pytest.raises(ValueError, match="float32"):
        new(n_members=K, member_counts=(x, xbc.numpy()))
    with pytest.raises(ValueError, match="X_bcmatch goes with"):
        new(n_members=K, member_counts=(x, None))
    with pytest.raises(ValueError, match="X_bcmatch goes with"):
        new(n_members=K, member_counts=(x, xbc), use_bcmatch=False)
    with pytest.raises(RuntimeError, match="ROCm GPU"):  # well-formed: past the checks
        new(n_members=K, member_counts=(x, xbc))
