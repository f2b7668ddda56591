"""Power study, the parts that need no GPU: the C entry point, the member plan, the summary, the --power-* flags with
their refusals, and what run_inference_power refuses before it builds an engine."""
import argparse
import contextlib
import ctypes
import io
import os
import re
import types
from functools import partial

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model import jackknife as jk
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bean_hip_simulate_power"
RUN = ["run", "sorting", "variant", "screen.h5ad"]
EFFECTS = ["--power-effects", "0.5,2"]


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text), f"{NAME} not declared in bean_hip.h"
    # declared after the other simulators: every other kernel keeps its place in the code object
    assert text.index("bean_hip_simulate_design(") < text.index(NAME + "(")
    (entry,) = [s for s in _lib.SYMBOLS if s[0] == NAME]
    # ctx, seed, first_draw, n_draws, effects, n_effects, plant, x_out, x_bytes, xbc_out, xbc_bytes, stream
    declared = re.search(NAME + r"\s*\(([^)]*)\)", text).group(1)
    assert entry[1] is ctypes.c_int32 and len(entry[2]) == len(declared.split(",")) == 12
    assert [s[0] for s in _lib.SYMBOLS].index("bean_hip_simulate_design") + 1 == [s[0] for s in _lib.SYMBOLS].index(NAME)
    assert NAME in _lib.ENSEMBLE_SYMBOLS
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), NAME), f"{NAME} not exported by {_lib.tree_path(build)}"


def test_null_handle_is_rejected_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    one = (ctypes.c_double * 1)(0.5)
    assert lib.bean_hip_simulate_power(None, 1, 0, 4, one, 1, None, None, 0, None, 0, None) < 0
    msg = lib.bean_hip_last_error().decode()
    assert "simulate_power" in msg and "null handle" in msg, msg


# ---------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def screen():
    return make_sorting_variant_screen(40, 2, seed=1, mask_fraction=0.05)


def _planes(data, D, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 50, (D, K) + tuple(data.X_masked.shape), generator=g).to(data.X_masked.dtype)


@pytest.mark.parametrize("with_bc", [True, False])
def test_power_plan(screen, with_bc):
    data = screen
    effects, K = [0.0, 0.25, -1.5], 3
    D = len(effects)
    x, xbc = _planes(data, D, K, 1), (_planes(data, D, K, 2) if with_bc else None)
    before = {k: v.clone() for k, v in vars(data).items() if torch.is_tensor(v)}
    ids = {k: id(v) for k, v in vars(data).items()}
    plan = jk.power_plan(data, 7, effects, x, xbc)
    assert isinstance(plan, jk.MemberPlan)
    assert list(plan.seeds) == [7] * (1 + D * K)  # common random numbers: the members differ through their data
    text = ["0", "0.25", "-1.5"]
    assert list(plan.labels) == ["the full screen"] + [f"effect {t} screen {j}" for t in text for j in range(K)]
    assert list(plan.tags) == ["full"] + [f"effect{t}_{j}" for t in text for j in range(K)]
    assert list(plan.dump_extra) == [{"effect": None, "screen": None, "seed": 7}] + [
        {"effect": e, "screen": j, "seed": 7} for e in effects for j in range(K)]
    assert plan.differ_in == ("masks", "counts") and plan.per_run == 63 and plan.label_halts
    assert plan.screen(0) is data
    for i in range(D):
        for j in range(K):
            member = plan.screen(1 + i * K + j)
            assert member is not data and type(member) is type(data)
            assert torch.equal(member.X_masked, x[i, j])
            if with_bc:
                assert torch.equal(member.X_bcmatch_masked, xbc[i, j])
            changed = {"X_masked"} | ({"X_bcmatch_masked"} if with_bc else set())
            for name, value in vars(member).items():
                if name not in changed:  # masks, size factors, a0, pi_a0: shared, conditioned on
                    assert value is vars(data)[name], name
    assert {k: id(v) for k, v in vars(data).items()} == ids
    for k, v in before.items():
        assert torch.equal(v, vars(data)[k]) or (v != v).any(), k
    got_x, _ = jk.stack_counts([plan.screen(1 + m) for m in range(D * K)])
    assert torch.equal(got_x, x.reshape((D * K,) + tuple(x.shape[2:])).float())
    with pytest.raises(ValueError, match="x_bcmatch"):
        jk.power_plan(data, 7, effects, x, x[:, :2])
    with pytest.raises(ValueError, match=r"\(D, K, R, B, G\)"):
        jk.power_plan(data, 7, effects, x[:2])
    with pytest.raises(ValueError, match=r"\(D, K, R, B, G\)"):
        jk.power_plan(data, 7, effects, x[0])


# ---------------------------------------------------------------- the summary
def _crossing(anchors, p, level):
    """The minimal detectable effect of one target: anchors ascending from 0, p its power at each."""
    if len(anchors) < 2:
        return np.inf
    if p[0] >= level:
        return anchors[1]
    for k in range(1, len(anchors)):
        if p[k] >= level:
            w = (level - p[k - 1]) / (p[k] - p[k - 1])
            return anchors[k - 1] * (1.0 - w) + anchors[k] * w
    return np.inf


def _numpy_summary(m, s, effects, planted, z, level):
    """power_summary restated: m, s (D, K, T), planted (T,) bool."""
    D, K, T = m.shape
    e = np.asarray(effects)
    det = np.abs(m) / s >= z
    for i in range(D):
        if e[i] != 0:
            det[i] &= np.sign(m[i]) == np.sign(e[i])
    power = det.mean(1)
    power[:, ~planted] = np.nan
    some = planted.any()
    out = {"power": power,
           "power_mean": np.array([det[i][:, planted].mean() if some else np.nan for i in range(D)]),
           "power_median": np.array([np.median(power[i][planted]) if some else np.nan for i in range(D)]),
           "mu_power_mean": m.mean(1), "mu_power_se": m.std(1, ddof=1),
           "shrinkage": np.array([np.median(m[i].mean(0)[planted] / e[i]) if some and e[i] != 0 else np.nan
                                  for i in range(D)])}
    null = effects.index(0.0)
    for key, sign in (("mde", 1.0), ("mde_neg", -1.0)):
        rows = sorted((sign * f, i) for i, f in enumerate(effects) if sign * f > 0)
        if key == "mde_neg" and not rows:
            continue
        anchors = [0.0] + [a for a, _ in rows]
        idx = [null] + [i for _, i in rows]
        out[key] = np.array([_crossing(anchors, power[idx, t], level) if planted[t] else np.nan for t in range(T)])
    return out


def _stores(m, s, T=None):
    T = m.shape[2] if T is None else T
    full = {"mu_loc": torch.zeros(T, 1, dtype=torch.float64), "mu_scale": torch.ones(T, 1, dtype=torch.float64)}
    fits = [[({"mu_loc": torch.as_tensor(m[i, j]).reshape(-1, 1), "mu_scale": torch.as_tensor(s[i, j]).reshape(-1, 1)},
              {"loss": []}) for j in range(m.shape[1])] for i in range(m.shape[0])]
    return full, fits


NUMERIC = ("power", "power_mean", "power_median", "mu_power_mean", "mu_power_se", "shrinkage", "mde")


def test_power_summary_is_numpys():
    rng = np.random.default_rng(5)
    for T, K, effects, z, level in ((7, 2, [0.0, 0.5], 1.0, 0.5), (12, 9, [0.25, 0.0, -1.0, 1.0, -0.25, 2.0], 1.96, 0.8),
                                    (1, 5, [0.0], 0.5, 0.8), (9, 6, [-0.5, 0.0, -2.0], 0.7, 0.6)):
        D = len(effects)
        e = np.asarray(effects)
        m = rng.normal(size=(D, K, T)) + 1.5 * e[:, None, None]
        s = 0.3 + rng.random((D, K, T))
        planted = rng.random(T) < 0.7 if T > 1 else np.array([True])
        planted[0] = True
        for mask in (None, planted):
            full, fits = _stores(m, s)
            out = jk.power_summary(full, fits, effects, plant=None if mask is None else torch.as_tensor(mask),
                                   z_hit=z, level=level)
            want = _numpy_summary(m, s, effects, np.ones(T, dtype=bool) if mask is None else mask, z, level)
            negative = any(f < 0 for f in effects)
            assert set(out) == set(NUMERIC) | {"n_planted", "n_screens", "effects", "level", "z_hit"} | (
                {"mde_neg"} if negative else set())
            for k in NUMERIC + (("mde_neg",) if negative else ()):
                assert out[k].dtype == torch.float64, k
                np.testing.assert_allclose(out[k].numpy(), want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
            assert out["power"].shape == (D, T) and out["power_mean"].shape == (D,) and out["mde"].shape == (T,)
            assert out["n_planted"] == (T if mask is None else int(mask.sum())) and out["n_screens"] == K
            assert out["effects"] == effects and out["level"] == level and out["z_hit"] == z
            assert bool(torch.isnan(out["shrinkage"][effects.index(0.0)]))
            if mask is not None and not mask.all():
                assert bool(torch.isnan(out["power"][:, ~torch.as_tensor(mask)]).all())
                assert bool(torch.isnan(out["mde"][~torch.as_tensor(mask)]).all())
                assert not bool(torch.isnan(out["mu_power_mean"]).any())


def _fixed(power_rows, effects, K=4):
    """Fits whose power is exactly power_rows (D, T), each a multiple of 1 / K: m = +-10 where detected, else 0."""
    rows = np.asarray(power_rows, dtype=np.float64)
    D, T = rows.shape
    m = np.zeros((D, K, T))
    for i in range(D):
        for t in range(T):
            n = int(round(rows[i, t] * K))
            assert n / K == rows[i, t]
            m[i, :n, t] = 10.0 if effects[i] >= 0 else -10.0
    return _stores(m, np.ones((D, K, T)))


def test_power_summary_edges():
    effects = [0.0, 0.5, 1.0, 2.0]
    #          never  at the smallest  non-monotone  exactly met  met at the null
    rows = [[0.00, 0.00, 0.00, 0.00, 0.75],
            [0.25, 1.00, 0.75, 0.25, 0.00],
            [0.50, 0.00, 0.25, 0.75, 0.00],
            [0.50, 0.00, 1.00, 1.00, 1.00]]
    out = jk.power_summary(*_fixed(rows, effects), effects, level=0.75)
    assert torch.equal(out["power"], torch.tensor(rows, dtype=torch.float64))
    mde = out["mde"].tolist()
    assert mde[0] == float("inf")  # never detected often enough
    assert mde[1] == 0.5 * 0.75  # between the null and the smallest effect
    assert mde[2] == 0.5  # the FIRST crossing, although the power falls again behind it
    assert mde[3] == 1.0  # the level exactly met at an anchor: that anchor
    assert mde[4] == 0.5  # the null already reaches the level: the smallest positive effect
    assert "mde_neg" not in out
    assert out["power_mean"].tolist() == pytest.approx([0.15, 0.45, 0.3, 0.7], rel=1e-14)
    assert out["power_median"].tolist() == [0.0, 0.25, 0.25, 1.0]
    # the effects in another order give the same anchors; negative effects have their own curve
    order = [2, 0, 3, 1]
    again = jk.power_summary(*_fixed([rows[i] for i in order], [effects[i] for i in order]), [effects[i] for i in order],
                             level=0.75)
    assert again["mde"].tolist() == mde
    mirrored = [-f for f in effects]
    neg = jk.power_summary(*_fixed(rows, mirrored), mirrored, level=0.75)
    assert neg["mde_neg"].tolist() == mde and bool(torch.isinf(neg["mde"]).all())
    # a detection needs the effect's sign off the null, either sign at it
    m = np.full((2, 2, 3), 5.0)
    m[:, :, 1] = -5.0
    m[:, 1, 2] = float("nan")
    out = jk.power_summary(*_stores(m, np.ones_like(m)), [0.0, -1.0])
    assert out["power"].tolist() == [[1.0, 1.0, 0.5], [0.0, 1.0, 0.0]]  # a NaN fit detects nothing
    assert bool(torch.isnan(out["mu_power_mean"][:, 2]).all()) and bool(torch.isnan(out["mu_power_se"][:, 2]).all())
    # nothing planted: NaN throughout, not an error
    out = jk.power_summary(*_fixed(rows, effects), effects, plant=torch.zeros(5, dtype=torch.bool))
    assert out["n_planted"] == 0
    for k in ("power", "power_mean", "power_median", "shrinkage", "mde"):
        assert bool(torch.isnan(out[k]).all()), k
    assert not bool(torch.isnan(out["mu_power_mean"]).any())
    # fewer than two screens, ragged rows, the wrong number of rows, no null, a mask of another length
    full, fits = _fixed(rows, effects)
    with pytest.raises(ValueError, match="at least two screens"):
        jk.power_summary(full, [row[:1] for row in fits], effects)
    with pytest.raises(ValueError, match="at least two screens"):
        jk.power_summary(full, [fits[0], fits[1][:3], fits[2], fits[3]], effects)
    with pytest.raises(ValueError, match="per effect"):
        jk.power_summary(full, fits[:3], effects)
    with pytest.raises(ValueError, match="effect 0"):
        jk.power_summary(full, fits, [0.25, 0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match="plant has 4 entries for 5 targets"):
        jk.power_summary(full, fits, effects, plant=torch.ones(4, dtype=torch.bool))


def test_power_columns_and_table(tmp_path):
    import pandas as pd

    from bean_amd.model.readwrite import write_result_table

    T, effects = 3, [0.0, 0.25, -1.0]
    targets = pd.DataFrame({"x": range(T)}, index=[f"t{k}" for k in range(T)])
    guides = pd.DataFrame({"y": range(4)}, index=[f"g{k}" for k in range(4)])
    params = {"mu_loc": torch.tensor([[0.1], [0.2], [-0.3]]), "mu_scale": torch.full((T, 1), 0.5),
              "sd_loc": torch.zeros(T, 1), "sd_scale": torch.ones(T, 1)}
    nan, inf = float("nan"), float("inf")
    rates = torch.tensor([[0.0, nan, 0.2], [0.4, nan, 0.6], [1.0, nan, 0.8]], dtype=torch.float64)
    summary = {"power": rates, "effects": effects, "n_screens": 5, "n_planted": 2, "level": 0.8, "z_hit": 1.96,
               "power_mean": torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64),
               "power_median": torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64),
               "shrinkage": torch.tensor([nan, 0.7, 0.6], dtype=torch.float64),
               "mu_power_mean": torch.zeros(3, T, dtype=torch.float64),
               "mu_power_se": torch.tensor([[1.0, 9.0, 3.0], [2.0, 9.0, 6.0], [0.5, 9.0, 1.5]], dtype=torch.float64),
               "mde": torch.tensor([inf, nan, 0.2], dtype=torch.float64),
               "mde_neg": torch.tensor([0.75, nan, 1.0], dtype=torch.float64)}
    kw = dict(model_label="M", adjust_confidence_by_negative_control=False)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    (tmp_path / "c").mkdir()
    write_result_table(targets, guides.copy(), params, prefix=f"{tmp_path}/a/", **kw)
    write_result_table(targets, guides.copy(), params, prefix=f"{tmp_path}/b/", power=summary, **kw)
    assert sorted(os.listdir(tmp_path / "a")) == ["bean_element_result.M.csv", "bean_sgRNA_result.M.csv"]
    assert sorted(os.listdir(tmp_path / "b")) == ["bean_element_result.M.csv", "bean_power.M.csv", "bean_sgRNA_result.M.csv"]
    assert (tmp_path / "a" / "bean_sgRNA_result.M.csv").read_bytes() == (tmp_path / "b" / "bean_sgRNA_result.M.csv").read_bytes()
    plain, el = pd.read_csv(tmp_path / "a" / "bean_element_result.M.csv"), pd.read_csv(tmp_path / "b" / "bean_element_result.M.csv")
    new = ["power_x0", "power_x0.25", "power_x-1", "mde80", "mde80_neg"]
    assert [c for c in el.columns if c not in plain.columns] == new
    pd.testing.assert_frame_equal(el.drop(columns=new), plain)  # (the rows are ranked by z: the same order in both)
    assert sorted(el["index"]) == list(targets.index)
    by_name = el.sort_values("index")
    np.testing.assert_array_equal(by_name[new[:3]].values.T, rates.numpy())
    np.testing.assert_array_equal(by_name["mde80"].values, [inf, nan, 0.2])
    np.testing.assert_array_equal(by_name["mde80_neg"].values, [0.75, nan, 1.0])
    table = pd.read_csv(tmp_path / "b" / "bean_power.M.csv")
    assert list(table.columns) == ["effect", "n_screens", "n_planted", "power_mean", "power_median", "shrinkage",
                                   "median_mu_power_se"]
    assert table["effect"].tolist() == effects and table["median_mu_power_se"].tolist() == [2.0, 4.0, 1.0]  # planted targets
    assert table["n_screens"].tolist() == [5] * 3 and table["n_planted"].tolist() == [2] * 3
    assert table["power_mean"].tolist() == [0.1, 0.5, 0.9] and np.isnan(table["shrinkage"][0])
    assert table["shrinkage"].tolist()[1:] == [0.7, 0.6]
    # another level names its column; without negative effects there is no _neg column
    other = {k: v for k, v in summary.items() if k != "mde_neg"}
    other["level"] = 0.5
    got = write_result_table(targets, guides.copy(), params, prefix=f"{tmp_path}/c/", power=other, return_result=True, **kw)
    assert [c for c in got.columns if c.startswith("mde")] == ["mde50"]
    assert sorted(os.listdir(tmp_path / "c")) == ["bean_power.M.csv", "bean_sgRNA_result.M.csv"]
    with pytest.raises(ValueError, match="the power study summary"):
        write_result_table(targets, guides.copy(), params, prefix=f"{tmp_path}/b/", power={**summary, "power": rates[:, :2]}, **kw)


# ---------------------------------------------------------------- the flags
def _parser_refuses(argv):
    from bean_amd.cli.execute import main

    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2
    return " ".join(err.getvalue().split())


def test_flag_defaults_and_mode():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import check_run_switches, get_parser
    from bean_amd.model.parser import parse_args

    parser = get_parser()
    args = parser.parse_args(RUN)
    assert args.power_effects is None and args.power_screens == 8 and args.power_seed == 101 and args.power_level == 0.8
    assert cli_run.member_mode(args) is None and cli_run.member_mode(argparse.Namespace()) is None
    args = parser.parse_args(RUN + ["--power-effects", "0.1,0.2, 0.4", "--power-screens", "3", "--power-seed", "7",
                                    "--power-level", "0.9"])
    assert args.power_effects == [0.1, 0.2, 0.4] and args.power_screens == 3 and args.power_seed == 7
    assert args.power_level == 0.9 and cli_run.member_mode(args) == "power"
    # negatives, and a list that begins with one
    assert parser.parse_args(RUN + ["--power-effects", "0.5,-0.5,1e-1"]).power_effects == [0.5, -0.5, 0.1]
    assert parser.parse_args(RUN + ["--power-effects=-1,2"]).power_effects == [-1.0, 2.0]
    assert parser.parse_args(RUN + ["--power-effects", "0"]).power_effects == [0.0]
    assert "power" in cli_run.MEMBER_RUNS and cli_run.MEMBER_RUNS["power"][1] == "power"
    assert [attr for attr, mode, _ in cli_run.MEMBER_FLAGS if mode == "power"] == ["power_effects"]
    # --power-screens alone asks for nothing
    assert cli_run.member_mode(parser.parse_args(RUN + ["--power-screens", "1"])) is None
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    for name in ("power_effects", "power_screens", "power_seed", "power_level"):
        assert not hasattr(plain.parse_args(RUN[1:]), name)  # the reference's flag table stays as it is
    both = parser.parse_args(RUN + EFFECTS + ["--posterior-predictive", "5"])
    assert cli_run.predictive_draws(both) == 5 and cli_run.member_mode(both) == "power"
    check_run_switches(parser, both)


@pytest.mark.parametrize("value,sentence", [
    ("0.5,large", "'large' is not a number: a comma-separated list of effects such as 0.1,0.2,0.4 is expected"),
    ("0.5,,2", "'' is not a number"),
    ("", "'' is not a number"),
    ("0.5,2,0.50", "effect 0.5 is given more than once"),
    ("=-1,2,-1.0", "effect -1 is given more than once"),
    ("nan", "a planted effect must be a finite number, got nan"),
    ("inf,2", "a planted effect must be a finite number, got inf"),
    ("=-inf", "a planted effect must be a finite number, got -inf"),
])
def test_bad_effect_lists_are_refused(value, sentence):
    argv = RUN + (["--power-effects" + value] if value.startswith("=") else ["--power-effects", value])
    assert sentence in _parser_refuses(argv)


@pytest.mark.parametrize("value", ["0", "1", "1.5", "-0.2", "high"])
def test_a_level_outside_the_open_unit_interval_is_refused(value):
    said = _parser_refuses(RUN + EFFECTS + ["--power-level=" + value])
    assert "argument --power-level:" in said and ("invalid" in said if value == "high" else f"must be in (0, 1), got {value}" in said)


def test_one_screen_per_effect_is_refused():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + EFFECTS + ["--power-screens", "1"]
    sentence = "--power-effects needs at least 2 screens per effect (--power-screens)."
    assert sentence in _parser_refuses(argv)
    with pytest.raises(ValueError, match=re.escape(sentence)):
        cli_run.member_mode(get_parser().parse_args(argv))
    assert "must be >= 1" in _parser_refuses(RUN + EFFECTS + ["--power-screens", "0"])


@pytest.mark.parametrize("extra,sentence", [
    (["--n-seeds", "2"], "--power-effects fits every member with the same seed and does not combine with --n-seeds > 1."),
    (["--jackknife-replicates"], "--jackknife-replicates and --power-effects are two runs: they do not combine in one."),
    (["--jackknife-guides"], "--jackknife-guides and --power-effects are two runs: they do not combine in one."),
    (["--jackknife-samples"], "--jackknife-samples and --power-effects are two runs: they do not combine in one."),
    (["--jackknife-conditions"], "--jackknife-conditions and --power-effects are two runs: they do not combine in one."),
    (["--bootstrap", "4"], "--bootstrap and --power-effects are two runs: they do not combine in one."),
    (["--design-depths", "0.5,2"], "--design-depths and --power-effects are two runs: they do not combine in one."),
    (["--load-existing"], "--power-effects needs the refits of its simulated screens and does not combine with --load-existing."),
    (["--num-particles", "2"], "--num-particles averages draws inside one fit and does not combine with --power-effects"),
])
def test_combinations_are_refused_by_the_parser_and_by_member_mode(extra, sentence):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + EFFECTS + extra
    assert sentence in _parser_refuses(argv)
    args = get_parser().parse_args(argv)
    check = cli_run.particle_count if extra[0] == "--num-particles" else cli_run.member_mode
    with pytest.raises(ValueError, match=re.escape(sentence)):
        check(args)


@pytest.mark.parametrize("attr", ["jackknife_replicates", "jackknife_guides", "jackknife_samples", "jackknife_conditions",
                                  "bootstrap", "design_depths"])
def test_two_runs_in_both_directions(attr):
    from bean_amd.cli import run as cli_run

    value = {"bootstrap": 4, "design_depths": [0.5, 2.0]}.get(attr, True)
    args = argparse.Namespace(power_effects=[0.5, 2.0], **{attr: value})
    flag = "--" + attr.replace("_", "-")
    with pytest.raises(ValueError, match=re.escape(f"--power-effects and {flag} are two runs: they do not combine in one.")):
        cli_run.member_mode(args, only=("power_effects",))
    with pytest.raises(ValueError, match=re.escape(f"{flag} and --power-effects are two runs: they do not combine in one.")):
        cli_run.member_mode(args, only=(attr,))


@pytest.mark.parametrize("selection,design,named", [("sorting", "tiling", "tiling screens (MultiMixtureNormal)"),
                                                     ("survival", "variant", "survival screens"),
                                                     ("survival", "tiling", "tiling screens (MultiMixtureNormal)")])
def test_unsupported_families_are_refused_at_the_parser_with_the_family_named(selection, design, named):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = ["run", selection, design, "screen.h5ad"] + EFFECTS
    sentence = ("--power-effects simulates the counts of the sorting variant models (Normal, MixtureNormal) and is not "
                f"available for {named}.")
    assert sentence in _parser_refuses(argv)
    with pytest.raises(ValueError, match=re.escape(sentence)):
        cli_run.member_mode(get_parser().parse_args(argv))
    assert cli_run.member_mode(get_parser().parse_args(argv[:-2])) is None  # without the flag nothing is refused


# ---------------------------------------------------------------- run_inference_power refuses before any engine
def test_power_effects_puts_the_null_in_front():
    import bean_amd.model.run as model_run

    assert model_run.power_effects([0.25, -4]) == [0.0, 0.25, -4.0]
    assert model_run.power_effects([0.25, 0, 4]) == [0.25, 0.0, 4.0]
    assert model_run.power_effects((0,)) == [0.0]
    assert model_run.power_effects([-0.0, 1]) == [-0.0, 1.0]  # (minus zero is zero)
    with pytest.raises(ValueError, match="at least one effect"):
        model_run.power_effects([])
    with pytest.raises(ValueError, match="effect 0.5 is given more than once"):
        model_run.power_effects([0.5, 2.0, 0.5])
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite number"):
            model_run.power_effects([0.5, bad])


def test_run_inference_power_refuses_before_an_engine_is_built(monkeypatch):
    import bean_amd.model.model as m
    import bean_amd.model.run as model_run
    import bean_amd.model.survival_model as sm
    from bean_amd.engine import PredictiveUnsupported

    def no_engine(*a, **k):
        raise AssertionError("an engine was built")

    monkeypatch.setattr(model_run, "build_engine", no_engine)
    monkeypatch.setattr(model_run, "run_inference", no_engine)
    screen = lambda **kw: types.SimpleNamespace(**{"selection": "sorting", "library_design": "variant", **kw})  # noqa: E731
    for model, guide, data, named in (
        (partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide), screen(library_design="tiling"), "MultiMixtureNormal"),
        (partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide), screen(selection="survival"), "survival"),
        (partial(m.ControlNormalModel), partial(m.ControlNormalGuide), screen(), "ControlNormal"),
        (partial(m.NormalModel), m.NormalGuide, screen(sample_covariates=["batch"]), "sample covariates (Normal)"),
    ):
        with pytest.raises(PredictiveUnsupported, match=re.escape(named)):
            model_run.run_inference_power(model, guide, data, [0.5, 2.0], n_screens=4)
    fit = partial(model_run.run_inference_power, partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), screen())
    for n_screens in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2 screens"):
            fit([0.5, 2.0], n_screens=n_screens)
    with pytest.raises(ValueError, match="at least one effect"):
        fit([])
    with pytest.raises(ValueError, match="effect 0.5 is given more than once"):
        fit([0.5, 2.0, 0.5])
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite number"):
            fit([0.5, bad])
    for per_run in (0, 64):
        with pytest.raises(ValueError, match="max_per_run"):
            fit([0.5, 2.0], max_per_run=per_run)
