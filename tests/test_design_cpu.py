"""Depth study, the parts that need no GPU: the C entry point, the member plan, the summary, the --design-* flags with
their refusals, and what run_inference_design refuses before it builds an engine."""
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
NAME = "bean_hip_simulate_design"
RUN = ["run", "sorting", "variant", "screen.h5ad"]
DEPTHS = ["--design-depths", "0.5,2"]


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text), f"{NAME} not declared in bean_hip.h"
    # declared after the other simulators: every other kernel keeps its place in the code object
    assert text.index("bean_hip_simulate_members(") < text.index(NAME + "(")
    (entry,) = [s for s in _lib.SYMBOLS if s[0] == NAME]
    assert entry[1] is ctypes.c_int32 and len(entry[2]) == 11
    assert NAME in _lib.ENSEMBLE_SYMBOLS
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), NAME), f"{NAME} not exported by {_lib.tree_path(build)}"


def test_null_handle_is_rejected_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    one = (ctypes.c_double * 1)(1.0)
    assert lib.bean_hip_simulate_design(None, 1, 0, 4, one, 1, None, 0, None, 0, None) < 0
    msg = lib.bean_hip_last_error().decode()
    assert "simulate_design" in msg and "null handle" in msg, msg


# ---------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def screen():
    return make_sorting_variant_screen(40, 2, seed=1, mask_fraction=0.05)


def _planes(data, D, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 50, (D, K) + tuple(data.X_masked.shape), generator=g).to(data.X_masked.dtype)


@pytest.mark.parametrize("with_bc", [True, False])
def test_design_plan(screen, with_bc):
    data = screen
    depths, K = [1.0, 0.25, 4.0], 3
    D = len(depths)
    x, xbc = _planes(data, D, K, 1), (_planes(data, D, K, 2) if with_bc else None)
    before = {k: v.clone() for k, v in vars(data).items() if torch.is_tensor(v)}
    ids = {k: id(v) for k, v in vars(data).items()}
    plan = jk.design_plan(data, 7, depths, x, xbc)
    assert isinstance(plan, jk.MemberPlan)
    assert list(plan.seeds) == [7] * (1 + D * K)  # common random numbers: the members differ through their data
    text = ["1", "0.25", "4"]
    assert list(plan.labels) == ["the full screen"] + [f"depth {t} screen {j}" for t in text for j in range(K)]
    assert list(plan.tags) == ["full"] + [f"depth{t}_{j}" for t in text for j in range(K)]
    assert list(plan.dump_extra) == [{"depth": None, "screen": None, "seed": 7}] + [
        {"depth": f, "screen": j, "seed": 7} for f in depths for j in range(K)]
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
        jk.design_plan(data, 7, depths, x, x[:, :2])
    with pytest.raises(ValueError, match=r"\(D, K, R, B, G\)"):
        jk.design_plan(data, 7, depths, x[:2])
    with pytest.raises(ValueError, match=r"\(D, K, R, B, G\)"):
        jk.design_plan(data, 7, depths, x[0])


# ---------------------------------------------------------------- the summary
def _numpy_summary(centre, scale, m, s, depths, z):
    """design_summary restated: centre, scale (T,), m, s (D, K, T)."""
    base = depths.index(1.0)
    se = m.std(1, ddof=1)
    den = se[base]
    ok = np.isfinite(den) & (den != 0)
    ratio = np.array([np.median(se[i][ok] / den[ok]) if ok.any() else np.nan for i in range(len(depths))])
    hit = np.abs(centre) / scale >= z
    found = (np.sign(m) == np.sign(centre)) & (np.abs(m) / s >= z)
    rec = found[:, :, hit].mean((1, 2)) if hit.any() else np.full(len(depths), np.nan)
    return se, s.mean(1), ratio, int((~ok).sum()), np.nonzero(hit)[0].tolist(), rec


def _stores(centre, scale, m, s):
    full = {"mu_loc": torch.as_tensor(centre).reshape(-1, 1), "mu_scale": torch.as_tensor(scale).reshape(-1, 1)}
    fits = [[({"mu_loc": torch.as_tensor(m[i, j]).reshape(-1, 1), "mu_scale": torch.as_tensor(s[i, j]).reshape(-1, 1)},
              {"loss": []}) for j in range(m.shape[1])] for i in range(m.shape[0])]
    return full, fits


def test_design_summary_is_numpys():
    rng = np.random.default_rng(5)
    for T, K, depths, z in ((7, 2, [1.0, 0.5], 1.0), (12, 9, [0.25, 1.0, 4.0], 1.96), (1, 5, [1.0], 0.5)):
        D = len(depths)
        centre, scale = rng.normal(size=T), 0.2 + rng.random(T)
        m, s = rng.normal(size=(D, K, T)), 0.2 + rng.random((D, K, T))
        full, fits = _stores(centre, scale, m, s)
        out = jk.design_summary(full, fits, depths, z_hit=z)
        assert set(out) == {"mu_design_se", "mu_design_sd", "se_ratio", "n_left_out", "hits", "n_hits", "recovery",
                            "n_screens", "median_total", "depths"}
        se, sd, ratio, left, hits, rec = _numpy_summary(centre, scale, m, s, depths, z)
        for k in ("mu_design_se", "mu_design_sd", "se_ratio", "recovery", "median_total"):
            assert out[k].dtype == torch.float64, k
        assert out["mu_design_se"].shape == (D, T) and out["se_ratio"].shape == (D,) and out["recovery"].shape == (D,)
        np.testing.assert_allclose(out["mu_design_se"].numpy(), se, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out["mu_design_sd"].numpy(), sd, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out["se_ratio"].numpy(), ratio, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out["recovery"].numpy(), rec, rtol=1e-12, atol=0, equal_nan=True)
        assert out["se_ratio"][depths.index(1.0)] == 1.0
        assert out["hits"] == hits and out["n_hits"] == len(hits) and out["n_left_out"] == left == 0
        assert out["n_screens"] == K and out["depths"] == depths
        assert bool(torch.isnan(out["median_total"]).all())  # no screen given


def test_design_summary_edges(screen):
    rng = np.random.default_rng(6)
    T, K, depths = 6, 4, [1.0, 2.0]
    centre, scale = rng.normal(size=T), np.full(T, 1e3)  # no |z| reaches 1.96: the hit set is empty
    m, s = rng.normal(size=(2, K, T)), 0.2 + rng.random((2, K, T))
    m[0, :, 2] = 0.75  # the baseline's refits agree exactly on target 2: a zero denominator
    m[0, :, 4] = np.nan  # and are not finite on target 4
    full, fits = _stores(centre, scale, m, s)
    out = jk.design_summary(full, fits, depths)
    assert out["n_hits"] == 0 and out["hits"] == [] and bool(torch.isnan(out["recovery"]).all())
    assert out["n_left_out"] == 2
    se, _, ratio, left, _, _ = _numpy_summary(centre, scale, m, s, depths, 1.96)
    assert left == 2
    np.testing.assert_allclose(out["se_ratio"].numpy(), ratio, rtol=1e-12, atol=0)
    # every denominator left out: NaN, not an error
    m[0] = 1.0
    out = jk.design_summary(*_stores(centre, scale, m, s), depths)
    assert out["n_left_out"] == T and bool(torch.isnan(out["se_ratio"]).all())
    # fewer than two screens, ragged rows, the wrong number of rows, no baseline
    full, fits = _stores(centre, scale, m, s)
    with pytest.raises(ValueError, match="at least two screens"):
        jk.design_summary(full, [row[:1] for row in fits], depths)
    with pytest.raises(ValueError, match="at least two screens"):
        jk.design_summary(full, [fits[0], fits[1][:3]], depths)
    with pytest.raises(ValueError, match="per depth"):
        jk.design_summary(full, fits[:1], depths)
    with pytest.raises(ValueError, match="depth 1"):
        jk.design_summary(full, fits, [0.5, 2.0])
    # the median total: floor(f n + 0.5) over the pairs repguide_mask keeps, float64 on the host
    data = screen
    T = int(data.n_targets)
    m, s = rng.normal(size=(3, 2, T)), np.ones((3, 2, T))
    out = jk.design_summary(*_stores(np.ones(T), np.ones(T), m, s), [1.0, 0.5, 3.0], data=data)
    n = data.X_masked.double().sum(1).numpy()[data.repguide_mask.numpy() != 0]
    want = [np.median(np.floor(f * n + 0.5)) for f in (1.0, 0.5, 3.0)]
    assert not bool(data.repguide_mask.bool().all())
    np.testing.assert_allclose(out["median_total"].numpy(), want, rtol=0, atol=0)
    assert torch.equal(jk.design_totals(torch.tensor([0.0, 1.0, 3.0, 5.0]), 0.5), torch.tensor([0.0, 1.0, 2.0, 3.0]).double())


def test_design_columns_and_table(tmp_path):
    import pandas as pd

    from bean_amd.model.readwrite import write_result_table

    T, depths = 3, [1.0, 0.25, 4.0]
    targets = pd.DataFrame({"x": range(T)}, index=[f"t{k}" for k in range(T)])
    guides = pd.DataFrame({"y": range(4)}, index=[f"g{k}" for k in range(4)])
    params = {"mu_loc": torch.tensor([[0.1], [0.2], [-0.3]]), "mu_scale": torch.full((T, 1), 0.5),
              "sd_loc": torch.zeros(T, 1), "sd_scale": torch.ones(T, 1)}
    se = torch.tensor([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.5, 1.0, 1.5]], dtype=torch.float64)
    summary = {"mu_design_se": se, "depths": depths, "n_screens": 5, "n_hits": 2,
               "median_total": torch.tensor([100.0, 25.0, 400.0], dtype=torch.float64),
               "se_ratio": torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64),
               "recovery": torch.tensor([0.5, 0.25, float("nan")], dtype=torch.float64)}
    kw = dict(model_label="M", adjust_confidence_by_negative_control=False)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    write_result_table(targets, guides.copy(), params, prefix=f"{tmp_path}/a/", **kw)
    write_result_table(targets, guides.copy(), params, prefix=f"{tmp_path}/b/", design=summary, **kw)
    assert sorted(os.listdir(tmp_path / "a")) == ["bean_element_result.M.csv", "bean_sgRNA_result.M.csv"]
    assert sorted(os.listdir(tmp_path / "b")) == ["bean_design.M.csv", "bean_element_result.M.csv", "bean_sgRNA_result.M.csv"]
    assert (tmp_path / "a" / "bean_sgRNA_result.M.csv").read_bytes() == (tmp_path / "b" / "bean_sgRNA_result.M.csv").read_bytes()
    plain, el = pd.read_csv(tmp_path / "a" / "bean_element_result.M.csv"), pd.read_csv(tmp_path / "b" / "bean_element_result.M.csv")
    new = ["mu_design_se_x1", "mu_design_se_x0.25", "mu_design_se_x4"]
    assert [c for c in el.columns if c not in plain.columns] == new
    pd.testing.assert_frame_equal(el.drop(columns=new), plain)  # (the rows are ranked by z: the same order in both)
    assert sorted(el["index"]) == list(targets.index)
    assert el.sort_values("index")[new].values.T.tolist() == se.tolist()
    table = pd.read_csv(tmp_path / "b" / "bean_design.M.csv")
    assert list(table.columns) == ["depth", "n_screens", "median_total", "median_mu_design_se", "se_ratio", "recovery", "n_hits"]
    assert table["depth"].tolist() == depths and table["median_mu_design_se"].tolist() == [2.0, 4.0, 1.0]
    assert table["n_screens"].tolist() == [5] * 3 and table["n_hits"].tolist() == [2] * 3
    assert table["recovery"].tolist()[:2] == [0.5, 0.25] and np.isnan(table["recovery"][2])
    with pytest.raises(ValueError, match="the depth study summary"):
        write_result_table(targets, guides.copy(), params, prefix=f"{tmp_path}/b/", design={**summary, "mu_design_se": se[:, :2]}, **kw)


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
    assert args.design_depths is None and args.design_screens == 8 and args.design_seed == 101
    assert cli_run.member_mode(args) is None and cli_run.member_mode(argparse.Namespace()) is None
    args = parser.parse_args(RUN + ["--design-depths", "0.25,0.5, 2,4", "--design-screens", "3", "--design-seed", "7"])
    assert args.design_depths == [0.25, 0.5, 2.0, 4.0] and args.design_screens == 3 and args.design_seed == 7
    assert cli_run.member_mode(args) == "design"
    assert parser.parse_args(RUN + ["--design-depths", "1e1"]).design_depths == [10.0]
    assert "design" in cli_run.MEMBER_RUNS and cli_run.MEMBER_RUNS["design"][1] == "design"
    assert [attr for attr, mode, _ in cli_run.MEMBER_FLAGS if mode == "design"] == ["design_depths"]
    # --design-screens alone asks for nothing
    assert cli_run.member_mode(parser.parse_args(RUN + ["--design-screens", "1"])) is None
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    for name in ("design_depths", "design_screens", "design_seed"):
        assert not hasattr(plain.parse_args(RUN[1:]), name)  # the reference's flag table stays as it is
    both = parser.parse_args(RUN + DEPTHS + ["--posterior-predictive", "5"])
    assert cli_run.predictive_draws(both) == 5 and cli_run.member_mode(both) == "design"
    check_run_switches(parser, both)


@pytest.mark.parametrize("value,sentence", [
    ("0.5,deep", "'deep' is not a number: a comma-separated list of depth factors such as 0.25,0.5,2,4 is expected"),
    ("0.5,,2", "'' is not a number"),
    ("", "'' is not a number"),
    ("0.5,2,0.50", "depth factor 0.5 is given more than once"),
    ("2,0", "a depth factor must be a finite number > 0, got 0"),
    ("=-1,2", "a depth factor must be a finite number > 0, got -1"),
    ("nan", "a depth factor must be a finite number > 0, got nan"),
    ("inf,2", "a depth factor must be a finite number > 0, got inf"),
])
def test_bad_depth_lists_are_refused(value, sentence):
    argv = RUN + (["--design-depths" + value] if value.startswith("=") else ["--design-depths", value])
    assert sentence in _parser_refuses(argv)


def test_one_screen_per_depth_is_refused():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + DEPTHS + ["--design-screens", "1"]
    sentence = "--design-depths needs at least 2 screens per depth (--design-screens)."
    assert sentence in _parser_refuses(argv)
    with pytest.raises(ValueError, match=re.escape(sentence)):
        cli_run.member_mode(get_parser().parse_args(argv))
    assert "must be >= 1" in _parser_refuses(RUN + DEPTHS + ["--design-screens", "0"])


@pytest.mark.parametrize("extra,sentence", [
    (["--n-seeds", "2"], "--design-depths fits every member with the same seed and does not combine with --n-seeds > 1."),
    (["--jackknife-replicates"], "--jackknife-replicates and --design-depths are two runs: they do not combine in one."),
    (["--jackknife-guides"], "--jackknife-guides and --design-depths are two runs: they do not combine in one."),
    (["--jackknife-samples"], "--jackknife-samples and --design-depths are two runs: they do not combine in one."),
    (["--jackknife-conditions"], "--jackknife-conditions and --design-depths are two runs: they do not combine in one."),
    (["--bootstrap", "4"], "--bootstrap and --design-depths are two runs: they do not combine in one."),
    (["--load-existing"], "--design-depths needs the refits of its simulated screens and does not combine with --load-existing."),
    (["--num-particles", "2"], "--num-particles averages draws inside one fit and does not combine with --design-depths"),
])
def test_combinations_are_refused_by_the_parser_and_by_member_mode(extra, sentence):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + DEPTHS + extra
    assert sentence in _parser_refuses(argv)
    args = get_parser().parse_args(argv)
    check = cli_run.particle_count if extra[0] == "--num-particles" else cli_run.member_mode
    with pytest.raises(ValueError, match=re.escape(sentence)):
        check(args)


@pytest.mark.parametrize("attr", ["jackknife_replicates", "jackknife_guides", "jackknife_samples", "jackknife_conditions",
                                  "bootstrap"])
def test_two_runs_in_both_directions(attr):
    from bean_amd.cli import run as cli_run

    args = argparse.Namespace(design_depths=[0.5, 2.0], **{attr: 4 if attr == "bootstrap" else True})
    flag = "--" + attr.replace("_", "-")
    with pytest.raises(ValueError, match=re.escape(f"--design-depths and {flag} are two runs: they do not combine in one.")):
        cli_run.member_mode(args, only=("design_depths",))
    with pytest.raises(ValueError, match=re.escape(f"{flag} and --design-depths are two runs: they do not combine in one.")):
        cli_run.member_mode(args, only=(attr,))


@pytest.mark.parametrize("selection,design,named", [("sorting", "tiling", "tiling screens (MultiMixtureNormal)"),
                                                     ("survival", "variant", "survival screens"),
                                                     ("survival", "tiling", "tiling screens (MultiMixtureNormal)")])
def test_unsupported_families_are_refused_at_the_parser_with_the_family_named(selection, design, named):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = ["run", selection, design, "screen.h5ad"] + DEPTHS
    sentence = ("--design-depths simulates the counts of the sorting variant models (Normal, MixtureNormal) and is not "
                f"available for {named}.")
    assert sentence in _parser_refuses(argv)
    with pytest.raises(ValueError, match=re.escape(sentence)):
        cli_run.member_mode(get_parser().parse_args(argv))
    assert cli_run.member_mode(get_parser().parse_args(argv[:-2])) is None  # without the flag nothing is refused


# ---------------------------------------------------------------- run_inference_design refuses before any engine
def test_design_depths_puts_the_baseline_in_front():
    import bean_amd.model.run as model_run

    assert model_run.design_depths([0.25, 4]) == [1.0, 0.25, 4.0]
    assert model_run.design_depths([0.25, 1, 4]) == [0.25, 1.0, 4.0]
    assert model_run.design_depths((1,)) == [1.0]


def test_run_inference_design_refuses_before_an_engine_is_built(monkeypatch):
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
            model_run.run_inference_design(model, guide, data, [0.5, 2.0], n_screens=4)
    fit = partial(model_run.run_inference_design, partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), screen())
    for n_screens in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2 screens"):
            fit([0.5, 2.0], n_screens=n_screens)
    with pytest.raises(ValueError, match="at least one depth"):
        fit([])
    with pytest.raises(ValueError, match="depth factor 0.5 is given more than once"):
        fit([0.5, 2.0, 0.5])
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite number > 0"):
            fit([0.5, bad])
    for per_run in (0, 64):
        with pytest.raises(ValueError, match="max_per_run"):
            fit([0.5, 2.0], max_per_run=per_run)


# ---------------------------------------------------------------- the law at another depth, on the host
@pytest.mark.parametrize("seed", [20261, 20262, 20263])
@pytest.mark.parametrize("regime", ["moderate", "sparse"])
def test_the_reference_sampler_passes_at_the_scaled_totals(regime, seed):
    """What test_gpu_design.py asks of the device's draws, asked of dm_reference.host_dm driven at floor(f n + 0.5): a
    correct sampler passes every check at these sizes (64 draws, threshold 1e-3 / N_P)."""
    import dm_reference as dm

    import design_common as dc

    n_obs = dm.regime_totals(regime)
    assert bool((n_obs % 2 == 1).any())  # odd totals: at depth 0.5 rounding and truncating differ
    for depth in dc.LAW_DEPTHS:
        x, alpha = dc.host_draws(regime, dc.scaled_totals(n_obs, depth), seed)
        rep = dc.law_report(regime, depth, x, n_obs, alpha, np.random.default_rng(seed))
        print(dc.describe(rep))
        assert len(rep["p"]) == dc.N_PVALUES[dc.label(regime, depth)]
        assert dc.failures(rep) == []
    assert sum(dc.N_PVALUES.values()) == dc.N_P == 95 and dc.P_MIN == 1e-3 / 95


@pytest.mark.parametrize("regime", ["moderate", "sparse"])
def test_planted_depth_faults_fail(regime):
    """Totals left at the observed ones, and totals truncated instead of rounded (depth 0.5, odd totals), are both seen."""
    import dm_reference as dm

    import design_common as dc

    n_obs = dm.regime_totals(regime)
    odd = int((n_obs % 2 == 1).sum())
    assert odd > 0
    for depth in dc.LAW_DEPTHS:
        x, alpha = dc.host_draws(regime, n_obs, 20261)  # not scaled
        rep = dc.law_report(regime, depth, x, n_obs, alpha, np.random.default_rng(1))
        assert rep["totals"] > 0 and dc.failures(rep) != []
    truncated = np.floor(0.5 * n_obs).astype(np.int64)
    x, alpha = dc.host_draws(regime, truncated, 20261)
    rep = dc.law_report(regime, 0.5, x, n_obs, alpha, np.random.default_rng(1))
    assert rep["totals"] == dc.LAW_DRAWS * odd and dc.failures(rep) != []  # exactly the pairs of odd totals
    assert np.array_equal(dc.scaled_totals(n_obs, 0.5) - truncated, n_obs % 2)
