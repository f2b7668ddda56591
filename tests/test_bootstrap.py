"""Parametric bootstrap, the parts that need no GPU: the C entry point, the member plan, the summary, the --bootstrap
flag with its refusals, and what run_inference_bootstrap refuses before it builds an engine."""
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
NAME = "bean_hip_simulate_members"
RUN = ["run", "sorting", "variant", "screen.h5ad"]


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text), f"{NAME} not declared in bean_hip.h"
    # declared after bean_hip_simulate: every other kernel keeps its place in the code object
    assert text.index("bean_hip_simulate(") < text.index(NAME + "(")
    (entry,) = [s for s in _lib.SYMBOLS if s[0] == NAME]
    assert entry[1] is ctypes.c_int32 and len(entry[2]) == 9
    assert NAME in _lib.ENSEMBLE_SYMBOLS
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), NAME), f"{NAME} not exported by {_lib.tree_path(build)}"


def test_null_handle_is_rejected_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    assert lib.bean_hip_simulate_members(None, 1, 0, 4, None, 0, None, 0, None) < 0
    msg = lib.bean_hip_last_error().decode()
    assert "simulate_members" in msg and "null handle" in msg, msg


# ---------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def screen():
    return make_sorting_variant_screen(40, 2, seed=1, mask_fraction=0.05)


def _planes(data, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 50, (K,) + tuple(data.X_masked.shape), generator=g).to(data.X_masked.dtype)


@pytest.mark.parametrize("with_bc", [True, False])
def test_bootstrap_plan(screen, with_bc):
    data = screen
    K = 3
    x, xbc = _planes(data, K, 1), (_planes(data, K, 2) if with_bc else None)
    before = {k: v.clone() for k, v in vars(data).items() if torch.is_tensor(v)}
    ids = {k: id(v) for k, v in vars(data).items()}
    plan = jk.bootstrap_plan(data, 7, x, xbc)
    assert isinstance(plan, jk.MemberPlan)
    assert list(plan.seeds) == [7] * (1 + K)  # common random numbers: the members differ through their data
    assert list(plan.labels) == ["the full screen"] + [f"bootstrap screen {j}" for j in range(K)]
    assert list(plan.tags) == ["full"] + [f"bootstrap{j}" for j in range(K)]
    assert list(plan.dump_extra) == [{"bootstrap": None, "seed": 7}] + [{"bootstrap": j, "seed": 7} for j in range(K)]
    assert plan.differ_in == ("masks", "counts") and plan.per_run == 63
    assert plan.screen(0) is data
    for j in range(K):
        member = plan.screen(1 + j)
        assert member is not data and type(member) is type(data)
        assert torch.equal(member.X_masked, x[j])
        if with_bc:
            assert torch.equal(member.X_bcmatch_masked, xbc[j])
        changed = {"X_masked"} | ({"X_bcmatch_masked"} if with_bc else set())
        for name, value in vars(member).items():
            if name not in changed:  # masks, size factors, a0, pi_a0, the control allele counts: shared, conditioned on
                assert value is vars(data)[name], name
    for name in ("sample_mask", "repguide_mask", "size_factor", "a0", "pi_a0"):
        assert hasattr(data, name), name
    # data is not modified
    assert {k: id(v) for k, v in vars(data).items()} == ids
    for k, v in before.items():
        assert torch.equal(v, vars(data)[k], ) or (v != v).any(), k
    # what the engine binds as member counts are the planes
    got_x, got_bc = jk.stack_counts([plan.screen(1 + j) for j in range(K)])
    assert torch.equal(got_x, x.float())
    if with_bc:
        assert torch.equal(got_bc, xbc.float())
    else:
        assert torch.equal(got_bc, torch.stack([data.X_bcmatch_masked.float()] * K))
    with pytest.raises(ValueError, match="x_bcmatch"):
        jk.bootstrap_plan(data, 7, x, x[:2])


# ---------------------------------------------------------------- the summary
def test_bootstrap_summary_is_numpys():
    rng = np.random.default_rng(5)
    for T, n in ((7, 2), (5, 9), (1, 32)):
        centre = rng.normal(size=(T, 1))
        m = rng.normal(size=(n, T, 1))
        full = {"mu_loc": torch.as_tensor(centre)}
        boots = [({"mu_loc": torch.as_tensor(m[j])}, {"loss": []}) for j in range(n)]  # results or their stores
        out = jk.bootstrap_summary(full, boots)
        assert set(out) == {"mu_boot_se", "mu_boot_bias", "n_boot"} and out["n_boot"] == n
        assert out["mu_boot_se"].dtype == torch.float64 and out["mu_boot_bias"].dtype == torch.float64
        np.testing.assert_allclose(out["mu_boot_se"].numpy(), m.std(0, ddof=1), rtol=1e-12, atol=0)
        np.testing.assert_allclose(out["mu_boot_bias"].numpy(), m.mean(0) - centre, rtol=1e-12, atol=1e-15)
    for boots in ([], [{"mu_loc": torch.zeros(3, 1)}]):
        with pytest.raises(ValueError, match="at least two"):
            jk.bootstrap_summary({"mu_loc": torch.zeros(3, 1)}, boots)


def test_summary_columns_in_the_element_table():
    import pandas as pd

    from bean_amd.model.readwrite import _add_summary_columns

    element = pd.DataFrame({"mu": [0.1, 0.2, 0.3]})
    summary = {"mu_boot_se": torch.tensor([[1.0], [2.0], [3.0]], dtype=torch.float64),
               "mu_boot_bias": torch.tensor([[-1.0], [0.0], [1.0]], dtype=torch.float64), "n_boot": 4}
    _add_summary_columns(element, summary, "the bootstrap summary", ("mu_boot_se", "mu_boot_bias"), None, "n_boot")
    assert list(element.columns) == ["mu", "mu_boot_se", "mu_boot_bias", "n_boot"]
    assert element["mu_boot_se"].tolist() == [1.0, 2.0, 3.0] and element["n_boot"].tolist() == [4, 4, 4]
    with pytest.raises(ValueError, match="the bootstrap summary"):
        _add_summary_columns(element.iloc[:2].copy(), summary, "the bootstrap summary", ("mu_boot_se", "mu_boot_bias"),
                             None, "n_boot")


# ---------------------------------------------------------------- the flag
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
    assert args.bootstrap == 0 and args.bootstrap_seed == 101
    assert cli_run.member_mode(args) is None and cli_run.member_mode(argparse.Namespace()) is None
    args = parser.parse_args(RUN + ["--bootstrap", "32", "--bootstrap-seed", "7"])
    assert args.bootstrap == 32 and args.bootstrap_seed == 7 and cli_run.member_mode(args) == "bootstrap"
    assert cli_run.member_mode(parser.parse_args(RUN + ["--bootstrap", "0"])) is None  # 0 is off
    assert "bootstrap" in cli_run.MEMBER_RUNS and cli_run.MEMBER_RUNS["bootstrap"][1] == "bootstrap"
    for bad in ("-1", "many"):
        with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(io.StringIO()):
            parser.parse_args(RUN + ["--bootstrap", bad])
        assert exc.value.code == 2
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    assert not hasattr(plain.parse_args(RUN[1:]), "bootstrap")  # the reference's flag table stays as it is
    # --posterior-predictive keeps combining with it, as with the other member sets
    both = parser.parse_args(RUN + ["--bootstrap", "4", "--posterior-predictive", "5"])
    assert cli_run.predictive_draws(both) == 5 and cli_run.member_mode(both) == "bootstrap"
    check_run_switches(parser, both)


@pytest.mark.parametrize("extra,sentence", [
    (["--n-seeds", "2"], "--bootstrap fits every member with the same seed and does not combine with --n-seeds > 1."),
    (["--jackknife-replicates"], "--jackknife-replicates and --bootstrap are two runs: they do not combine in one."),
    (["--jackknife-guides"], "--jackknife-guides and --bootstrap are two runs: they do not combine in one."),
    (["--jackknife-samples"], "--jackknife-samples and --bootstrap are two runs: they do not combine in one."),
    (["--jackknife-conditions"], "--jackknife-conditions and --bootstrap are two runs: they do not combine in one."),
    (["--load-existing"], "--bootstrap needs the refits of its simulated screens and does not combine with --load-existing."),
    (["--num-particles", "2"], "--num-particles averages draws inside one fit and does not combine with --bootstrap"),
])
def test_combinations_are_refused_by_the_parser_and_by_member_mode(extra, sentence):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + ["--bootstrap", "4"] + extra
    assert sentence in _parser_refuses(argv)
    args = get_parser().parse_args(argv)
    check = cli_run.particle_count if extra[0] == "--num-particles" else cli_run.member_mode
    with pytest.raises(ValueError, match=re.escape(sentence)):
        check(args)


@pytest.mark.parametrize("attr", ["jackknife_replicates", "jackknife_guides", "jackknife_samples", "jackknife_conditions"])
def test_two_runs_in_both_directions(attr):
    """The bootstrap's own row refuses the jackknives too: looked at alone, it names itself first."""
    from bean_amd.cli import run as cli_run

    args = argparse.Namespace(bootstrap=4, **{attr: True})
    flag = "--" + attr.replace("_", "-")
    with pytest.raises(ValueError, match=re.escape(f"--bootstrap and {flag} are two runs: they do not combine in one.")):
        cli_run.member_mode(args, only=("bootstrap",))
    with pytest.raises(ValueError, match=re.escape(f"{flag} and --bootstrap are two runs: they do not combine in one.")):
        cli_run.member_mode(args, only=(attr,))


@pytest.mark.parametrize("selection,design,named", [("sorting", "tiling", "tiling screens (MultiMixtureNormal)"),
                                                     ("survival", "variant", "survival screens"),
                                                     ("survival", "tiling", "tiling screens (MultiMixtureNormal)")])
def test_unsupported_families_are_refused_at_the_parser_with_the_family_named(selection, design, named):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = ["run", selection, design, "screen.h5ad", "--bootstrap", "4"]
    sentence = ("--bootstrap simulates the counts of the sorting variant models (Normal, MixtureNormal) and is not "
                f"available for {named}.")
    assert sentence in _parser_refuses(argv)
    with pytest.raises(ValueError, match=re.escape(sentence)):
        cli_run.member_mode(get_parser().parse_args(argv))
    assert cli_run.member_mode(get_parser().parse_args(argv[:-2])) is None  # without the flag nothing is refused


def test_one_screen_is_refused():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + ["--bootstrap", "1"]
    assert "--bootstrap needs at least 2 screens." in _parser_refuses(argv)
    with pytest.raises(ValueError, match="at least 2"):
        cli_run.member_mode(get_parser().parse_args(argv))


# ---------------------------------------------------------------- run_inference_bootstrap refuses before any engine
def test_run_inference_bootstrap_refuses_before_an_engine_is_built(monkeypatch):
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
            model_run.run_inference_bootstrap(model, guide, data, n_boot=4)
    for n_boot in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2"):
            model_run.run_inference_bootstrap(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), screen(),
                                              n_boot=n_boot)
    for per_run in (0, 64):
        with pytest.raises(ValueError, match="max_per_run"):
            model_run.run_inference_bootstrap(partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), screen(),
                                              n_boot=4, max_per_run=per_run)
