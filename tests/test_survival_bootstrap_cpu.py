"""The survival bootstrap without a GPU: the --survival-bootstrap flag with its refusals, what run_survival_bootstrap
refuses before it builds an engine, the plug-in noise of survival_bootstrap_engine and the batching of
survival_bootstrap_screens on a stub engine, the C entry point and its binding."""
import argparse
import contextlib
import ctypes
import io
import os
import re
import types
from functools import partial

import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bean_hip_simulate_survival_members"
RUN = ["run", "survival", "variant", "screen.h5ad"]
FLAG = "--survival-bootstrap"


def _parser_refuses(argv):
    from bean_amd.cli.execute import main

    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2
    return " ".join(err.getvalue().split())


# ---------------------------------------------------------------- the flag
def test_flag_defaults_and_mode():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import check_run_switches, get_parser
    from bean_amd.model.parser import parse_args

    parser = get_parser()
    args = parser.parse_args(RUN)
    assert args.survival_bootstrap == 0 and args.bootstrap_seed == 101
    assert cli_run.member_mode(args) is None and cli_run.member_mode(argparse.Namespace()) is None
    args = parser.parse_args(RUN + [FLAG, "32", "--bootstrap-seed", "7"])
    assert args.survival_bootstrap == 32 and args.bootstrap_seed == 7 and args.bootstrap == 0
    assert cli_run.member_mode(args) == "survival_bootstrap"
    assert cli_run.member_mode(parser.parse_args(RUN + [FLAG, "0"])) is None  # 0 is off
    # the raw key is the bootstrap's; the existing rows of the table are where they were
    assert cli_run.MEMBER_RUNS["survival_bootstrap"][1] == "bootstrap"
    assert [attr for attr, mode, _ in cli_run.MEMBER_FLAGS if mode == "survival_bootstrap"] == ["survival_bootstrap"]
    assert [attr for attr, _, _ in cli_run.MEMBER_FLAGS][:7] == [
        "jackknife_replicates", "jackknife_guides", "jackknife_samples", "jackknife_conditions", "bootstrap",
        "design_depths", "power_effects"]
    for bad in ("-1", "many"):
        with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(io.StringIO()):
            parser.parse_args(RUN + [FLAG, bad])
        assert exc.value.code == 2
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    assert not hasattr(plain.parse_args(RUN[1:]), "survival_bootstrap")  # the reference's flag table stays as it is
    both = parser.parse_args(RUN + [FLAG, "4", "--survival-predictive", "5"])
    assert cli_run.survival_predictive_draws(both) == 5 and cli_run.member_mode(both) == "survival_bootstrap"
    check_run_switches(parser, both)
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    assert FLAG in help_text and "mu_boot_se" in help_text


_TWO = "{} and {} are two runs: they do not combine in one."


@pytest.mark.parametrize("extra,sentence", [
    (["--n-seeds", "2"], FLAG + " fits every member with the same seed and does not combine with --n-seeds > 1."),
    (["--jackknife-replicates"], _TWO.format(FLAG, "--jackknife-replicates")),
    (["--jackknife-guides"], _TWO.format(FLAG, "--jackknife-guides")),
    (["--jackknife-samples"], _TWO.format(FLAG, "--jackknife-samples")),
    (["--jackknife-conditions"], _TWO.format(FLAG, "--jackknife-conditions")),
    (["--load-existing"], FLAG + " needs the refits of its simulated screens and does not combine with --load-existing."),
    (["--num-particles", "2"], "--num-particles averages draws inside one fit and does not combine with " + FLAG),
])
def test_combinations_are_refused_by_the_parser_and_by_member_mode(extra, sentence):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + [FLAG, "4"] + extra
    assert sentence in _parser_refuses(argv)
    args = get_parser().parse_args(argv)
    check = cli_run.particle_count if extra[0] == "--num-particles" else cli_run.member_mode
    with pytest.raises(ValueError, match=re.escape(sentence)):
        check(args)


@pytest.mark.parametrize("attr,value", [("bootstrap", 4), ("design_depths", [0.5, 2.0]), ("power_effects", [0.5])])
def test_the_other_simulated_studies_are_two_runs(attr, value):
    """Looked at alone, the survival bootstrap's own row refuses them (on a survival screen their own rows refuse the
    family first: test_bootstrap_still_refuses_survival_screens_with_its_own_sentence)."""
    from bean_amd.cli import run as cli_run

    args = argparse.Namespace(survival_bootstrap=4, selection="survival", library_design="variant", **{attr: value})
    other = "--" + attr.replace("_", "-")
    with pytest.raises(ValueError, match=re.escape(_TWO.format(FLAG, other))):
        cli_run.member_mode(args, only=("survival_bootstrap",))


@pytest.mark.parametrize("selection,design,named", [
    ("sorting", "variant", "sorting screens (--bootstrap serves them)"),
    ("sorting", "tiling", "tiling screens (MultiMixtureNormal)"),
    ("survival", "tiling", "tiling screens (MultiMixtureNormal)")])
def test_unsupported_families_are_refused_at_the_parser_with_the_family_named(selection, design, named):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = ["run", selection, design, "screen.h5ad", FLAG, "4"]
    sentence = (FLAG + " simulates the counts of the survival variant models (Normal, MixtureNormal) and is not "
                f"available for {named}.")
    assert sentence in _parser_refuses(argv)
    with pytest.raises(ValueError, match=re.escape(sentence)):
        cli_run.member_mode(get_parser().parse_args(argv))
    assert cli_run.member_mode(get_parser().parse_args(argv[:-2])) is None  # without the flag nothing is refused


def test_one_screen_is_refused():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    argv = RUN + [FLAG, "1"]
    assert FLAG + " needs at least 2 screens." in _parser_refuses(argv)
    with pytest.raises(ValueError, match="at least 2"):
        cli_run.member_mode(get_parser().parse_args(argv))


@pytest.mark.parametrize("extra", [[], [FLAG, "4"]])
def test_bootstrap_still_refuses_survival_screens_with_its_own_sentence(extra):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    sentence = ("--bootstrap simulates the counts of the sorting variant models (Normal, MixtureNormal) and is not "
                "available for survival screens.")
    argv = RUN + ["--bootstrap", "4"] + extra
    msg = _parser_refuses(argv)
    assert msg.endswith("error: " + sentence), msg
    with pytest.raises(ValueError) as exc:
        cli_run.member_mode(get_parser().parse_args(argv))
    assert str(exc.value) == sentence


# ---------------------------------------------------------------- run_survival_bootstrap refuses before any engine
def test_run_survival_bootstrap_refuses_before_an_engine_is_built(monkeypatch):
    import bean_amd.model.model as m
    import bean_amd.model.run as model_run
    import bean_amd.model.survival_model as sm
    from bean_amd.engine import PredictiveUnsupported

    def no_engine(*a, **k):
        raise AssertionError("an engine was built")

    monkeypatch.setattr(model_run, "build_engine", no_engine)
    monkeypatch.setattr(model_run, "run_inference", no_engine)
    screen = lambda **kw: types.SimpleNamespace(**{"selection": "survival", "library_design": "variant", **kw})  # noqa: E731
    for model, guide, data, named in (
        (partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), screen(selection="sorting"),
         "sorting screens (MixtureNormal)"),
        (partial(sm.MultiMixtureNormalModel), partial(sm.MultiMixtureNormalGuide), screen(library_design="tiling"),
         "tiling screens (MultiMixtureNormal)"),
        (partial(sm.ControlNormalModel), partial(sm.ControlNormalGuide), screen(), "ControlNormal"),
        (partial(sm.NormalModel), sm.NormalGuide, screen(sample_covariates=["batch"]), "sample covariates (Normal)"),
    ):
        with pytest.raises(PredictiveUnsupported, match=re.escape(named)) as exc:
            model_run.run_survival_bootstrap(model, guide, data, n_boot=4)
        assert "a survival bootstrap is not available for" in str(exc.value)
    for n_boot in (1, 0, -3):
        with pytest.raises(ValueError, match="a survival bootstrap needs at least 2 screens"):
            model_run.run_survival_bootstrap(partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide), screen(),
                                             n_boot=n_boot)


# ---------------------------------------------------------------- the plug-in and the batching on a stub engine
class _Stub:
    """What survival_bootstrap_engine and survival_bootstrap_screens use of an engine, on host tensors."""
    device = torch.device("cpu")

    def __init__(self, T, R, B, G, surv_normal, acc, use_bc=True):
        self.T, self.surv_normal, self.scale_by_accessibility, self.use_bc = T, surv_normal, acc, use_bc
        self.shape = (R, B, G)
        self.noise, self.calls, self.closed = None, [], False

    def set_noise(self, noise):
        self.noise = noise

    def simulate_survival_members(self, first_draw, n_draws, seed=101):
        self.calls.append((first_draw, n_draws, seed))
        # plane j of the whole set holds j (and 1000 + j in the barcode-matched counts)
        x = torch.arange(first_draw, first_draw + n_draws, dtype=torch.float32).reshape(-1, 1, 1, 1).expand(-1, *self.shape)
        return {"X": x.clone(), "X_bcmatch": x + 1000} if self.use_bc else {"X": x.clone()}

    def close(self):
        self.closed = True


def _plug_in(monkeypatch, surv_normal, acc, store):
    import bean_amd.model.run as model_run

    R, B, G, T = 3, 4, 5, 2
    stub = _Stub(T, R, B, G, surv_normal, acc)
    loaded = []
    data = types.SimpleNamespace(n_guides=G, n_reps=R)
    data.to = lambda device: data
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(model_run, "build_engine", lambda model, guide, d, **kw: stub)
    monkeypatch.setattr(model_run, "load_parameters", lambda eng, st: loaded.append((eng, st)))
    assert model_run.survival_bootstrap_engine("model", "guide", data, store) is stub
    assert loaded == [(stub, store)] and not stub.closed
    return stub


@pytest.mark.parametrize("surv_normal,acc,keys", [(True, False, {"eps_mu", "q_0"}),
                                                  (False, False, {"eps_mu"}),
                                                  (False, True, {"eps_mu", "eps_noise"})],
                         ids=["Normal", "MixtureNormal", "MixtureNormal+Acc"])
def test_plug_in_noise(monkeypatch, surv_normal, acc, keys):
    ia = torch.tensor([0.5, 1.5, 2.0, 0.25, 3.75], dtype=torch.float32)
    stub = _plug_in(monkeypatch, surv_normal, acc, {"initial_abundance": ia})
    noise = stub.noise
    assert set(noise) == keys and "eps_u" not in noise and "eps_sd" not in noise and "mu_negctrl" not in noise and "pi" not in noise
    for k, n in (("eps_mu", 2), ("eps_noise", 5)):
        if k in keys:
            assert noise[k].dtype == torch.float64 and noise[k].shape == (n,) and not bool(noise[k].any()), k
    if surv_normal:
        # the mean of Dirichlet(initial_abundance), the same for every replicate
        want = torch.tensor([0.0625, 0.1875, 0.25, 0.03125, 0.46875], dtype=torch.float64)
        assert noise["q_0"].dtype == torch.float64 and noise["q_0"].shape == (3, 5)
        assert torch.equal(noise["q_0"], want.expand(3, 5))


def test_plug_in_closes_the_engine_when_the_store_is_not_a_fit(monkeypatch):
    import bean_amd.model.run as model_run

    stub = _Stub(2, 3, 4, 5, True, False)
    data = types.SimpleNamespace(n_guides=5, n_reps=3)
    data.to = lambda device: data
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(model_run, "build_engine", lambda *a, **kw: stub)
    monkeypatch.setattr(model_run, "load_parameters", lambda eng, st: None)
    with pytest.raises(KeyError):
        model_run.survival_bootstrap_engine("model", "guide", data, {})
    assert stub.closed


@pytest.mark.parametrize("n_boot,calls", [(3, [(0, 3)]), (64, [(0, 64)]), (65, [(0, 64), (64, 1)]),
                                          (150, [(0, 64), (64, 64), (128, 22)])])
@pytest.mark.parametrize("use_bc", [True, False])
def test_screens_are_batched_with_the_draw_index_advancing(n_boot, calls, use_bc):
    from bean_amd.model.run import survival_bootstrap_screens

    assert _lib.MAX_MEMBERS == 64
    stub = _Stub(2, 2, 3, 4, False, False, use_bc=use_bc)
    x, x_bc = survival_bootstrap_screens(stub, n_boot, boot_seed=9)
    assert stub.calls == [(a, k, 9) for a, k in calls]
    assert x.shape == (n_boot, 2, 3, 4) and torch.equal(x[:, 0, 0, 0], torch.arange(n_boot, dtype=torch.float32))
    if use_bc:
        assert torch.equal(x_bc, x + 1000)
    else:
        assert x_bc is None


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    header = " ".join(open(os.path.join(ROOT, "include", "bean_hip.h")).read().split())
    assert ("int bean_hip_simulate_survival_members(bean_hip_ctx* ctx, uint64_t seed, uint64_t first_draw, int32_t n_draws, "
            "void* x_out, uint64_t x_bytes, void* xbc_out, uint64_t xbc_bytes, void* stream);") in header
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert bound[NAME] == bound["bean_hip_simulate_members"] and bound[NAME][0] is ctypes.c_int32 and len(bound[NAME][1]) == 9
    assert NAME in _lib.ENSEMBLE_SYMBOLS
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), NAME), f"{NAME} not exported by {_lib.tree_path(build)}"


def test_null_handle_is_rejected_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    assert lib.bean_hip_simulate_survival_members(None, 1, 0, 4, None, 0, None, 0, None) < 0
    assert lib.bean_hip_last_error().decode() == NAME + ": null handle"
