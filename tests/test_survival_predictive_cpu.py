"""The survival posterior predictive check without a GPU: the power of the law check of tests/test_gpu_survival_predictive.py
(dm_reference.host_dm at its sizes: the correct sampler passes its threshold, planted faults fail it), the flag, the
refusals of run_survival_predictive, survival_predictive on a stub engine against hand-computed values, the header."""
import argparse
import contextlib
import io
import os
import re
import types
from functools import partial

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.preprocessing.synthetic import make_survival_variant_screen

import dm_reference as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["run", "survival", "variant", "screen.h5ad"]
T3 = (0.0, 7.0, 14.0)
T11 = tuple(float(t) for t in range(0, 22, 2))
# the configurations of the GPU file's law test, and the p-values each gives: timepoints x 2 likelihoods
LAW = [
    ("Normal", dict(), dict(), 12),
    ("MixtureNormal", dict(), dict(), 12),
    ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True), dict(), 12),
    ("MixtureNormal", dict(), dict(times=T3), 6),
    ("MixtureNormal", dict(), dict(times=T11), 22),
]
N_P = sum(c[3] for c in LAW)
P_MIN = 1e-3 / N_P
DRAWS = 64


# ---------------------------------------------------------------- host power
def _oracle_case(family, kw, gen_kw):
    """Totals (R, G) of both likelihoods, the concentrations (2, R, B, G) the oracle's dirmult_concentration forms inside
    oracle.survival.LOSSES[family] at parameters moved by 0.3 randn, and the sample mask."""
    from oracle import elbo
    from oracle import survival as osurv

    data = make_survival_variant_screen(128, 2, seed=21, mask_fraction=0.05, depth_per_guide=100.0,
                                        with_accessibility=bool(kw.get("scale_by_accessibility")), **gen_kw)
    torch.manual_seed(5)
    params = osurv.init_params(family, data, scale_by_acc=bool(kw.get("scale_by_accessibility")))
    params = {k: (v.detach() + 0.3 * torch.randn_like(v)).double() for k, v in params.items()}
    seen = []
    real = elbo.dirmult_concentration

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(out.detach().permute(0, 2, 1).clone())
        return out

    elbo.dirmult_concentration = spy
    try:
        osurv.LOSSES[family](elbo.as_float64(data), params, **kw)
    finally:
        elbo.dirmult_concentration = real
    assert len(seen) == 2
    n = [getattr(data, k).double().sum(1).numpy().astype(np.int64) for k in ("X_masked", "X_bcmatch_masked")]
    return n, torch.stack(seen).numpy(), data.sample_mask.numpy() != 0


def _smallest_p(n, alpha2, keep, fault, seed=3):
    rng = np.random.default_rng(seed)
    _, R, B, G = alpha2.shape
    flat = lambda a: np.moveaxis(a, 1, 2).reshape(R * G, B)  # noqa: E731
    back = lambda a: np.moveaxis(a.reshape(DRAWS, R, G, B), 3, 2)  # noqa: E731
    ps = []
    for i in range(2):
        x = back(dm.host_dm(n[i].reshape(-1), flat(alpha2[i]), DRAWS, rng, fault))
        assert (x.sum(2) == n[i][None]).all()
        ps += [p for _, p in dm.pit_marginals(x, n[i], alpha2[i], rng, keep=keep)]
    return min(ps), len(ps)


@pytest.mark.parametrize("family,kw,gen_kw,n_p", LAW,
                         ids=["Normal", "MixtureNormal", "MixtureNormal+Acc", "3-timepoints", "11-timepoints"])
def test_law_check_passes_the_host_sampler_and_sees_planted_faults(family, kw, gen_kw, n_p):
    assert N_P == 64
    n, alpha2, keep = _oracle_case(family, kw, gen_kw)
    B = alpha2.shape[2]
    assert 50 * B < np.median(n[0]) < 150 * B and not keep.all()  # depth 100 per guide and timepoint
    p, count = _smallest_p(n, alpha2, keep, None)
    print(f"{family} {kw} {gen_kw}: correct sampler, smallest of {count} p-values {p:.3e} (threshold {P_MIN:.3e})")
    assert count == n_p and p > P_MIN
    faults = ["conc_x1.25", "shift", "no_dirichlet"] + (["last_pair"] if alpha2.shape[2] % 2 else [])
    for fault in faults:
        p, _ = _smallest_p(n, alpha2, keep, fault)
        print(f"    fault {fault}: smallest p {p:.3e}")
        assert p <= P_MIN, (fault, p)


# ---------------------------------------------------------------- the flag
def test_flag_default_and_values():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser
    from bean_amd.model.parser import parse_args

    parser = get_parser()
    args = parser.parse_args(RUN)
    assert args.survival_predictive == 0 and args.predictive_seed == 101
    assert cli_run.survival_predictive_draws(args) == 0 and cli_run.survival_predictive_draws(argparse.Namespace()) == 0
    args = parser.parse_args(RUN + ["--survival-predictive", "200", "--predictive-seed", "7"])
    assert args.survival_predictive == 200 and args.predictive_seed == 7 and cli_run.survival_predictive_draws(args) == 200
    for bad in ("-1", "many"):
        with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(io.StringIO()):
            parser.parse_args(RUN + ["--survival-predictive", bad])
        assert exc.value.code == 2
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    assert not hasattr(plain.parse_args(RUN[1:]), "survival_predictive")  # the reference's flag table stays as it is
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    assert "--survival-predictive" in help_text and "read-weighted mean time" in help_text


@pytest.mark.parametrize("selection,design,named", [("sorting", "variant", "sorting screens"),
                                                     ("sorting", "tiling", "tiling screens (MultiMixtureNormal)"),
                                                     ("survival", "tiling", "tiling screens (MultiMixtureNormal)")])
def test_sorting_and_tiling_screens_are_refused_at_the_parser(selection, design, named):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser, main

    argv = ["run", selection, design, "screen.h5ad", "--survival-predictive", "50"]
    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2
    msg = " ".join(err.getvalue().split())
    assert "--survival-predictive" in msg and named in msg and "is not available for" in msg
    with pytest.raises(ValueError, match=re.escape(named)):
        cli_run.survival_predictive_draws(get_parser().parse_args(argv))
    assert cli_run.survival_predictive_draws(get_parser().parse_args(argv[:-2])) == 0


def test_posterior_predictive_still_refuses_survival_screens():
    from bean_amd.cli.execute import main

    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(RUN + ["--posterior-predictive", "50"])
    assert exc.value.code == 2
    msg = " ".join(err.getvalue().split())
    assert "--posterior-predictive" in msg and "is not available for survival screens" in msg


def test_run_survival_predictive_names_the_family_it_refuses():
    import bean_amd.model.model as m
    import bean_amd.model.survival_model as sm
    from bean_amd.engine import PredictiveUnsupported
    from bean_amd.model.run import run_survival_predictive

    screen = lambda **kw: types.SimpleNamespace(**{"selection": "survival", "library_design": "variant", **kw})  # noqa: E731
    for model, guide, data, named in (
        (partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide), screen(selection="sorting"),
         "sorting screens (MixtureNormal)"),
        (partial(m.NormalModel), m.NormalGuide, screen(selection="sorting"), "sorting screens (Normal)"),
        (partial(sm.MultiMixtureNormalModel), partial(sm.MultiMixtureNormalGuide), screen(library_design="tiling"),
         "tiling screens (MultiMixtureNormal)"),
        (partial(sm.ControlNormalModel), partial(sm.ControlNormalGuide), screen(), "ControlNormal"),
    ):
        with pytest.raises(PredictiveUnsupported, match=re.escape(named)) as exc:
            run_survival_predictive(model, guide, data, {})
        assert "a survival predictive check is not available for" in str(exc.value)


def test_run_survival_predictive_refuses_several_ranks(monkeypatch):
    import torch.distributed as dist

    import bean_amd.model.survival_model as sm
    from bean_amd.engine import PredictiveUnsupported
    from bean_amd.model.run import run_survival_predictive

    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    data = types.SimpleNamespace(selection="survival", library_design="variant")
    with pytest.raises(PredictiveUnsupported, match=re.escape("guide-sharded fits over 2 ranks (MixtureNormal)")):
        run_survival_predictive(partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide), data, {})


# ---------------------------------------------------------------- survival_predictive on a stub engine
class _Stub:
    """What survival_predictive reads of an engine, on host tensors; simulate_survival hands out planted counts."""
    family, survival, use_bcmatch = "MixtureNormal", True, False
    survival_predictive_supported = True

    def __init__(self, x_obs, draws, times):
        R, B, G = x_obs.shape
        self.data = types.SimpleNamespace(repguide_mask=torch.ones(R, G, dtype=torch.bool),
                                          sample_mask=torch.ones(R, B, dtype=torch.int64))
        self._keep = {"X": x_obs, "TIMEPOINTS": torch.tensor(times, dtype=torch.float64)}
        self._shape = types.SimpleNamespace(mask_thres=10)
        self.draws, self.calls = draws, []

    def simulate_survival(self, draw, seed=101, alphas=False):
        self.calls.append((draw, seed))
        return {"X": self.draws[draw]}


def test_survival_predictive_reproduces_hand_computed_values():
    from bean_amd.engine import PredictiveUnsupported
    from bean_amd.model.predictive import survival_predictive

    f = lambda *cols: torch.tensor(cols, dtype=torch.float32).T.reshape(1, 3, len(cols))  # noqa: E731  columns are guides
    obs = f((10, 10, 20), (40, 0, 0))
    draws = [f((20, 10, 10), (10, 10, 20)), f((10, 10, 20), (20, 10, 10)), f((0, 0, 40), (30, 10, 0))]
    eng = _Stub(obs, draws, (0.0, 0.5, 1.0))
    out = survival_predictive(eng, n_draws=3, seed=9)
    assert eng.calls == [(0, 9), (1, 9), (2, 9)] and out["n_draws"] == 3
    # T_rg = sum_b t_b x_b / n with t = (0, 0.5, 1): guide 0 holds (5 + 20) / 40, guide 1 no read after t = 0
    assert out["T_obs"].tolist() == [0.625, 0.0]
    # guide 0: the draws' T are 0.375, 0.625, 1.0 - two >= 0.625, two <= 0.625: p = min(1, 2 * 3 / 4) = 1
    # guide 1: 0.625, 0.375, 0.125 - three >= 0, none <= 0: p = 2 * 1 / 4
    assert out["ppc_p_score"].tolist() == [1.0, 0.5]
    t0, t1 = np.array([0.375, 0.625, 1.0]), np.array([0.625, 0.375, 0.125])
    want_z = [(0.625 - t0.mean()) / t0.std(ddof=1), (0.0 - t1.mean()) / t1.std(ddof=1)]
    np.testing.assert_allclose(out["ppc_z_score"].numpy(), want_z, rtol=1e-12)
    assert want_z[0] < 0 and want_z[1] < 0
    assert bool(torch.isnan(out["ppc_p_spread"]).all())  # one replicate: no spread between replicates
    # cells: with three draws no p-value is below 2 / 4, so no sample has a cell at p <= 0.05
    assert out["frac_cells_p05"].tolist() == [[0.0, 0.0, 0.0]]
    stack = torch.stack(draws).double()
    z = (obs.double() - stack.mean(0)) / stack.std(0, unbiased=True)
    # (timepoint 1 of guide 1 is 10 in every draw: sd 0, no z, and the sample's mean is guide 0's alone)
    assert float(stack[:, 0, 1, 1].std()) == 0
    want_mean_z = [float(z[0, 0].mean()), float(z[0, 1, 0]), float(z[0, 2].mean())]
    np.testing.assert_allclose(out["mean_z"].numpy().reshape(-1), want_mean_z, rtol=1e-12)
    with pytest.raises(ValueError, match="n_draws must be >= 1"):
        survival_predictive(eng, n_draws=0)
    eng.survival_predictive_supported = False
    with pytest.raises(PredictiveUnsupported, match="MixtureNormal, survival"):
        survival_predictive(eng, n_draws=3)


# ---------------------------------------------------------------- the header
def test_the_two_entry_points_are_declared():
    from bean_amd import _lib

    header = " ".join(open(os.path.join(ROOT, "include", "bean_hip.h")).read().split())
    assert "int bean_hip_survival_predictive_supported(const bean_hip_ctx* ctx);" in header
    assert ("int bean_hip_simulate_survival(bean_hip_ctx* ctx, uint64_t seed, uint64_t draw, void* x_out, uint64_t "
            "x_bytes, void* xbc_out, uint64_t xbc_bytes, void* alpha_out, uint64_t alpha_bytes, void* stream);") in header
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert len(bound["bean_hip_survival_predictive_supported"]) == 1
    assert bound["bean_hip_simulate_survival"] == bound["bean_hip_simulate"]
