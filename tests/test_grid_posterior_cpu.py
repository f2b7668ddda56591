"""The grid posterior of (mu, sd) per target, the parts that need no GPU: grid_summary on an
analytic density, grid_posterior over the CPU rule against the exact moments of section 21's claim test, the Bayes factor's
null line, the NaN rule, the C entry point's declaration, the two flags with their refusals, and the table writer."""
import contextlib
import ctypes
import io
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.grid_posterior import GRID_KEYS, grid_posterior, grid_summary

import grid_common as gc
import importance_common as ic
import marginal_reference as mr
from oracle import elbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "golden")
RUN = ["run", "sorting", "variant", "screen.h5ad"]
CPU_TARGETS = (0, 3, 5, 7)  # target 0 carries an effect (mean -1.12), the others are null: the prior's kink is in the grid


# ---------------------------------------------------------------- grid_summary on a density with closed forms
def _gaussian_case():
    """Five targets, each an axis-aligned Gaussian in (mu, y) times its own constant, on its own 49 x 49 grid of step
    0.325 sd (+- 7.8 sd: beyond it lies 6e-15 of the mass and 2e-13 of the variance); centres off the means."""
    m = torch.tensor([-1.12, 0.03, 0.0, 0.4, 2.0], dtype=torch.float64)
    s = torch.tensor([0.05, 0.07, 0.2, 1.0, 0.3], dtype=torch.float64)
    ym = torch.tensor([0.03, -0.2, 0.0, 0.5, 0.1], dtype=torch.float64)
    ys = torch.tensor([0.01, 0.02, 0.05, 0.1, 0.03], dtype=torch.float64)
    logz = torch.tensor([-1234.5, 10.0, 0.0, -3.0, 77.0], dtype=torch.float64)
    n = 49
    c_mu, c_y = m + torch.tensor([0.1, -0.2, 0.0, 0.15, -0.05]) * s, ym + torch.tensor([-0.1, 0.2, 0.05, 0.0, 0.1]) * ys
    s_mu, s_y = 0.325 * s, 0.325 * ys

    def lj_of(m_):
        i = torch.arange(n, dtype=torch.float64) - (n - 1) / 2.0
        MU = (c_mu[None] + i[:, None] * s_mu[None])[:, None, :]
        Y = (c_y[None] + i[:, None] * s_y[None])[None, :, :]
        return (logz - 0.5 * ((MU - m_) / s) ** 2 - 0.5 * ((Y - ym) / ys) ** 2 - (s * ys).log() - math.log(2.0 * math.pi))

    return dict(m=m, s=s, ym=ym, ys=ys, logz=logz, grid=(c_mu, c_y, s_mu, s_y), lj_of=lj_of)


def test_grid_summary_meets_the_closed_forms_of_a_gaussian():
    c = _gaussian_case()
    got = grid_summary(c["lj_of"](c["m"]), *c["grid"])
    want = {"mu_grid": c["m"], "mu_sd_grid": c["s"], "log_evidence_grid": c["logz"],
            "p_mu_pos_grid": 0.5 * torch.erfc(-c["m"] / c["s"] / math.sqrt(2.0)),
            "sd_grid": (c["ym"] + 0.5 * c["ys"] ** 2).exp()}
    for k, w in want.items():
        d = (got[k] - w).abs()
        print(f"{k}: largest |diff| {float(d.max()):.2e}")
        assert bool((d <= 1e-10).all()), (k, got[k], w)
    assert bool(got["grid_ok"].all()) and bool((got["grid_border"] < 1e-12).all())
    assert bool((got["grid_step_shift"] < 1e-10).all())
    # a target with half its mass left of 0 and a node at 0: the indicator counts that node half
    assert float(got["p_mu_pos_grid"][2]) == pytest.approx(0.5, abs=1e-12)


def test_mass_on_the_border_turns_that_target_not_ok_and_no_other():
    c = _gaussian_case()
    base = grid_summary(c["lj_of"](c["m"]), *c["grid"])
    moved = c["m"].clone()
    moved[1] = c["grid"][0][1] + 24 * c["grid"][2][1]  # the last grid line of mu
    got = grid_summary(c["lj_of"](moved), *c["grid"])
    assert got["grid_ok"].tolist() == [True, False, True, True, True]
    assert float(got["grid_border"][1]) > 0.5
    others = torch.tensor([True, False, True, True, True])
    for k in base:
        assert torch.equal(got[k][others], base[k][others]), k  # nothing of a target is read from another's lj
    with pytest.raises(ValueError, match="n_mu, n_y, T"):
        grid_summary(torch.zeros(3, 4), *c["grid"])
    with pytest.raises(ValueError, match="for 5 targets"):
        grid_summary(c["lj_of"](c["m"]), c["grid"][0][:4], *c["grid"][1:])


def test_one_node_of_mu_is_a_line_integral():
    c = _gaussian_case()
    c_mu, c_y, s_mu, s_y = c["grid"]
    lj = c["lj_of"](c["m"])[24:25]  # the middle line of mu: mu = c_mu
    got = grid_summary(lj, c_mu, c_y, torch.ones(5, dtype=torch.float64), s_y)
    want = c["logz"] - 0.5 * ((c_mu - c["m"]) / c["s"]) ** 2 - c["s"].log() - 0.5 * math.log(2.0 * math.pi)
    assert bool(((got["log_evidence_grid"] - want).abs() <= 1e-10).all())
    assert bool((got["mu_sd_grid"] == 0).all()) and bool((got["grid_border"] < 1e-12).all())


# ---------------------------------------------------------------- grid_posterior over the CPU rule
@pytest.fixture(scope="module")
def cpu_run():
    data = ic.claim_screen()
    eng = gc.RuleEngine(data, CPU_TARGETS)
    return data, eng, grid_posterior(eng)


def test_grid_posterior_reaches_the_exact_moments_from_the_start_zero(cpu_run):
    """The claim screen (40 x 3, seed 3), targets 0, 3, 5, 7, the engine serving marginal_log_joint from the start
    (mu, y) = (0, 0) with grid_posterior's defaults: five zoom passes of 17 x 17 (16 quadrature nodes) and the 41 x 21
    grid (32; exact_marginal_moments has 64 inside, and the two agree to every digit printed).
    Measured: see DESIGN.md section 22."""
    data, eng, res = cpu_run
    assert eng.calls[:5] == [(17, 17, 16)] * 5 and eng.calls[5] == (41, 21, 32)
    assert eng.calls[6:11] == [(1, 17, 16)] * 5 and eng.calls[11:] == [(1, 21, 32)]
    for j, t in enumerate(CPU_TARGETS):
        gc.assert_meets_exact(res, j, mr.claim_exact(data, t), f"CPU rule, target {t}")
    assert float(res["mu_grid"][0]) < -1.0 and float(res["p_mu_pos_grid"][0]) < 1e-6  # the effect target
    assert float(res["log_bf10_grid"][0]) > 10.0
    assert bool((res["sd_grid"] > 0.9).all()) and bool((res["sd_grid"] < 1.2).all())


def test_null_line_evidence_is_the_dense_integral(cpu_run):
    """log int p(x | mu = 0, y) p(y) dy of the null line against composite Simpson on 2001 points of
    marginal_log_joint(mu = 0, y) over the line's own interval, less log p(mu = 0) = - log 2: within the line's
    step-doubling move."""
    data, eng, res = cpu_run
    n = 2001
    for j, t in enumerate(CPU_TARGETS):
        assert bool(res["grid_null_ok"][j])
        c, s = float(res["grid_null_centre_y"][j]), float(res["grid_null_step_y"][j])
        ys = torch.linspace(c - 10 * s, c + 10 * s, n, dtype=torch.float64)
        sub, cp = eng.subs[j]
        lj = mr.marginal_log_joint(sub, cp, torch.zeros_like(ys), ys, Q=32)
        w = torch.where(torch.arange(n) % 2 == 1, 4.0, 2.0).double()
        w[0] = w[-1] = 1.0
        want = float(torch.logsumexp(lj + w.log(), 0)) + math.log(float(ys[1] - ys[0]) / 3.0) + math.log(2.0)
        got, move = float(res["log_evidence_null_grid"][j]), float(res["log_evidence_null_step_move"][j])
        print(f"target {t}: null evidence {got:.10f} dense {want:.10f} |diff| {abs(got - want):.2e} step-doubling move "
              f"{move:.2e}; log_bf10_grid {float(res['log_bf10_grid'][j]):.4f}")
        assert move < 1e-3 and abs(got - want) <= move, (t, got, want, move)
        assert float(res["log_bf10_grid"][j]) == float(res["log_evidence_grid"][j]) - got


def test_bayes_factor_takes_the_normal_prior_of_prior_params():
    """grid_posterior over an engine with --prior-params priors: the null line's evidence against composite Simpson of the
    served log joint at mu = 0 less log Normal(0; mu_loc, mu_scale) from torch.distributions - the host-side prior of
    the Bayes factor is the one the log joint was formed with.  One value per prior is taken for every target; any
    other length is refused."""
    import torch.distributions as tdist

    from bean_amd.model.grid_posterior import log_prior_mu_at_zero

    data = ic.claim_screen()
    prior = {"mu_loc": torch.tensor([0.3, -0.2]), "mu_scale": torch.tensor([0.5, 2.0]),
             "sd_loc": torch.tensor([0.02, -0.01]), "sd_scale": torch.tensor([0.05, 0.08])}
    eng = gc.RuleEngine(data, (3, 5), prior_params=prior)
    res = grid_posterior(eng, nodes=16, zoom_nodes=16)
    assert res["grid_ok"].tolist() == [True, True] and bool(res["grid_null_ok"].all())
    n = 2001
    for j in range(2):
        c, s = float(res["grid_null_centre_y"][j]), float(res["grid_null_step_y"][j])
        ys = torch.linspace(c - 10 * s, c + 10 * s, n, dtype=torch.float64)
        sub, cp = eng.subs[j]
        d_mu, d_sd = elbo._priors((n,), 0.01, None)
        p_sd = tdist.LogNormal(prior["sd_loc"][j].double(), prior["sd_scale"][j].double())
        lik_and_sd = (mr.marginal_log_joint(sub, cp, torch.zeros_like(ys), ys, Q=16) - d_mu.log_prob(torch.zeros_like(ys))
                      - d_sd.log_prob(ys.exp()) + p_sd.log_prob(ys.exp()))
        w = torch.where(torch.arange(n) % 2 == 1, 4.0, 2.0).double()
        w[0] = w[-1] = 1.0
        want = float(torch.logsumexp(lik_and_sd + w.log(), 0)) + math.log(float(ys[1] - ys[0]) / 3.0)
        got, move = float(res["log_evidence_null_grid"][j]), float(res["log_evidence_null_step_move"][j])
        print(f"prior-params target {(3, 5)[j]}: null evidence {got:.10f} dense {want:.10f} |diff| {abs(got - want):.2e} "
              f"move {move:.2e}; log_bf10_grid {float(res['log_bf10_grid'][j]):.4f}")
        assert move < 1e-3 and abs(got - want) <= move, (j, got, want, move)
    like = torch.zeros(2, dtype=torch.float64)
    want0 = tdist.Normal(prior["mu_loc"].double(), prior["mu_scale"].double()).log_prob(like)
    assert bool(((log_prior_mu_at_zero(eng, like) - want0).abs() < 1e-14).all())
    eng.prior_params = {"mu_scale": torch.tensor(2.0)}  # one value, mu_loc left at 0
    assert bool(((log_prior_mu_at_zero(eng, like) - tdist.Normal(like, 2.0 + like).log_prob(like)).abs() < 1e-14).all())
    eng.prior_params = {"sd_loc": prior["sd_loc"]}  # no Normal prior on mu: Laplace(0, 1)
    assert log_prior_mu_at_zero(eng, like).tolist() == [-math.log(2.0)] * 2
    eng.prior_params = {"mu_loc": torch.zeros(3)}
    with pytest.raises(ValueError, match="3 entries for 2 targets"):
        log_prior_mu_at_zero(eng, like)


def test_nan_rule_fires_for_unresolved_pairs_and_keeps_the_diagnostics():
    data = ic.claim_screen()
    eng = gc.RuleEngine(data, (3, 5), n_unresolved=torch.tensor([0, 2], dtype=torch.int32))
    res = grid_posterior(eng, nodes=16, zoom_nodes=16)
    assert res["grid_ok"].tolist() == [True, False] and res["n_pairs_unresolved"].tolist() == [0.0, 2.0]
    for k in GRID_KEYS[:-1]:
        assert math.isfinite(float(res[k][0])) and math.isnan(float(res[k][1])), k
    for k in ("grid_border", "grid_step_shift", "mu_grid_coarse"):
        assert math.isfinite(float(res[k][1])), k
    assert bool(res["grid_resolved"].all())


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    name = "bean_hip_marginal_grid"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in {s[0] for s in _lib.SYMBOLS} and name in _lib.ENSEMBLE_SYMBOLS
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), name), _lib.tree_path(build)
    lib = _lib.load()
    assert lib.bean_hip_marginal_grid(None, 32, 1, 1, None, None, None, None, None, 0, None, 0, None, 0, None) < 0
    assert "null handle" in lib.bean_hip_last_error().decode()


# ---------------------------------------------------------------- the flags
def test_flags_defaults_parsing_and_help():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    parser = get_parser()
    args = parser.parse_args(RUN)
    assert args.grid_posterior is False and args.grid_nodes == 32 and cli_run.grid_nodes(args) is None
    assert cli_run.grid_nodes(parser.parse_args(RUN + ["--grid-nodes", "64"])) is None
    assert cli_run.grid_nodes(parser.parse_args(RUN + ["--grid-posterior"])) == 32
    for q in (16, 32, 64):
        assert cli_run.grid_nodes(parser.parse_args(RUN + ["--grid-posterior", "--grid-nodes", str(q)])) == q
    with pytest.raises(ValueError, match="16, 32, 64"):
        cli_run.grid_nodes(parser.parse_args(RUN + ["--grid-posterior", "--grid-nodes", "20"]))
    with pytest.raises(ValueError, match="--scale-by-acc"):
        cli_run.grid_nodes(parser.parse_args(RUN + ["--grid-posterior", "--scale-by-acc"]))
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    for word in ("--grid-posterior", "--grid-nodes", "mu_grid", "mu_sd_grid", "sd_grid", "p_mu_pos_grid",
                 "log_evidence_grid", "log_bf10_grid", "grid_ok", "n_pairs_unresolved", "second mode"):
        assert word in help_text, word


@pytest.mark.parametrize("argv,words", [
    (RUN + ["--grid-posterior", "--grid-nodes", "20"], ("--grid-nodes", "16, 32, 64")),
    (RUN + ["--grid-nodes", "128"], ("--grid-nodes", "16, 32, 64")),
    (RUN + ["--grid-posterior", "--scale-by-acc"], ("--grid-posterior", "--scale-by-acc", "further latent per guide")),
    (["run", "sorting", "tiling", "screen.h5ad", "--grid-posterior"],
     ("--grid-posterior", "tiling screens (MultiMixtureNormal)")),
    (["run", "survival", "variant", "screen.h5ad", "--grid-posterior"], ("--grid-posterior", "survival screens")),
])
def test_refusals_at_the_parser(argv, words):
    from bean_amd.cli.execute import main

    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2
    msg = " ".join(err.getvalue().split())
    for w in words:
        assert w in msg, (w, msg)


def test_run_grid_posterior_refuses_what_only_the_model_shows():
    import types
    from functools import partial

    import bean_amd.model.model as m
    from bean_amd.engine import PredictiveUnsupported
    from bean_amd.model.run import run_grid_posterior

    data = types.SimpleNamespace(selection="sorting", library_design="variant")
    with pytest.raises(PredictiveUnsupported, match="ControlNormal"):
        run_grid_posterior(partial(m.ControlNormalModel), partial(m.ControlNormalGuide), data, {})
    with pytest.raises(PredictiveUnsupported, match="accessibility scaling .MixtureNormal.*further latent per guide"):
        run_grid_posterior(partial(m.MixtureNormalModel, scale_by_accessibility=True),
                           partial(m.MixtureNormalGuide, scale_by_accessibility=True), data, {})


# ---------------------------------------------------------------- the table
def _writer_case():
    src = open(os.path.join(HERE, "make_readwrite_golden.py")).read()
    ns = {}
    exec("import numpy as np, pandas as pd, torch\n" + src[src.index("CASES = {"):src.index("def main():")], ns)
    return ns["build"]("plain", 100)


def _grid_summary_of(T, seed=4):
    g = torch.Generator().manual_seed(seed)
    ok = torch.ones(T, dtype=torch.bool)
    ok[5] = False
    n = torch.zeros(T, dtype=torch.float64)
    n[3] = 2
    ok[3] = False
    out = {k: torch.randn(T, generator=g, dtype=torch.float64) for k in GRID_KEYS[:-1]}
    out = {k: torch.where(ok, v, torch.full_like(v, math.nan)) for k, v in out.items()}
    out.update({"grid_ok": ok, "n_pairs_unresolved": n, "grid_border": torch.zeros(T, dtype=torch.float64)})
    return out


def test_table_writer_puts_the_columns_behind_the_importance_columns(tmp_path):
    from bean_amd.model import readwrite
    from bean_amd.model.importance import MARGINAL_KEYS

    own = list(GRID_KEYS) + ["n_pairs_unresolved"]
    written = {}
    for what in ("plain", "grid", "importance", "both"):
        target, guide, P, neg, kw = _writer_case()
        T = len(target)
        extra = {}
        if what in ("importance", "both"):
            g = torch.Generator().manual_seed(4)
            imp = {k: torch.rand(T, generator=g, dtype=torch.float64) for k in ("psis_k", "mu_is", "mu_sd_is", "is_ess")}
            imp["n_is"] = torch.full((T,), 500.0, dtype=torch.float64)
            imp.update({k: torch.rand(T, generator=g, dtype=torch.float64) for k in MARGINAL_KEYS[:4]})
            imp["n_pairs_unresolved"] = torch.zeros(T, dtype=torch.float64)
            extra["importance"] = imp
        if what in ("grid", "both"):
            extra["grid"] = _grid_summary_of(T)
        prefix = str(tmp_path / what) + "/"
        os.makedirs(prefix)
        with contextlib.redirect_stdout(io.StringIO()):
            readwrite.write_result_table(target, guide, P, "M", prefix=prefix, **{**kw, **extra})
        written[what] = {n_: open(prefix + n_, "rb").read() for n_ in ("bean_element_result.M.csv", "bean_sgRNA_result.M.csv")}
    read = lambda what: pd.read_csv(io.BytesIO(written[what]["bean_element_result.M.csv"]), index_col=0)  # noqa: E731
    assert written["plain"]["bean_sgRNA_result.M.csv"] == written["both"]["bean_sgRNA_result.M.csv"]
    plain, got = read("plain"), read("grid")
    assert [c for c in got.columns if c not in plain.columns] == own
    assert got.drop(columns=own).equals(plain)
    assert got["grid_ok"].dtype == np.int64 and got["n_pairs_unresolved"].dtype == np.int64
    out = (got["grid_ok"] == 0) | (got["n_pairs_unresolved"] > 0)
    assert int(out.sum()) == 2
    for k in GRID_KEYS[:-1]:
        assert got[k][out].isna().all() and got[k][~out].notna().all(), k
    # behind the importance columns; n_pairs_unresolved once, where the marginal check has written it
    imp, both = read("importance"), read("both")
    assert [c for c in both.columns if c not in imp.columns] == list(GRID_KEYS)
    cols = list(both.columns)
    at = cols.index("n_pairs_unresolved")
    assert cols[at + 1:at + 1 + len(GRID_KEYS)] == list(GRID_KEYS) and cols.count("n_pairs_unresolved") == 1
    assert both.drop(columns=list(GRID_KEYS)).equals(imp)
