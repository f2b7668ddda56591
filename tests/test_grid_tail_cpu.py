"""The tail rule of the grid posterior, the parts that need no GPU: the two C entry points'
declarations, the flag with its refusals, the table writer, grid_summary's tail_err, and grid_posterior over the CPU rule
(tail_reference.py behind tail_common.TailRuleEngine) on a screen with unedited guides against its exact posterior."""
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
from bean_amd.model.grid_posterior import GRID_KEYS, TAIL_BOUND, TAIL_KEYS, grid_posterior, grid_summary

import grid_common as gc
import importance_common as ic
import marginal_reference as mr
import tail_common as tc
import tail_reference as tr
from oracle import elbo
from test_grid_posterior_cpu import _gaussian_case, _grid_summary_of, _writer_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["run", "sorting", "variant", "screen.h5ad"]
EXACT_TARGETS = (3, 5)


# ---------------------------------------------------------------- the C entry points
def test_entry_points_declared_listed_and_exported_by_every_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    names = ("bean_hip_marginal_grid_tail", "bean_hip_marginal_tail_nodes")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
        assert name in {s[0] for s in _lib.SYMBOLS} and name in _lib.ENSEMBLE_SYMBOLS
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build in _lib.ALL_BUILDS:
        lib = ctypes.CDLL(_lib.build_library(amax=build))
        for name in names:
            assert hasattr(lib, name), (_lib.tree_path(build), name)
    lib = _lib.load()
    assert lib.bean_hip_marginal_grid_tail(None, 32, 1, 1, None, None, None, None, None, 0, None, 0, None, 0, None, 0,
                                           None) < 0
    assert lib.bean_hip_last_error().decode() == "bean_hip_marginal_grid_tail: null handle"
    assert lib.bean_hip_marginal_tail_nodes(None, 0, None, None, None, None, None, None) < 0
    assert lib.bean_hip_last_error().decode() == "bean_hip_marginal_tail_nodes: null handle"
    assert _lib.TAIL_NODES == tr.TAIL_NODES + tr.TAIL_CHECK_NODES == 112


# ---------------------------------------------------------------- the flag
def test_flag_default_parsing_and_help():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    parser = get_parser()
    assert parser.parse_args(RUN).grid_tail_rule is False and cli_run.grid_tail_rule(parser.parse_args(RUN)) is False
    assert cli_run.grid_tail_rule(parser.parse_args(RUN + ["--grid-posterior"])) is False
    assert cli_run.grid_tail_rule(parser.parse_args(RUN + ["--grid-posterior", "--grid-tail-rule"])) is True
    with pytest.raises(ValueError, match="--grid-posterior"):
        cli_run.grid_tail_rule(parser.parse_args(RUN + ["--grid-tail-rule"]))
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    for word in ("--grid-tail-rule", "Gauss-Jacobi", "n_pairs_tail", "grid_tail_err", "1e-3 nat per pair",
                 "prior-data conflict", "Refused without --grid-posterior"):
        assert word in help_text, word


@pytest.mark.parametrize("argv,words", [
    (RUN + ["--grid-tail-rule"], ("--grid-tail-rule", "--grid-posterior", "needs that flag")),
    (RUN + ["--grid-posterior", "--grid-tail-rule", "--scale-by-acc"], ("--grid-posterior", "--scale-by-acc")),
    (["run", "sorting", "tiling", "screen.h5ad", "--grid-posterior", "--grid-tail-rule"],
     ("--grid-posterior", "tiling screens (MultiMixtureNormal)")),
    (["run", "survival", "variant", "screen.h5ad", "--grid-posterior", "--grid-tail-rule"],
     ("--grid-posterior", "survival screens")),
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


# ---------------------------------------------------------------- the table
def test_table_writer_puts_the_two_columns_behind_the_grid_columns(tmp_path):
    from bean_amd.model import readwrite

    written = {}
    for what in ("grid", "tail"):
        target, guide, P, neg, kw = _writer_case()
        T = len(target)
        grid = _grid_summary_of(T)
        if what == "tail":
            g = torch.Generator().manual_seed(9)
            grid["n_pairs_tail"] = grid["n_pairs_unresolved"].clone()
            grid["grid_tail_err"] = torch.rand(T, generator=g, dtype=torch.float64) * 1e-6
        prefix = str(tmp_path / what) + "/"
        os.makedirs(prefix)
        with contextlib.redirect_stdout(io.StringIO()):
            readwrite.write_result_table(target, guide, P, "M", prefix=prefix, **{**kw, "grid": grid})
        written[what] = {n_: open(prefix + n_, "rb").read() for n_ in ("bean_element_result.M.csv", "bean_sgRNA_result.M.csv")}
    assert written["grid"]["bean_sgRNA_result.M.csv"] == written["tail"]["bean_sgRNA_result.M.csv"]
    read = lambda what: pd.read_csv(io.BytesIO(written[what]["bean_element_result.M.csv"]), index_col=0)  # noqa: E731
    plain, got = read("grid"), read("tail")
    assert [c for c in got.columns if c not in plain.columns] == list(TAIL_KEYS)
    cols = list(got.columns)
    at = cols.index("n_pairs_unresolved")
    assert cols[at - len(GRID_KEYS):at] == list(GRID_KEYS) and cols[at + 1:at + 3] == list(TAIL_KEYS)
    assert got.drop(columns=list(TAIL_KEYS)).equals(plain)
    assert got["n_pairs_tail"].dtype == np.int64 and got["n_pairs_tail"].tolist() == got["n_pairs_unresolved"].tolist()
    assert got["grid_tail_err"].dtype == np.float64 and bool(got["grid_tail_err"].notna().all())


# ---------------------------------------------------------------- grid_summary
def test_grid_summary_reports_the_tail_err_where_the_density_is():
    c = _gaussian_case()
    lj = c["lj_of"](c["m"])
    base = grid_summary(lj, *c["grid"])
    assert "grid_tail_err" not in base
    err = torch.zeros_like(lj)
    err[24, 24, :] = torch.tensor([1e-5, 2e-5, 3e-5, 4e-5, 5e-5], dtype=torch.float64)  # the middle node: at the peak
    err[0, 0, :] = 7.0                                                                   # a corner: no density there
    dens = (lj - lj.reshape(-1, 5).max(0).values).exp()
    assert bool((dens[0, 0] < 1e-6).all()) and bool((dens[24, 24] > 0.5).all())
    got = grid_summary(lj, *c["grid"], tail_err=err)
    assert got["grid_tail_err"].tolist() == [1e-5, 2e-5, 3e-5, 4e-5, 5e-5]
    for k in base:
        assert torch.equal(got[k], base[k]), k
    # the bar is the border's: a node at 1e-6 of the peak counts, one below does not
    line = torch.tensor([0.0, math.log(1e-6) + 1e-9, math.log(1e-6) - 1e-9], dtype=torch.float64).reshape(3, 1, 1)
    e = torch.tensor([1.0, 2.0, 4.0], dtype=torch.float64).reshape(3, 1, 1)
    one = [torch.zeros(1, dtype=torch.float64)] * 2 + [torch.ones(1, dtype=torch.float64)] * 2
    assert float(grid_summary(line, *one, tail_err=e)["grid_tail_err"]) == 2.0
    with pytest.raises(ValueError, match="tail_err has shape"):
        grid_summary(lj, *c["grid"], tail_err=err[:, :, :4])


# ---------------------------------------------------------------- grid_posterior over the CPU rule
@pytest.fixture(scope="module")
def unedited():
    return tc.claim_screen_with_unedited_guides()


@pytest.fixture(scope="module")
def cpu_run(unedited):
    data, alpha = unedited
    eng = tc.TailRuleEngine(data, alpha, range(data.n_targets))
    return eng, grid_posterior(eng, tail_rule=True)


def test_every_target_with_an_unedited_guide_gets_numbers_with_the_rule_and_none_without(unedited, cpu_run):
    data, alpha = unedited
    eng, res = cpu_run
    T = data.n_targets
    assert all(c[3] for c in eng.calls) and len(eng.calls) == 12  # every pass, the zooms and the null line included
    assert bool((res["n_pairs_tail"] > 0).all()) and torch.equal(res["n_pairs_tail"], res["n_pairs_unresolved"])
    print(f"grid_tail_err {[f'{v:.1e}' for v in res['grid_tail_err'].tolist()]}; null line "
          f"{[f'{v:.1e}' for v in res['grid_null_tail_err'].tolist()]}; tail pairs {res['n_pairs_tail'].tolist()}")
    assert bool(res["grid_ok"].all()) and bool(res["grid_tail_ok"].all()) and bool(res["grid_null_ok"].all())
    assert bool((res["grid_tail_err"] <= TAIL_BOUND * res["n_pairs_tail"]).all())
    for k in GRID_KEYS[:-1]:
        assert bool(torch.isfinite(res[k]).all()), k
    # without the rule: a cheap pass is enough, the NaN rule does not depend on the grid
    eng0 = tc.TailRuleEngine(data, alpha, range(T))
    plain = grid_posterior(eng0, nodes=16, zoom_nodes=16, n_zoom=1, n_z=5, n_mu=5, n_y=3)
    assert not any(c[3] for c in eng0.calls) and "grid_tail_err" not in plain and "n_pairs_tail" not in plain
    assert not bool(plain["grid_ok"].any())
    for k in GRID_KEYS[:-1]:
        assert bool(torch.isnan(plain[k]).all()), k


@pytest.mark.parametrize("t", EXACT_TARGETS)
def test_moments_meet_the_exact_posterior(unedited, cpu_run, t):
    """mu_grid and mu_sd_grid against exact_marginal_moments with the 128-node Jacobi rule inside for the tail pairs,
    under section 22's bound: the two quadratures' step-doubling moves plus 1e-9 (grid_common.assert_meets_exact).
    Measured: DESIGN.md section 23."""
    data, alpha = unedited
    _, res = cpu_run
    c_p = mr.model_conc(data, {"alpha_pi": alpha})
    idx = ic.target_guides(data, t)
    ex = tr.exact_marginal_moments(elbo.as_float64(data[idx]), c_p[idx])
    gc.assert_meets_exact(res, t, ex, f"CPU rule, tail rule, target {t}")


def test_a_planted_conflict_pair_turns_its_target_nan_and_keeps_the_diagnostic(unedited):
    """The conflict row of tests/test_tail_reference.py - c_p = (0.08, 40), control counts (0, 300), on the pairs of the
    screen's first target at (mu, sd) = (2, 1.3) - gives |J64 - J48| of tens of nats.  That figure, from the rule itself,
    (the largest over the pairs) is served as the tail_err of one pair of target 7 at every node: the target is NaN, grid_tail_err is reported and is
    that figure; target 5 beside it keeps its numbers.  (The conflict is planted in what the engine serves and not in
    the screen: planted in the data of one guide of five - exponents (0.08, 80) against sorting reads moved into the
    top bin, at three read depths - it did not reach the nodes that hold the posterior, because the posterior of mu
    moves to where that guide is consistent, and grid_tail_err stayed at 1e-11.)"""
    data, alpha = unedited
    first = elbo.as_float64(data[ic.target_guides(data, 0)])
    c_p = torch.tensor([0.08, 40.0], dtype=torch.float64).expand(first.n_guides, 2).clone()
    ctrl = torch.zeros_like(first.allele_counts_control.double())
    ctrl[:, 0, :, 1] = 300.0
    h = mr.PairIntegrand(first, torch.tensor([2.0]), torch.tensor([1.3]), c_p, ctrl=ctrl)
    a_prime = mr.beta_exponents(first, c_p, ctrl)
    planted = float((tr.jacobi_rule(h, a_prime, tr.TAIL_NODES) - tr.jacobi_rule(h, a_prime, tr.TAIL_CHECK_NODES)).abs().max())
    assert planted > 1.0

    class Served(tc.TailRuleEngine):
        def marginal_grid(self, *a, **kw):
            out = super().marginal_grid(*a, **kw)
            if kw.get("tail_rule"):
                out["tail_err"][:, :, 1] += planted
            return out

    eng = Served(data, alpha, (5, 7))
    res = grid_posterior(eng, tail_rule=True)
    print(f"conflict: |J64 - J48| planted {planted:.3g}; grid_tail_err {res['grid_tail_err'].tolist()} against "
          f"{(TAIL_BOUND * res['n_pairs_tail']).tolist()}; grid_ok {res['grid_ok'].tolist()}")
    assert res["grid_ok"].tolist() == [True, False] and res["grid_tail_ok"].tolist() == [True, False]
    assert bool(res["grid_resolved"].all()) and res["grid_null_ok"].tolist() == [True, False]
    for k in GRID_KEYS[:-1]:
        assert math.isfinite(float(res[k][0])) and math.isnan(float(res[k][1])), k
    assert abs(float(res["grid_tail_err"][1]) - planted) < 1e-9 and float(res["n_pairs_tail"][1]) > 0
    for k in ("grid_border", "grid_step_shift", "mu_grid_coarse"):
        assert math.isfinite(float(res[k][1])), k
