"""The tail rule of the marginal importance check, the parts that need no GPU: the C entry point's
declaration, marginal_summary's bar, the flag with its refusals, the table writer, the rule under accessibility - whose
clamp of the scaled share is a kink inside the mass of the rule's weight - against section 21's bound, and
importance_check over the CPU rule (tail_reference.py behind a fake engine) on a screen with unedited guides."""
import contextlib
import ctypes
import io
import json
import math
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.importance import (MARGINAL_KEYS, TAIL_BOUND, TAIL_KEYS, TAIL_WEIGHT_MIN, importance_check,
                                       importance_summary, marginal_summary)
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

import importance_common as ic
import marginal_reference as mr
import tail_common as tc
import tail_reference as tr
from oracle import elbo
from test_grid_posterior_cpu import _grid_summary_of, _writer_case
from test_marginal_reference import BOUND, _override
from test_tail_reference import SETTINGS, TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = ["run", "sorting", "variant", "screen.h5ad"]
MARG = ["--importance-check", "100", "--importance-integrate-pi"]


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    name = "bean_hip_log_weights_marginal_tail"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in {s[0] for s in _lib.SYMBOLS} and name in _lib.ENSEMBLE_SYMBOLS
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), name), _lib.tree_path(build)
    lib = _lib.load()
    assert lib.bean_hip_log_weights_marginal_tail(None, 101, 0, 1, 32, None, 0, None, 0, None, 0, None, 0, None, 0, None,
                                                  0, None) < 0
    assert lib.bean_hip_last_error().decode() == name + ": null handle"


# ---------------------------------------------------------------- marginal_summary's bar
def _weights(S=200, T=4, seed=2):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(S, T, generator=g, dtype=torch.float64), torch.randn(S, T, generator=g, dtype=torch.float64))


def test_bar_passes_at_the_bound_and_refuses_above_it():
    """Targets with 0, 2, 2 and 3 tail pairs; is_tail_err 0, exactly 2e-3, just above 2e-3, 1e-4: numbers, numbers, NaN,
    numbers - and both diagnostics on every one."""
    assert TAIL_BOUND == tr.TAIL_BOUND == BOUND == 1e-3 and TAIL_WEIGHT_MIN == 1e-6
    logw, mu = _weights()
    n = torch.tensor([0, 2, 2, 3], dtype=torch.int32)
    te = torch.zeros_like(logw)
    top = logw.argmax(0)
    te[top[1], 1] = 2.0 * TAIL_BOUND
    te[top[2], 2] = math.nextafter(2.0 * TAIL_BOUND, 1.0)
    te[:, 3] = 1e-4
    plain = marginal_summary(logw, mu, n)
    got = marginal_summary(logw, mu, n, tail_err=te)
    base = importance_summary(logw, mu)
    assert tuple(plain) == MARGINAL_KEYS and tuple(got) == MARGINAL_KEYS + TAIL_KEYS
    assert got["n_pairs_tail"].tolist() == [0.0, 2.0, 2.0, 3.0] and torch.equal(got["n_pairs_unresolved"], got["n_pairs_tail"])
    assert got["is_tail_err"].tolist() == [0.0, 2.0 * TAIL_BOUND, math.nextafter(2.0 * TAIL_BOUND, 1.0), 1e-4]
    for k in MARGINAL_KEYS[:4]:
        assert torch.isnan(plain[k]).tolist() == [False, True, True, True], k
        assert torch.isnan(got[k]).tolist() == [False, False, True, False], k
        assert torch.equal(got[k][[0, 1, 3]], base[k[:-5]][[0, 1, 3]]) and torch.equal(got[k][0], plain[k][0]), k
    # a NaN error refuses, and is kept
    te[5, 3] = math.nan
    bad = marginal_summary(logw, mu, n, tail_err=te)
    assert bool(torch.isnan(bad["psis_k_marg"][3])) and not bool(torch.isnan(bad["psis_k_marg"][1]))
    with pytest.raises(TypeError):
        marginal_summary(logw, mu, n, te)  # keyword only
    with pytest.raises(ValueError, match="tail_err has shape"):
        marginal_summary(logw, mu, n, tail_err=te[:-1])


def test_a_low_weight_draw_with_a_huge_tail_err_is_ignored():
    """The draws that count are those whose raw logw is within log 1e6 of the target's largest."""
    logw, mu = _weights(T=2)
    n = torch.tensor([1, 1], dtype=torch.int32)
    low = int(logw[:, 0].argmin())
    logw[low, 0] = logw[:, 0].max() + math.log(TAIL_WEIGHT_MIN) - 1e-9   # just outside
    logw[low, 1] = logw[:, 1].max() + math.log(TAIL_WEIGHT_MIN) + 1e-9   # just inside
    te = torch.full_like(logw, 1e-7)
    te[low] = 50.0
    got = marginal_summary(logw, mu, n, tail_err=te)
    assert got["is_tail_err"].tolist() == [1e-7, 50.0]
    assert bool(torch.isfinite(got["psis_k_marg"][0])) and bool(torch.isnan(got["psis_k_marg"][1]))
    for k in MARGINAL_KEYS[:4]:
        assert bool(torch.isnan(got[k][1])), k
    assert got["n_pairs_tail"].tolist() == [1.0, 1.0]


# ---------------------------------------------------------------- the flag
def test_flag_default_parsing_help_and_the_references_flag_table():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser
    from bean_amd.model import parser as run_parser

    parser = get_parser()
    assert parser.parse_args(RUN).importance_tail_rule is False
    assert cli_run.importance_tail_rule(parser.parse_args(RUN)) is False
    assert cli_run.importance_tail_rule(parser.parse_args(RUN + MARG)) is False
    assert cli_run.importance_tail_rule(parser.parse_args(RUN + MARG + ["--importance-tail-rule"])) is True
    with pytest.raises(ValueError, match="--importance-integrate-pi"):
        cli_run.importance_tail_rule(parser.parse_args(RUN + ["--importance-tail-rule"]))
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    for word in ("--importance-tail-rule", "Gauss-Jacobi", "n_pairs_tail", "is_tail_err", "1e-3 nat per pair",
                 "Refused without --importance-integrate-pi"):
        assert word in help_text, word
    # the reference's own flags are what they were: the new one is this project's
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "run_flags.json")))
    dests = [a.dest for a in run_parser.parse_args()._actions if a.dest != "help"]
    assert dests == [w["dest"] for w in want] and "importance_tail_rule" not in dests


@pytest.mark.parametrize("argv,words", [
    (RUN + ["--importance-tail-rule"], ("--importance-tail-rule", "--importance-integrate-pi", "needs that flag")),
    (RUN + ["--importance-check", "100", "--importance-tail-rule"], ("--importance-tail-rule", "needs that flag")),
    (RUN + ["--importance-integrate-pi", "--importance-tail-rule"], ("--importance-integrate-pi", "--importance-check")),
    (["run", "sorting", "tiling", "screen.h5ad"] + MARG + ["--importance-tail-rule"],
     ("--importance-check", "tiling screens (MultiMixtureNormal)")),
    (["run", "survival", "variant", "screen.h5ad"] + MARG + ["--importance-tail-rule"],
     ("--importance-check", "survival screens")),
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
def test_table_writer_puts_the_two_columns_behind_the_marginal_columns(tmp_path):
    from bean_amd.model import readwrite

    written = {}
    for what in ("marg", "tail", "tail+grid"):
        target, guide, P, neg, kw = _writer_case()
        T = len(target)
        g = torch.Generator().manual_seed(4)
        imp = {k: torch.rand(T, generator=g, dtype=torch.float64) for k in ("psis_k", "mu_is", "mu_sd_is", "is_ess")}
        imp["n_is"] = torch.full((T,), 500.0, dtype=torch.float64)
        imp.update({k: torch.rand(T, generator=g, dtype=torch.float64) for k in MARGINAL_KEYS[:4]})
        imp["n_pairs_unresolved"] = torch.zeros(T, dtype=torch.float64)
        imp["n_pairs_unresolved"][3] = 2
        extra = {"importance": imp}
        if what != "marg":
            imp["n_pairs_tail"] = imp["n_pairs_unresolved"].clone()
            imp["is_tail_err"] = torch.rand(T, generator=g, dtype=torch.float64) * 1e-6
        if what == "tail+grid":
            grid = _grid_summary_of(T)
            grid["n_pairs_tail"] = grid["n_pairs_unresolved"].clone()
            grid["grid_tail_err"] = torch.full((T,), 1e-9, dtype=torch.float64)
            extra["grid"] = grid
        prefix = str(tmp_path / what) + "/"
        os.makedirs(prefix)
        with contextlib.redirect_stdout(io.StringIO()):
            readwrite.write_result_table(target, guide, P, "M", prefix=prefix, **{**kw, **extra})
        written[what] = {n_: open(prefix + n_, "rb").read() for n_ in ("bean_element_result.M.csv", "bean_sgRNA_result.M.csv")}
    assert written["marg"]["bean_sgRNA_result.M.csv"] == written["tail"]["bean_sgRNA_result.M.csv"]
    read = lambda what: pd.read_csv(io.BytesIO(written[what]["bean_element_result.M.csv"]), index_col=0)  # noqa: E731
    plain, got, both = read("marg"), read("tail"), read("tail+grid")
    assert [c for c in got.columns if c not in plain.columns] == list(TAIL_KEYS)
    cols = list(got.columns)
    at = cols.index("n_pairs_unresolved")
    assert cols[at - 4:at] == list(MARGINAL_KEYS[:4]) and cols[at + 1:at + 3] == list(TAIL_KEYS)
    assert got.drop(columns=list(TAIL_KEYS)).equals(plain)
    assert got["n_pairs_tail"].dtype == np.int64 and got["n_pairs_tail"].tolist() == got["n_pairs_unresolved"].tolist()
    assert got["is_tail_err"].dtype == np.float64 and bool(got["is_tail_err"].notna().all())
    # n_pairs_tail once where --grid-tail-rule also writes it; grid_tail_err keeps its place behind the grid columns
    cols = list(both.columns)
    assert cols.count("n_pairs_tail") == 1 and cols.index("n_pairs_tail") == cols.index("n_pairs_unresolved") + 1
    assert cols.index("grid_tail_err") > cols.index("grid_ok") and both["n_pairs_tail"].tolist() == got["n_pairs_tail"].tolist()


# ---------------------------------------------------------------- the rule under accessibility
@pytest.fixture(scope="module")
def first_target_with_accessibility():
    screen = make_sorting_variant_screen(40, 3, seed=3, with_accessibility=True)
    return elbo.as_float64(screen[ic.target_guides(screen, 0)])


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"cp={r[0]}-counts={r[1]}")
def test_rule_under_accessibility_on_the_unresolved_rows(first_target_with_accessibility, row):
    """The rows of tests/test_tail_reference.py with the accessibility scaling on - marg_h<true>'s integrand, whose clamp
    of the scaled share at 1e-3 is a kink inside the mass of the weight - at four (mu, sd), guide noise 0 and 0.5 randn:
    the rule's own check |J64 - J48| and its distance to the 320-node rule are below section 21's bound of 1e-3 nat per
    pair; without accessibility the same figures are the smooth integrand's.  Measured: DESIGN.md section 25."""
    data = first_target_with_accessibility
    cp, counts = row
    c_p, ctrl = _override(data, cp, counts)
    a_prime = mr.beta_exponents(data, c_p, ctrl)
    assert not bool(mr.resolved(data, c_p, ctrl).any())
    rg = data.repguide_mask
    T, G = data.n_targets, data.n_guides
    noises = (torch.zeros(G, dtype=torch.float64),
              0.5 * torch.randn(G, generator=torch.Generator().manual_seed(1), dtype=torch.float64))
    worst = {}
    for acc in (False, True):
        check = far = 0.0
        for mu, sd in SETTINGS:
            for lpn in noises:
                h = mr.PairIntegrand(data, torch.full((T,), mu), torch.full((T,), sd), c_p, scale_by_accessibility=acc,
                                     lpn=lpn if acc else None, ctrl=ctrl)
                J = {Q_: tr.jacobi_rule(h, a_prime, Q_) for Q_ in (tr.TAIL_CHECK_NODES, tr.TAIL_NODES, 320)}
                assert bool(torch.isfinite(J[320][rg]).all())
                check = max(check, float((J[64] - J[48]).abs()[rg].max()))
                far = max(far, float((J[64] - J[320]).abs()[rg].max()))
        worst[acc] = (check, far)
    print(f"c_p = {cp}, control counts {counts}: without accessibility |J64 - J48| {worst[False][0]:.1e}, |J64 - J320| "
          f"{worst[False][1]:.1e}; with accessibility |J64 - J48| {worst[True][0]:.1e}, |J64 - J320| {worst[True][1]:.1e}")
    for acc in (False, True):
        assert worst[acc][0] <= BOUND and worst[acc][1] <= BOUND, (acc, worst[acc])


# ---------------------------------------------------------------- importance_check over the CPU rule
class TailWeightsEngine:
    """``log_weights`` from the CPU rule, in the style of tail_common.TailRuleEngine: draws of q(mu, log sd) from torch's
    generator - draw d is the same whatever the call - ``logw`` the marginal log joint less log q, with
    ``tail_rule=True`` tail_reference's combined rule and its tail_err, without it marginal_reference's rule."""

    def __init__(self, data, alpha_pi, targets, loc, scale=(mr.CLAIM_MU_SCALE, mr.CLAIM_SD_SCALE)):
        c_p = mr.model_conc(data, {"alpha_pi": alpha_pi})
        full = mr.n_unresolved(data, {"alpha_pi": alpha_pi})
        self.subs = [(elbo.as_float64(data[ic.target_guides(data, t)]), c_p[ic.target_guides(data, t)]) for t in targets]
        self.n_unresolved = torch.tensor([int(full[t]) for t in targets], dtype=torch.int32)
        self.loc, self.scale = loc, scale
        self.calls = []

    def log_weights(self, first_draw, n_draws, seed=101, pairs=False, integrate_pi=None, tail_rule=False):
        self.calls.append((first_draw, n_draws, integrate_pi, tail_rule))
        T = len(self.subs)
        eps = torch.randn(first_draw + n_draws, 2, T, generator=torch.Generator().manual_seed(seed),
                          dtype=torch.float64)[first_draw:]
        centre = torch.tensor(self.loc, dtype=torch.float64)                     # (T, 2)
        mu = centre[:, 0] + self.scale[0] * eps[:, 0]
        y = centre[:, 1] + self.scale[1] * eps[:, 1]
        out = {"mu": mu, "y": y}
        if integrate_pi is None:
            out["logw"] = torch.zeros_like(mu)  # (the joint weights are not this test's subject)
            return out
        logq = (-0.5 * eps ** 2).sum(1) - math.log(self.scale[0] * self.scale[1]) - math.log(2.0 * math.pi)
        lj = torch.empty_like(mu)
        err = torch.zeros_like(mu)
        for j, (sub, cp) in enumerate(self.subs):
            if tail_rule:
                lj[:, j], err[:, j] = tr.marginal_log_joint(sub, cp, mu[:, j], y[:, j], Q=integrate_pi, with_err=True)
            else:
                lj[:, j] = mr.marginal_log_joint(sub, cp, mu[:, j], y[:, j], Q=integrate_pi)
        out.update({"logw": lj - logq, "n_unresolved": self.n_unresolved})
        if tail_rule:
            out["tail_err"] = err
        return out


def test_importance_check_passes_the_rule_through_and_reports_the_targets():
    """Targets 3 and 5 of tail_common.claim_screen_with_unedited_guides() (three tail pairs each), q centred near their
    posteriors, 256 draws: with tail_rule both get numbers and diagnostics far below the bar; without it both are NaN
    and no tail key appears; tail_rule without integrate_pi is refused."""
    data, alpha = tc.claim_screen_with_unedited_guides()
    eng = TailWeightsEngine(data, alpha, (3, 5), loc=[(-0.07, 0.02), (0.87, 0.01)])
    got = importance_check(eng, n_draws=256, seed=7, integrate_pi=32, tail_rule=True)
    plain = importance_check(eng, n_draws=256, seed=7, integrate_pi=32)
    assert eng.calls == [(0, 256, None, False), (0, 256, 32, True), (0, 256, None, False), (0, 256, 32, False)]
    assert set(TAIL_KEYS) <= set(got) and not set(TAIL_KEYS) & set(plain)
    assert got["n_pairs_tail"].tolist() == [3.0, 3.0] and plain["n_pairs_unresolved"].tolist() == [3.0, 3.0]
    print(f"CPU rule behind importance_check: is_tail_err {got['is_tail_err'].tolist()}, psis_k_marg "
          f"{got['psis_k_marg'].tolist()}, is_ess_marg {got['is_ess_marg'].tolist()}")
    assert bool((got["is_tail_err"] > 0).all()) and bool((got["is_tail_err"] <= TAIL_BOUND * got["n_pairs_tail"]).all())
    for k in MARGINAL_KEYS[:4]:
        assert bool(torch.isfinite(got[k]).all()) and bool(torch.isnan(plain[k]).all()), k
    assert bool((got["is_ess_marg"] >= 1.0).all()) and bool((got["is_ess_marg"] <= 256.0).all())
    with pytest.raises(ValueError, match="needs integrate_pi"):
        importance_check(eng, n_draws=256, tail_rule=True)
