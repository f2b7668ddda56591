"""The importance check with pi integrated out, the parts that need no GPU: the suffixed summary and
its NaN rule, the C entry point's declaration, the two flags with their refusals, the table writer, and the claim of the
GPU test made with the CPU rule and torch's generator alone."""
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
from bean_amd.model.importance import MARGINAL_KEYS, importance_check, importance_summary, marginal_summary

import importance_common as ic
import marginal_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "golden")
RUN = ["run", "sorting", "variant", "screen.h5ad"]


# ---------------------------------------------------------------- the summary
def _weights(S=400, T=6, seed=2):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(S, T, generator=g, dtype=torch.float64)
    return 0.3 * torch.randn(S, T, generator=g, dtype=torch.float64) - 0.5 * mu, mu


def test_marginal_summary_keys_and_the_nan_rule():
    logw, mu = _weights()
    n = torch.tensor([0, 2, 0, 0, 1, 0], dtype=torch.int32)
    got = marginal_summary(logw, mu, n)
    assert tuple(got) == MARGINAL_KEYS
    plain = importance_summary(logw, mu)
    left_out = n > 0
    for k in ("psis_k", "mu_is", "mu_sd_is", "is_ess"):
        assert bool(torch.isnan(got[k + "_marg"][left_out]).all())
        assert torch.equal(got[k + "_marg"][~left_out], plain[k][~left_out])
    assert got["n_pairs_unresolved"].tolist() == [0.0, 2.0, 0.0, 0.0, 1.0, 0.0]
    none = marginal_summary(logw, mu, torch.zeros(6, dtype=torch.int32))
    assert all(torch.equal(none[k + "_marg"], plain[k]) for k in ("psis_k", "mu_is", "mu_sd_is", "is_ess"))
    with pytest.raises(ValueError, match="one count per target"):
        marginal_summary(logw, mu, n[:-1])


class _Engine:
    """What importance_check asks of an engine."""

    def __init__(self):
        self.calls = []
        self.joint, self.mu = _weights()
        self.marg = self.joint + 0.1 * self.mu

    def log_weights(self, first, n, seed=101, integrate_pi=None):
        self.calls.append((first, n, seed, integrate_pi))
        out = {"logw": self.joint if integrate_pi is None else self.marg, "mu": self.mu, "y": self.mu}
        if integrate_pi is not None:
            out["n_unresolved"] = torch.tensor([0, 0, 3, 0, 0, 0], dtype=torch.int32)
        return out


def test_importance_check_merges_the_two_summaries():
    eng = _Engine()
    plain = importance_check(eng, n_draws=400, seed=7)
    assert eng.calls == [(0, 400, 7, None)] and set(plain) == {"psis_k", "is_ess", "mu_is", "mu_sd_is", "n_is"}
    both = importance_check(eng, n_draws=400, seed=7, integrate_pi=32)
    assert eng.calls[1:] == [(0, 400, 7, None), (0, 400, 7, 32)]
    assert list(both) == list(plain) + list(MARGINAL_KEYS)
    for k in plain:
        assert torch.equal(both[k], plain[k])
    want = marginal_summary(eng.marg, eng.mu, torch.tensor([0, 0, 3, 0, 0, 0]))
    for k in MARGINAL_KEYS:
        assert torch.equal(both[k].isnan(), want[k].isnan()) and torch.equal(both[k].nan_to_num(), want[k].nan_to_num())
    assert math.isnan(float(both["mu_is_marg"][2])) and float(both["n_pairs_unresolved"][2]) == 3.0


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    name = "bean_hip_log_weights_marginal"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in {s[0] for s in _lib.SYMBOLS} and name in _lib.ENSEMBLE_SYMBOLS and _lib.MARGINAL_NODES == (16, 32, 64)
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), name), _lib.tree_path(build)
    lib = _lib.load()
    assert lib.bean_hip_log_weights_marginal(None, 1, 0, 1, 32, None, 0, None, 0, None, 0, None, 0, None, 0, None) < 0
    assert "null handle" in lib.bean_hip_last_error().decode()


# ---------------------------------------------------------------- the flags
def test_flags_defaults_parsing_and_help():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    parser = get_parser()
    args = parser.parse_args(RUN)
    assert args.importance_integrate_pi is False and args.importance_nodes == 32 and cli_run.importance_nodes(args) is None
    assert cli_run.importance_nodes(parser.parse_args(RUN + ["--importance-check", "100"])) is None
    args = parser.parse_args(RUN + ["--importance-check", "100", "--importance-integrate-pi"])
    assert cli_run.importance_nodes(args) == 32 and cli_run.importance_draws(args) == 100
    for q in (16, 32, 64):
        args = parser.parse_args(RUN + ["--importance-check", "100", "--importance-integrate-pi", "--importance-nodes", str(q)])
        assert cli_run.importance_nodes(args) == q
    with pytest.raises(ValueError, match="16, 32, 64"):
        cli_run.importance_nodes(parser.parse_args(RUN + ["--importance-check", "100", "--importance-integrate-pi",
                                                          "--importance-nodes", "20"]))
    with pytest.raises(ValueError, match="needs that flag"):
        cli_run.importance_nodes(parser.parse_args(RUN + ["--importance-integrate-pi"]))
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    for word in ("--importance-integrate-pi", "--importance-nodes", "psis_k_marg", "n_pairs_unresolved"):
        assert word in help_text, word


@pytest.mark.parametrize("argv,words", [
    (RUN + ["--importance-integrate-pi"], ("--importance-integrate-pi", "--importance-check")),
    (RUN + ["--importance-check", "50", "--importance-integrate-pi", "--importance-nodes", "20"], ("--importance-nodes", "16, 32, 64")),
    (["run", "sorting", "tiling", "screen.h5ad", "--importance-check", "50", "--importance-integrate-pi"],
     ("--importance-check", "tiling screens (MultiMixtureNormal)")),
    (["run", "survival", "variant", "screen.h5ad", "--importance-check", "50", "--importance-integrate-pi"],
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


def test_run_importance_check_refuses_control_normal_with_the_flag():
    import types
    from functools import partial

    import bean_amd.model.model as m
    from bean_amd.engine import PredictiveUnsupported
    from bean_amd.model.run import run_importance_check

    data = types.SimpleNamespace(selection="sorting", library_design="variant")
    with pytest.raises(PredictiveUnsupported, match="ControlNormal"):
        run_importance_check(partial(m.ControlNormalModel), partial(m.ControlNormalGuide), data, {}, integrate_pi=32)


# ---------------------------------------------------------------- the table
def _writer_case():
    src = open(os.path.join(HERE, "make_readwrite_golden.py")).read()
    ns = {}
    exec("import numpy as np, pandas as pd, torch\n" + src[src.index("CASES = {"):src.index("def main():")], ns)
    return ns["build"]("plain", 100)


def test_table_writer_puts_the_five_columns_behind_the_importance_columns(tmp_path):
    from bean_amd.model import readwrite

    written = {}
    for what in ("joint", "both"):
        target, guide, P, neg, kw = _writer_case()
        T = len(target)
        g = torch.Generator().manual_seed(4)
        summary = {"psis_k": torch.rand(T, generator=g, dtype=torch.float64), "mu_is": torch.randn(T, generator=g, dtype=torch.float64),
                   "mu_sd_is": torch.rand(T, generator=g, dtype=torch.float64), "is_ess": 1 + 99 * torch.rand(T, generator=g, dtype=torch.float64),
                   "n_is": torch.full((T,), 500.0, dtype=torch.float64)}
        if what == "both":
            n = torch.zeros(T, dtype=torch.int32)
            n[3] = 2
            summary.update(marginal_summary(*_weights(S=500, T=T), n))
        prefix = str(tmp_path / what) + "/"
        os.makedirs(prefix)
        with contextlib.redirect_stdout(io.StringIO()):
            readwrite.write_result_table(target, guide, P, "M", prefix=prefix, **{**kw, "importance": summary})
        written[what] = {n_: open(prefix + n_, "rb").read() for n_ in ("bean_element_result.M.csv", "bean_sgRNA_result.M.csv")}
    assert written["joint"]["bean_sgRNA_result.M.csv"] == written["both"]["bean_sgRNA_result.M.csv"]
    joint = pd.read_csv(io.BytesIO(written["joint"]["bean_element_result.M.csv"]), index_col=0)
    got = pd.read_csv(io.BytesIO(written["both"]["bean_element_result.M.csv"]), index_col=0)
    assert [c for c in got.columns if c not in joint.columns] == list(MARGINAL_KEYS)
    cols = list(got.columns)
    assert cols[cols.index("n_is") + 1:cols.index("n_is") + 6] == list(MARGINAL_KEYS)
    assert got.drop(columns=list(MARGINAL_KEYS)).equals(joint)
    assert got["n_pairs_unresolved"].dtype == np.int64 and int(got["n_pairs_unresolved"].sum()) == 2
    left_out = got["n_pairs_unresolved"] > 0
    for k in MARGINAL_KEYS[:4]:
        assert got[k][left_out].isna().all() and got[k][~left_out].notna().all()


# ---------------------------------------------------------------- the claim, without the device
def test_the_marginal_claim_holds_for_the_cpu_rule_alone():
    """importance_common.claim_screen(), MixtureNormal, alpha_pi at its initial value, q set by hand (marginal_reference.
    CLAIM_*), S = 4096 draws of (mu, log sd) from torch's generator; logw_marg = the one-target marginal log joint by the
    Q = 32 rule less log q.  The exact E[mu | x], sd[mu | x] come from a 61 x 31 grid over (mu, log sd) of the same log
    joint with the Q = 64 rule inside.  On every CLAIM_TARGET with psis_k_marg < 0.7 (at least two of three),
    |mu_is_marg - E[mu | x]| <= 4 sd[mu | x] / sqrt(is_ess_marg).
    Measured here: psis_k_marg -0.81, -0.64, -0.50; is_ess_marg 436, 383, 318; |mu_is_marg - E| 0.0013, 0.0040, 0.0003
    against caps of 0.0117, 0.0162, 0.0119; mu_sd_is_marg 0.0609, 0.0813, 0.0543 against the exact 0.0612, 0.0790, 0.0530;
    doubling the grid step moves the exact mean by at most 3e-5."""
    from oracle import elbo

    data = ic.claim_screen()
    S, T = ic.CLAIM_DRAWS, data.n_targets
    c_p = mr.model_conc(data, elbo.init_params("MixtureNormal", data))
    assert bool(mr.resolved(elbo.as_float64(data), c_p).all())
    g = torch.Generator().manual_seed(11)
    summary = {k: torch.full((T,), float("nan"), dtype=torch.float64) for k in MARGINAL_KEYS}
    for t in ic.CLAIM_TARGETS:
        idx = ic.target_guides(data, t)
        sub = elbo.as_float64(data[idx])
        e1 = torch.randn(S, generator=g, dtype=torch.float64)
        e2 = torch.randn(S, generator=g, dtype=torch.float64)
        mu, y = e1 * mr.CLAIM_MU_SCALE, e2 * mr.CLAIM_SD_SCALE
        logq = -0.5 * e1 * e1 - 0.5 * e2 * e2  # q as a density in (mu, log sd), as marginal_log_joint is; up to a constant
        logw = mr.marginal_log_joint(sub, c_p[idx], mu, y, Q=32) - logq
        one = marginal_summary(logw.reshape(S, 1), mu.reshape(S, 1), torch.zeros(1, dtype=torch.int32))
        for k in summary:
            summary[k][t] = one[k][0]
    mr.assert_marginal_claim(summary, data, ic.CLAIM_TARGETS, "CPU rule alone")
