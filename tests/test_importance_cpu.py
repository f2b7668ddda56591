"""Importance-sampling check of the mean-field posterior, the parts that need no GPU: the Pareto fit against exact
quantiles and an analytic tail, the summary's properties, the oracle-only version of the claim the GPU test makes, the C
entry point, the --importance-check flag with its refusals, and the table writer."""
import argparse
import contextlib
import ctypes
import io
import math
import os
import re
import types

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.importance import gpd_fit, importance_summary, psis, tail_size

import importance_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "golden")
RUN = ["run", "sorting", "variant", "screen.h5ad"]


def _scipy_k(x):
    from scipy.stats import genpareto

    return float(genpareto.fit(np.asarray(x, dtype=np.float64), floc=0)[0])


# ---------------------------------------------------------------- the Pareto fit
@pytest.mark.parametrize("k", [-0.3, 0.0, 0.3, 0.7, 1.2])
def test_gpd_fit_on_exact_quantiles(k):
    """M = 200 exact GPD(k, 1) quantiles at (i - 0.5) / M: |k_hat - k| is held to the error of scipy's maximum-likelihood
    fit (location fixed at 0) of the same values plus 0.05 - the diagnostic is read at 0.5 / 0.7, half its resolution.
    The shrinkage is not applied (shrink=False)."""
    from scipy.stats import genpareto

    M = 200
    x = genpareto.ppf((np.arange(1, M + 1) - 0.5) / M, k)
    got, sigma = gpd_fit(torch.tensor(x).reshape(M, 1), shrink=False)
    ref = _scipy_k(x)
    print(f"k {k}: ours {float(got):.4f} (sigma {float(sigma):.4f}), scipy {ref:.4f}")
    assert abs(float(got) - k) <= abs(ref - k) + 0.05
    shrunk, _ = gpd_fit(torch.tensor(x).reshape(M, 1))
    assert float(shrunk) == pytest.approx((float(got) * M + 5.0) / (M + 10.0), abs=1e-12)


@pytest.mark.parametrize("sigma", [0.8, 0.5])
def test_psis_finds_the_analytic_tail(sigma):
    """Target N(0, 1), proposal N(0, sigma^2): the weights' tail index is k = 1 - sigma^2 (0.36, 0.75).  S = 20 000,
    generator seeded with 1234, M = 425.  With the shrinkage undone, |k_hat - k| is held to the error of scipy's fit of
    the same M exceedances plus 0.05.  Measured here: sigma 0.8 - ours 0.4428, scipy 0.4363 (true 0.36: a tail of 425
    out of 20 000 draws is not yet the asymptotic one); sigma 0.5 - ours 0.8264, scipy 0.8230 (true 0.75); ours and
    scipy's differ by 0.0065 and 0.0034, so the test also holds them within 0.02 of each other."""
    S = 20000
    g = torch.Generator().manual_seed(1234)
    z = torch.randn(S, 3, generator=g, dtype=torch.float64)[:, :1] * sigma
    logw = -0.5 * z * z + 0.5 * z * z / sigma ** 2
    smoothed, k = psis(logw)
    M = tail_size(S)
    assert M == 425
    raw = (float(k) * (M + 10) - 5.0) / M
    lw = logw[:, 0] - logw[:, 0].max()
    srt, _ = torch.sort(lw)
    ref = _scipy_k((srt[S - M:].exp() - srt[S - M - 1].exp()).numpy())
    true = 1.0 - sigma ** 2
    print(f"sigma {sigma}: k {true:.3f}, ours {raw:.4f}, scipy {ref:.4f}")
    assert abs(raw - true) <= abs(ref - true) + 0.05
    assert abs(raw - ref) <= 0.02
    # the smoothed weights: only the tail changes, order kept, truncated at the raw maximum
    assert smoothed.shape == logw.shape and float(smoothed.max()) <= 0.0
    order = torch.argsort(lw)
    body = order[: S - M]
    assert torch.equal(smoothed[body, 0], lw[body])
    assert bool((smoothed[order[S - M:], 0].diff() >= 0).all())


def test_psis_refuses_too_few_draws_and_other_shapes():
    with pytest.raises(ValueError, match="25"):
        psis(torch.zeros(24, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(S, T\)"):
        psis(torch.zeros(100, dtype=torch.float64))
    assert tail_size(25) == 5 and tail_size(100) == 20 and tail_size(1000) == 95 and tail_size(4096) == 192
    psis(torch.randn(25, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(0)))


def test_psis_is_vectorised_over_targets():
    g = torch.Generator().manual_seed(5)
    lw = torch.randn(400, 7, generator=g, dtype=torch.float64) * torch.linspace(0.2, 3.0, 7, dtype=torch.float64)
    both, k = psis(lw)
    for t in range(7):
        one, k1 = psis(lw[:, t:t + 1])
        # (the same arithmetic; the reductions run over other strides, so to float64 rounding and not bit for bit)
        np.testing.assert_allclose(one[:, 0], both[:, t], rtol=1e-10, atol=1e-12)
        assert float(k1) == pytest.approx(float(k[t]), abs=1e-10)


# ---------------------------------------------------------------- the summary
def test_importance_summary_properties():
    S, T = 300, 4
    g = torch.Generator().manual_seed(2)
    mu = torch.randn(S, T, generator=g, dtype=torch.float64)
    # equal weights: is_ess = S and the plain moments
    out = importance_summary(torch.full((S, T), -3.0, dtype=torch.float64), mu)
    assert set(out) == {"psis_k", "is_ess", "mu_is", "mu_sd_is", "n_is"}
    np.testing.assert_allclose(out["is_ess"], np.full(T, float(S)), rtol=1e-12)
    np.testing.assert_allclose(out["mu_is"], mu.mean(0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(out["mu_sd_is"], mu.std(0, unbiased=False), rtol=1e-12)
    assert out["n_is"].tolist() == [float(S)] * T
    # one dominant weight: is_ess -> 1, and the moments are that draw's (the smoothing hands the other tail draws the
    # fitted quantiles, a per cent of the mass between them: is_ess 1.01 here)
    lw = torch.randn(S, T, generator=g, dtype=torch.float64)
    lw[17] += 200.0
    out = importance_summary(lw, mu)
    print("one dominant weight: is_ess", out["is_ess"].tolist())
    assert bool((out["is_ess"] < 1.05).all()) and bool((out["is_ess"] >= 1.0).all())
    np.testing.assert_allclose(out["mu_is"], mu[17], atol=0.05)
    assert bool((out["psis_k"] > 0.7).all())
    # a per-target constant added to logw changes nothing
    lw = torch.randn(S, T, generator=g, dtype=torch.float64) * 1.5
    a = importance_summary(lw, mu)
    b = importance_summary(lw + torch.tensor([1e3, -1e3, 0.5, 7.0], dtype=torch.float64), mu)
    for key in a:
        np.testing.assert_allclose(b[key], a[key], rtol=1e-9, atol=1e-12, err_msg=key)
    assert bool(torch.isfinite(a["psis_k"]).all())
    with pytest.raises(ValueError, match="shape"):
        importance_summary(lw, mu[:, :2])


def test_the_claim_holds_for_the_oracle_alone():
    """The claim of tests/test_gpu_importance.py::test_check_recovers_the_exact_posterior with the device taken out: the
    same screen, the same hand-set q, S = 4096 draws from torch's generator, logw = the oracle's one-target log joint
    less log q.  On every CLAIM_TARGET with psis_k < 0.7 (at least two of three), |mu_is - E[mu | x]| <= 4 sd[mu | x] /
    sqrt(is_ess) against the 2-D quadrature."""
    from oracle import elbo

    data = ic.claim_screen()
    S, T = ic.CLAIM_DRAWS, data.n_targets
    g = torch.Generator().manual_seed(11)
    summary = {k: torch.full((T,), float("nan"), dtype=torch.float64) for k in ("psis_k", "is_ess", "mu_is", "mu_sd_is")}
    for t in ic.CLAIM_TARGETS:
        sub = elbo.as_float64(data[ic.target_guides(data, t)])
        e1 = torch.randn(S, generator=g, dtype=torch.float64)
        e2 = torch.randn(S, generator=g, dtype=torch.float64)
        mu, y = e1 * ic.CLAIM_MU_SCALE, e2 * ic.CLAIM_SD_SCALE
        logq = -0.5 * e1 * e1 - 0.5 * e2 * e2 - y  # up to a constant (the LogNormal's Jacobian is - y)
        logw = ic.normal_log_joint(sub, mu, y) - logq
        one = importance_summary(logw.reshape(S, 1), mu.reshape(S, 1))
        for k in summary:
            summary[k][t] = one[k][0]
    ic.assert_claim(summary, data, "oracle alone")


def test_one_target_log_joint_is_the_oracles():
    """normal_log_joint (the quadrature's integrand) against oracle.elbo.normal_loss's model sites on the cut screen."""
    from oracle import elbo

    data = ic.claim_screen()
    t = ic.CLAIM_TARGETS[1]
    sub = elbo.as_float64(data[ic.target_guides(data, t)])
    mu = torch.tensor([-0.7, 0.0, 0.31], dtype=torch.float64)
    y = torch.tensor([0.02, -0.01, 0.0], dtype=torch.float64)
    got = ic.normal_log_joint(sub, mu, y)
    for i in range(3):
        rec = {}
        params = {"mu_loc": mu[i].reshape(1, 1), "mu_scale": torch.zeros(1, 1, dtype=torch.float64),
                  "sd_loc": y[i].reshape(1, 1), "sd_scale": torch.zeros(1, 1, dtype=torch.float64)}
        zero = {"eps_mu": torch.zeros(1, 1, dtype=torch.float64), "eps_sd": torch.zeros(1, 1, dtype=torch.float64)}
        elbo.normal_loss(sub, params, noise=zero, record=rec)
        want = sum(rec["model"].values())
        assert abs(float(got[i]) - want) <= 1e-10 * sum(abs(v) for v in rec["model"].values())


# ---------------------------------------------------------------- the C entry point
def test_entry_point_declared_listed_and_exported_by_every_library():
    text = open(os.path.join(ROOT, "include", "bean_hip.h")).read()
    assert "#define BEAN_HIP_MAX_LOGW_DRAWS 4096" in text and _lib.MAX_LOGW_DRAWS == 4096
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "bean_hip_log_weights"
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert name in {s[0] for s in _lib.SYMBOLS} and name in _lib.ENSEMBLE_SYMBOLS
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for build in _lib.ALL_BUILDS:
        assert hasattr(ctypes.CDLL(_lib.build_library(amax=build)), name), _lib.tree_path(build)
    lib = _lib.load()
    assert lib.bean_hip_log_weights(None, 1, 0, 1, None, 0, None, 0, None, 0, None, 0, None) < 0
    assert "null handle" in lib.bean_hip_last_error().decode()


# ---------------------------------------------------------------- the flag
def test_flag_defaults_and_help():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser
    from bean_amd.model.parser import parse_args

    parser = get_parser()
    args = parser.parse_args(RUN)
    assert args.importance_check == 0 and args.importance_seed == 101
    assert cli_run.importance_draws(args) == 0 and cli_run.importance_draws(argparse.Namespace()) == 0
    args = parser.parse_args(RUN + ["--importance-check", "1000", "--importance-seed", "7"])
    assert args.importance_check == 1000 and args.importance_seed == 7 and cli_run.importance_draws(args) == 1000
    for bad in ("-1", "many"):
        with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(io.StringIO()):
            parser.parse_args(RUN + ["--importance-check", bad])
        assert exc.value.code == 2
    with pytest.raises(ValueError, match="at least 25"):
        cli_run.importance_draws(parser.parse_args(RUN + ["--importance-check", "24"]))
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    assert not hasattr(plain.parse_args(RUN[1:]), "importance_check")  # the reference's flag table stays as it is
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    assert "--importance-check" in help_text and "psis_k" in help_text and "--importance-seed" in help_text
    # it combines with the member flags, the predictive check and --load-existing
    for extra in (["--n-seeds", "2"], ["--jackknife-replicates"], ["--load-existing"], ["--num-particles", "2"],
                  ["--bootstrap", "4"], ["--posterior-predictive", "10"]):
        assert cli_run.importance_draws(parser.parse_args(RUN + extra + ["--importance-check", "50"])) == 50


@pytest.mark.parametrize("selection,design,named", [("sorting", "tiling", "tiling screens (MultiMixtureNormal)"),
                                                     ("survival", "variant", "survival screens"),
                                                     ("survival", "tiling", "tiling screens (MultiMixtureNormal)")])
def test_unsupported_families_are_refused_at_the_parser_and_in_cli_run(selection, design, named):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser, main

    argv = ["run", selection, design, "screen.h5ad", "--importance-check", "50"]
    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2
    msg = " ".join(err.getvalue().split())
    assert "--importance-check" in msg and named in msg and "is not available for" in msg
    with pytest.raises(ValueError, match=re.escape(named)):
        cli_run.importance_draws(get_parser().parse_args(argv))
    assert cli_run.importance_draws(get_parser().parse_args(argv[:-2])) == 0  # without the flag nothing is refused


def test_too_few_draws_are_refused_at_the_parser():
    from bean_amd.cli.execute import main

    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(RUN + ["--importance-check", "10"])
    assert exc.value.code == 2 and "at least 25" in " ".join(err.getvalue().split())


def test_run_importance_check_names_the_family_it_refuses():
    from functools import partial

    import bean_amd.model.model as m
    import bean_amd.model.survival_model as sm
    from bean_amd.engine import PredictiveUnsupported
    from bean_amd.model.run import run_importance_check

    screen = lambda **kw: types.SimpleNamespace(**{"selection": "sorting", "library_design": "variant", **kw})  # noqa: E731
    for model, guide, data, named in (
        (partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide), screen(library_design="tiling"), "MultiMixtureNormal"),
        (partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide), screen(selection="survival"), "survival"),
        (partial(m.ControlNormalModel), partial(m.ControlNormalGuide), screen(), "ControlNormal"),
        (partial(m.NormalModel), m.NormalGuide, screen(sample_covariates=["batch"]), "sample covariates (Normal)"),
    ):
        with pytest.raises(PredictiveUnsupported, match=re.escape(named)) as exc:
            run_importance_check(model, guide, data, {})
        assert "an importance-sampling check is not available for" in str(exc.value)


# ---------------------------------------------------------------- the table
def _writer_case():
    src = open(os.path.join(HERE, "make_readwrite_golden.py")).read()
    ns = {}
    exec("import numpy as np, pandas as pd, torch\n" + src[src.index("CASES = {"):src.index("def main():")], ns)
    return ns["build"]("plain", 100)


def test_table_writer_with_and_without_the_columns(tmp_path):
    from bean_amd.model import readwrite

    written, summary = {}, None
    for what in ("plain", "none", "checked"):
        target, guide, P, neg, kw = _writer_case()
        prefix = str(tmp_path / what) + "/"
        os.makedirs(prefix)
        if what == "checked":
            T = len(target)
            g = torch.Generator().manual_seed(4)
            summary = {"psis_k": torch.rand(T, generator=g, dtype=torch.float64), "mu_is": torch.randn(T, generator=g, dtype=torch.float64),
                       "mu_sd_is": torch.rand(T, generator=g, dtype=torch.float64), "is_ess": 1 + 99 * torch.rand(T, generator=g, dtype=torch.float64),
                       "n_is": torch.full((T,), 500.0, dtype=torch.float64)}
            summary["psis_k"][3] = math.inf
            kw = {**kw, "importance": summary}
        elif what == "none":
            kw = {**kw, "importance": None}
        with contextlib.redirect_stdout(io.StringIO()):
            readwrite.write_result_table(target, guide, P, "M", prefix=prefix, **kw)
        written[what] = {n: open(prefix + n, "rb").read() for n in ("bean_element_result.M.csv", "bean_sgRNA_result.M.csv")}
    assert written["plain"] == written["none"]
    assert written["plain"]["bean_sgRNA_result.M.csv"] == written["checked"]["bean_sgRNA_result.M.csv"]
    plain = pd.read_csv(io.BytesIO(written["plain"]["bean_element_result.M.csv"]), index_col=0)
    got = pd.read_csv(io.BytesIO(written["checked"]["bean_element_result.M.csv"]), index_col=0)
    own = ["psis_k", "mu_is", "mu_sd_is", "is_ess", "n_is"]
    assert [c for c in got.columns if c not in plain.columns] == own
    assert got.drop(columns=own).equals(plain)
    assert (got["n_is"] == 500).all() and got["n_is"].dtype == np.int64
    assert sorted(got["mu_is"].tolist()) == pytest.approx(sorted(summary["mu_is"].tolist()))
    assert np.isinf(got["psis_k"]).sum() == 1
    target, guide, P, neg, kw = _writer_case()
    with pytest.raises(ValueError, match="importance-sampling summary"):
        readwrite.write_result_table(target, guide, P, "M", prefix=str(tmp_path / "checked") + "/",
                                     **{**kw, "importance": {k: v[:-1] for k, v in summary.items()}})
