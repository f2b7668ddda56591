"""Posterior predictive check, the parts that need no GPU: the summary statistics on hand-made arrays, their
accumulation over draws, the two C entry points, the --posterior-predictive flag with its refusals, and the files."""
import argparse
import contextlib
import ctypes
import io
import os
import re
import types

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.predictive import (bin_midpoints, predictive_summary, two_sided_p, write_predictive_tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "golden")
NAMES = ("bean_hip_predictive_supported", "bean_hip_simulate")
RUN = ["run", "sorting", "variant", "screen.h5ad"]
NAN = float("nan")


# ---------------------------------------------------------------- the C entry points
def test_entry_points_declared_listed_and_exported_by_every_library():
    text = open(os.path.join(ROOT, "include", "bean_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    listed = {s[0] for s in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in bean_hip.h"
        assert name in listed, f"{name} not in _lib.SYMBOLS"
    for build in _lib.ALL_BUILDS:
        lib = ctypes.CDLL(_lib.build_library(amax=build))
        for name in NAMES:
            assert hasattr(lib, name), f"{name} not exported by {_lib.tree_path(build)}"


def test_null_handles_are_rejected_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    for what, call in (("predictive_supported", lambda: lib.bean_hip_predictive_supported(None)),
                       ("simulate", lambda: lib.bean_hip_simulate(None, 1, 0, None, 0, None, 0, None, 0, None))):
        assert call() < 0, what
        msg = lib.bean_hip_last_error().decode()
        assert what in msg and "null handle" in msg, (what, msg)


# ---------------------------------------------------------------- the summary
def _masks(R, B, G, thres=10):
    return {"repguide": torch.ones((R, G), dtype=torch.bool), "sample": torch.ones((R, B)), "mask_thres": thres}


def test_two_sided_p_at_its_ends():
    S = 9
    n = lambda v: torch.tensor([float(v)])  # noqa: E731
    assert two_sided_p(n(S), n(0), S).item() == pytest.approx(2 * 1 / 10)   # every draw above the observed value
    assert two_sided_p(n(0), n(S), S).item() == pytest.approx(2 * 1 / 10)   # every draw below
    assert two_sided_p(n(S), n(S), S).item() == 1.0                         # ties everywhere: capped at 1
    assert two_sided_p(n(5), n(4), S).item() == 1.0                         # 2 * 5 / 10
    assert two_sided_p(n(7), n(2), S).item() == pytest.approx(2 * 3 / 10)


def test_cell_and_guide_p_values_above_below_ties():
    R, B, G, S = 2, 2, 3, 9
    mid = torch.tensor([0.25, 0.75])
    obs = torch.tensor([[[10., 10., 10.], [10., 10., 10.]]] * R)            # (R, B, G), totals 20
    # guide 0: every draw has more reads in bin 1 (score above); guide 1: fewer; guide 2: the observed counts again
    rep = obs.clone()
    rep[:, 0, 0], rep[:, 1, 0] = 5., 15.
    rep[:, 0, 1], rep[:, 1, 1] = 15., 5.
    out = predictive_summary({"X": obs}, ({"X": rep.clone()} for _ in range(S)), _masks(R, B, G), mid)
    lo = 2 * 1 / (S + 1)
    assert out["n_draws"] == S
    assert out["ppc_p_score"].tolist() == pytest.approx([lo, lo, 1.0])
    assert out["cell_p"][:, :, 0].flatten().tolist() == pytest.approx([lo] * 4)
    assert out["cell_p"][:, :, 2].flatten().tolist() == [1.0] * 4
    assert out["cell_mean"][0, 1].tolist() == [15., 5., 10.] and float(out["cell_sd"].abs().max()) == 0.0
    assert torch.isnan(out["cell_z"]).all() and torch.isnan(out["mean_z"]).all()  # sd 0: no z
    assert out["T_obs"].tolist() == pytest.approx([0.5, 0.5, 0.5])
    # identical replicates: V_obs = 0 and every draw's V is 0 too, so n_ge = S and the one-sided p is 1
    assert out["V_obs"].tolist() == [0.0, 0.0, 0.0] and out["ppc_p_spread"].tolist() == [1.0, 1.0, 1.0]
    assert out["frac_cells_p05"].tolist() == [[0.0, 0.0], [0.0, 0.0]]  # lo = 0.2 > 0.05 with nine draws
    assert "ppc_p_score_bcmatch" not in out


def test_masked_pairs_and_samples_are_left_out():
    R, B, G, S = 3, 2, 2, 19
    g = torch.Generator().manual_seed(1)
    obs = torch.randint(20, 60, (R, B, G), generator=g).float()
    obs[2, :, 1] = torch.tensor([3., 4.])                       # total 7 <= mask_thres: pair (2, 1) masked
    draws = [torch.randint(0, 80, (R, B, G), generator=g).float() for _ in range(S)]
    masks = _masks(R, B, G)
    masks["repguide"][0, 0] = False                             # pair (0, 0) masked
    masks["sample"][1, 0] = 0                                   # sample (1, 0) masked
    mid = torch.tensor([0.1, 0.9])
    out = predictive_summary({"X": obs}, ({"X": d} for d in draws), masks, mid)
    assert out["pair_unmasked"].tolist() == [[False, True], [True, True], [True, False]]
    assert not out["cell_unmasked"][1, 0].any() and out["cell_unmasked"][1, 1].all()
    # changing what is masked changes no guide or sample statistic
    obs2, draws2 = obs.clone(), [d.clone() for d in draws]
    obs2[0, :, 0] = torch.tensor([50., 50.])
    for d in draws2:
        d[0, :, 0] += 7
        d[2, :, 1] *= 3
    out2 = predictive_summary({"X": obs2}, ({"X": d} for d in draws2), masks, mid)
    for k in ("ppc_p_score", "ppc_p_spread", "ppc_z_score", "T_obs", "V_obs"):
        assert torch.equal(out[k], out2[k]), k
    # sample statistics: the cell mask takes the masked pairs out; the masked sample has none
    for k in ("frac_cells_p05", "mean_z"):
        assert torch.equal(torch.nan_to_num(out[k], nan=-1.0), torch.nan_to_num(out2[k], nan=-1.0)), k
        assert torch.isnan(out[k][1, 0])
    # by hand: guide 0 over replicates 1 and 2
    t = lambda x, r, gi: float((x[r, :, gi] * mid).sum() / x[r, :, gi].sum())  # noqa: E731
    want = (t(obs, 1, 0) + t(obs, 2, 0)) / 2
    assert out["T_obs"][0].item() == pytest.approx(want)
    tg = [(t(d, 1, 0) + t(d, 2, 0)) / 2 for d in draws]
    n_ge, n_le = sum(v >= want for v in tg), sum(v <= want for v in tg)
    assert out["ppc_p_score"][0].item() == pytest.approx(min(1.0, 2 * min(n_ge + 1, n_le + 1) / (S + 1)))
    assert out["ppc_z_score"][0].item() == pytest.approx((want - np.mean(tg)) / np.std(tg, ddof=1))
    frac = out["frac_cells_p05"][0, 0].item()  # sample (0, 0): guide 1 only
    assert frac == float(out["cell_p"][0, 0, 1] <= 0.05)


def test_spread_needs_two_unmasked_replicates():
    R, B, G, S = 2, 2, 2, 5
    obs = torch.tensor([[[20., 20.], [30., 10.]], [[25., 30.], [25., 30.]]])
    masks = _masks(R, B, G)
    masks["repguide"][1, 1] = False          # guide 1 has one unmasked replicate
    g = torch.Generator().manual_seed(2)
    draws = [torch.randint(5, 50, (R, B, G), generator=g).float() for _ in range(S)]
    out = predictive_summary({"X": obs}, ({"X": d} for d in draws), masks, torch.tensor([0.2, 0.8]))
    assert torch.isnan(out["V_obs"][1]) and torch.isnan(out["ppc_p_spread"][1])
    assert not torch.isnan(out["ppc_p_score"][1])
    t0 = [(0.2 * 20 + 0.8 * 30) / 50, (0.2 * 25 + 0.8 * 25) / 50]
    assert out["V_obs"][0].item() == pytest.approx(np.var(t0, ddof=1))
    assert 1 / (S + 1) <= out["ppc_p_spread"][0].item() <= 1.0
    # no unmasked replicate at all: every guide statistic is NaN
    masks["repguide"][0, 1] = False
    out = predictive_summary({"X": obs}, ({"X": d} for d in draws), masks, torch.tensor([0.2, 0.8]))
    for k in ("T_obs", "ppc_p_score", "ppc_z_score", "ppc_p_spread"):
        assert torch.isnan(out[k][1]) and not torch.isnan(out[k][0]), k


def test_midpoints_come_from_the_bounds():
    up = torch.tensor([0.2, 0.4, 0.8, 1.0, 1.0])
    lo = torch.tensor([0.0, 0.2, 0.6, 0.0, 0.8])
    assert bin_midpoints(up, lo).tolist() == pytest.approx([0.1, 0.3, 0.7, 0.5, 0.9])
    assert bin_midpoints(up, lo).dtype == torch.float64


def test_accumulation_equals_the_stacked_draws():
    R, B, G, S = 2, 3, 5, 40
    g = torch.Generator().manual_seed(3)
    obs = {"X": torch.randint(10, 60, (R, B, G), generator=g).float(),
           "X_bcmatch": torch.randint(10, 40, (R, B, G), generator=g).float()}
    draws = [{k: torch.randint(0, 70, (R, B, G), generator=g).float() for k in obs} for _ in range(S)]
    mid = torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64)
    consumed = []

    def one_at_a_time():
        for i, d in enumerate(draws):
            consumed.append(i)
            yield d

    out = predictive_summary(obs, one_at_a_time(), _masks(R, B, G), mid)
    assert consumed == list(range(S)) and out["n_draws"] == S
    for key, sfx in (("X", ""), ("X_bcmatch", "_bcmatch")):
        stack = torch.stack([d[key] for d in draws]).double()          # (S, R, B, G)
        x = obs[key].double()
        np.testing.assert_allclose(out["cell_mean" + sfx], stack.mean(0), rtol=1e-12)
        np.testing.assert_allclose(out["cell_sd" + sfx], stack.std(0, unbiased=True), rtol=1e-10)
        n_ge, n_le = (stack >= x).sum(0), (stack <= x).sum(0)
        want_p = torch.clamp(2 * torch.minimum(n_ge + 1, n_le + 1).double() / (S + 1), max=1.0)
        assert torch.equal(out["cell_p" + sfx], want_p)
        np.testing.assert_allclose(out["cell_z" + sfx], (x - stack.mean(0)) / stack.std(0, unbiased=True), rtol=1e-9)
        t = (stack * mid.reshape(1, 1, -1, 1)).sum(2) / stack.sum(2)   # (S, R, G)
        t_obs = (x * mid.reshape(1, -1, 1)).sum(1) / x.sum(1)
        tg, tg_obs = t.mean(1), t_obs.mean(0)
        np.testing.assert_allclose(out["T_obs" + sfx], tg_obs, rtol=1e-12)
        want = torch.clamp(2 * torch.minimum((tg >= tg_obs).sum(0) + 1, (tg <= tg_obs).sum(0) + 1).double() / (S + 1), max=1.0)
        assert torch.equal(out["ppc_p_score" + sfx], want)
        np.testing.assert_allclose(out["ppc_z_score" + sfx], (tg_obs - tg.mean(0)) / tg.std(0, unbiased=True), rtol=1e-8)
        vg, vg_obs = t.var(1, unbiased=True), t_obs.var(0, unbiased=True)
        assert torch.equal(out["ppc_p_spread" + sfx], ((vg >= vg_obs).sum(0) + 1).double() / (S + 1))
        np.testing.assert_allclose(out["frac_cells_p05" + sfx], (want_p <= 0.05).double().mean(2))
    with pytest.raises(ValueError, match="at least one"):
        predictive_summary(obs, iter(()), _masks(R, B, G), mid)


# ---------------------------------------------------------------- the flag
def test_flag_defaults_and_help():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser
    from bean_amd.model.parser import parse_args

    parser = get_parser()
    args = parser.parse_args(RUN)
    assert args.posterior_predictive == 0 and args.predictive_seed == 101
    assert cli_run.predictive_draws(args) == 0 and cli_run.predictive_draws(argparse.Namespace()) == 0
    args = parser.parse_args(RUN + ["--posterior-predictive", "200", "--predictive-seed", "7"])
    assert args.posterior_predictive == 200 and args.predictive_seed == 7 and cli_run.predictive_draws(args) == 200
    for bad in ("-1", "many"):
        with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(io.StringIO()):
            parser.parse_args(RUN + ["--posterior-predictive", bad])
        assert exc.value.code == 2
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    assert not hasattr(plain.parse_args(RUN[1:]), "posterior_predictive")  # the reference's flag table stays as it is
    help_text = " ".join(parser._subparsers._group_actions[0].choices["run"].format_help().split())
    assert "--posterior-predictive" in help_text and "--fit-negctrl control fit is not checked" in help_text
    # it combines with the member flags and with --load-existing
    for extra in (["--n-seeds", "2"], ["--jackknife-replicates"], ["--load-existing"], ["--num-particles", "2"]):
        assert cli_run.predictive_draws(parser.parse_args(RUN + extra + ["--posterior-predictive", "5"])) == 5


@pytest.mark.parametrize("selection,design,named", [("sorting", "tiling", "tiling screens (MultiMixtureNormal)"),
                                                     ("survival", "variant", "survival screens"),
                                                     ("survival", "tiling", "tiling screens (MultiMixtureNormal)")])
def test_unsupported_families_are_refused_at_the_parser_and_in_cli_run(selection, design, named):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser, main

    argv = ["run", selection, design, "screen.h5ad", "--posterior-predictive", "50"]
    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2
    msg = " ".join(err.getvalue().split())
    assert "--posterior-predictive" in msg and named in msg and "is not available for" in msg
    with pytest.raises(ValueError, match=re.escape(named)):
        cli_run.predictive_draws(get_parser().parse_args(argv))
    assert cli_run.predictive_draws(get_parser().parse_args(argv[:-2])) == 0  # without the flag nothing is refused


def test_run_posterior_predictive_names_the_family_it_refuses():
    from functools import partial

    import bean_amd.model.model as m
    import bean_amd.model.survival_model as sm
    from bean_amd.engine import PredictiveUnsupported
    from bean_amd.model.run import run_posterior_predictive

    screen = lambda **kw: types.SimpleNamespace(**{"selection": "sorting", "library_design": "variant", **kw})  # noqa: E731
    for model, guide, data, named in (
        (partial(m.MultiMixtureNormalModel), partial(m.MultiMixtureNormalGuide), screen(library_design="tiling"), "MultiMixtureNormal"),
        (partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide), screen(selection="survival"), "survival"),
        (partial(m.ControlNormalModel), partial(m.ControlNormalGuide), screen(), "ControlNormal"),
        (partial(m.NormalModel), m.NormalGuide, screen(sample_covariates=["batch"]), "sample covariates (Normal)"),
    ):
        with pytest.raises(PredictiveUnsupported, match=re.escape(named)):
            run_posterior_predictive(model, guide, data, {})
    assert issubclass(PredictiveUnsupported, ValueError)


# ---------------------------------------------------------------- the files
def _writer_case():
    src = open(os.path.join(HERE, "make_readwrite_golden.py")).read()
    ns = {}
    exec("import numpy as np, pandas as pd, torch\n" + src[src.index("CASES = {"):src.index("def main():")], ns)
    return ns["build"]("plain", 100)


def test_files_and_the_other_tables_stay_as_they_are(tmp_path):
    from bean_amd.model import readwrite

    written = {}
    for what in ("plain", "checked"):
        target, guide, P, neg, kw = _writer_case()
        prefix = str(tmp_path / what) + "/"
        os.makedirs(prefix)
        with contextlib.redirect_stdout(io.StringIO()):
            readwrite.write_result_table(target, guide, P, "M", prefix=prefix, **kw)
        if what == "checked":
            G, R, B = len(guide), 2, 3
            g = torch.Generator().manual_seed(4)
            summary = {"n_draws": 50}
            for s in ("", "_bcmatch"):
                for c in ("ppc_p_score", "ppc_p_spread", "ppc_z_score"):
                    summary[c + s] = torch.rand(G, generator=g, dtype=torch.float64)
                for c in ("frac_cells_p05", "mean_z"):
                    summary[c + s] = torch.rand((R, B), generator=g, dtype=torch.float64)
            summary["ppc_p_spread"][0] = NAN
            data = types.SimpleNamespace(n_reps=R, n_condits=B, sample_mask=torch.tensor([[1, 1, 1], [0, 1, 1]]))
            paths = write_predictive_tables(summary, guide, data, prefix, "M", "")
            assert [os.path.basename(p) for p in paths] == ["bean_predictive_guides.M.csv", "bean_predictive_samples.M.csv"]
            sg = pd.read_csv(prefix + "bean_sgRNA_result.M.csv", index_col=0)
            got = pd.read_csv(paths[0], index_col=0)
            own = [c + s for s in ("", "_bcmatch") for c in ("ppc_p_score", "ppc_p_spread", "ppc_z_score")]
            assert list(got.columns) == list(sg.columns) + own and list(got.index) == list(sg.index)
            np.testing.assert_allclose(got["ppc_z_score_bcmatch"].values, summary["ppc_z_score_bcmatch"].numpy())
            assert np.isnan(got["ppc_p_spread"].values[0])
            sam = pd.read_csv(paths[1], index_col=0)
            assert list(sam.index) == [f"r{r}_c{b}" for r in range(R) for b in range(B)]
            assert list(sam.columns) == ["replicate", "condition", "masked", "frac_cells_p05", "mean_z",
                                         "frac_cells_p05_bcmatch", "mean_z_bcmatch", "n_draws"]
            assert sam["masked"].tolist() == [False, False, False, True, False, False]
            np.testing.assert_allclose(sam["mean_z"].values, summary["mean_z"].reshape(-1).numpy())
            with pytest.raises(ValueError, match="guides"):
                write_predictive_tables(summary, guide.iloc[:-1], data, prefix, "M", "")
        written[what] = {n: open(prefix + n, "rb").read() for n in ("bean_element_result.M.csv", "bean_sgRNA_result.M.csv")}
    assert written["plain"] == written["checked"]
