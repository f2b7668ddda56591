"""Replicate jackknife, the parts that need no GPU: leave_out, the candidate replicates, jackknife_summary on hand-computed
numbers, the --jackknife-replicates flag, the four added columns of the element table, the C entry point (declared,
exported, listed, null handle rejected) and - through the CPU oracle - that a masked replicate has no influence on the
fit: no gradient, and only a constant in the loss."""
import copy
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model import readwrite
from bean_amd.model.jackknife import candidate_replicates, jackknife_summary, leave_out, member_masks
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen
from oracle import elbo, svi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
COLUMNS = ["mu_jk_se", "mu_jk_max_shift", "mu_jk_max_shift_rep", "n_jk"]


# ---------------------------------------------------------------- leave_out / candidates
def test_leave_out_changes_the_two_mask_rows_and_nothing_else():
    data = make_sorting_variant_screen(200, 3, seed=5, mask_fraction=0.05)
    before = {k: v.clone() for k, v in data.tensor_items()}
    out = leave_out(data, 1)
    for k, v in data.tensor_items():  # the original is not modified
        assert torch.equal(v, before[k]), k
    assert set(vars(out)) == set(vars(data))
    for k, v in vars(data).items():
        if k in ("sample_mask", "repguide_mask"):
            continue
        w = getattr(out, k)
        assert w is v or (isinstance(v, torch.Tensor) and torch.equal(v, w)), k
    for name in ("sample_mask", "repguide_mask"):
        a, b = getattr(data, name), getattr(out, name)
        assert a.dtype == b.dtype and a.shape == b.shape
        assert not bool(b[1].any()), name
        assert torch.equal(a[[0, 2]], b[[0, 2]]), name
        assert bool(a[1].any()), name
    assert out.sample_mask.data_ptr() != data.sample_mask.data_ptr()
    with pytest.raises(ValueError, match="replicate 3"):
        leave_out(data, 3)


def test_candidates_and_member_masks():
    data = make_sorting_variant_screen(120, 4, seed=5, mask_fraction=0.05)
    assert candidate_replicates(data) == [0, 1, 2, 3]
    gone = leave_out(data, 2)
    assert candidate_replicates(gone) == [0, 1, 3]  # an already fully masked replicate is not left out again
    rg, sm = member_masks(gone, [0, 1, 3])
    assert rg.shape == (4, 4, 120) and rg.dtype == torch.bool and sm.shape == (4, 4, data.n_condits)
    assert torch.equal(rg[0], gone.repguide_mask) and torch.equal(sm[0], gone.sample_mask)
    for j, r in enumerate([0, 1, 3]):
        assert torch.equal(rg[1 + j], leave_out(gone, r).repguide_mask) and torch.equal(sm[1 + j], leave_out(gone, r).sample_mask)
    two = make_sorting_variant_screen(120, 2, seed=5)
    assert candidate_replicates(two) == [0, 1]
    with pytest.raises(ValueError, match="found 1"):
        candidate_replicates(leave_out(two, 0))
    with pytest.raises(ValueError, match="found 0"):
        candidate_replicates(leave_out(leave_out(two, 0), 1))


# ---------------------------------------------------------------- jackknife_summary
def _fit(mu):
    return {"mu_loc": torch.tensor(mu, dtype=torch.float32).reshape(-1, 1)}


def test_summary_matches_hand_computed_numbers():
    """Three replicates, two targets.  Target 0: m = (1, 2, 6), mean 3, sum of squares 4 + 1 + 9 = 14,
    se = sqrt(2/3 * 14); full 2.5: shifts 1.5, 0.5, 3.5 -> replicate 'c'.  Target 1: m = (0, -3, 0), mean -1,
    sum of squares 1 + 4 + 1 = 6, se = sqrt(2/3 * 6) = 2; full 0.25: shifts 0.25, 3.25, 0.25 -> replicate 'b'."""
    full = _fit([2.5, 0.25])
    loo = [_fit([1.0, 0.0]), _fit([2.0, -3.0]), (_fit([6.0, 0.0]), {"loss": [], "params": {}})]  # results or bare stores
    out = jackknife_summary(full, loo, [0, 1, 2], ["a", "b", "c"])
    assert set(out) == set(COLUMNS)
    assert out["mu_jk_se"].dtype == torch.float64 and out["mu_jk_se"].shape == (2, 1)
    np.testing.assert_allclose(out["mu_jk_se"].reshape(-1).numpy(), [np.sqrt(2.0 / 3.0 * 14.0), 2.0], rtol=1e-15)
    np.testing.assert_allclose(out["mu_jk_max_shift"].reshape(-1).numpy(), [3.5, 3.25], rtol=1e-15)
    assert out["mu_jk_max_shift_rep"] == ["c", "b"] and out["n_jk"] == 3
    # the left-out replicates need not be 0 .. n-1: a screen whose replicate 1 was masked from the start
    out = jackknife_summary(full, loo, [0, 2, 3], ["a", "b", "c", "d"])
    assert out["mu_jk_max_shift_rep"] == ["d", "c"]


def test_summary_of_two_replicates():
    """n = 2: m = (1, 3.5), mean 2.25, se = sqrt(1/2 * 2 * 1.25^2) = 1.25 = |m_0 - m_1| / 2."""
    out = jackknife_summary(_fit([2.0]), [_fit([1.0]), _fit([3.5])], [0, 1], ["r1", "r2"])
    np.testing.assert_allclose(out["mu_jk_se"].reshape(-1).numpy(), [1.25], rtol=1e-15)
    np.testing.assert_allclose(out["mu_jk_max_shift"].reshape(-1).numpy(), [1.5], rtol=1e-15)
    assert out["mu_jk_max_shift_rep"] == ["r2"] and out["n_jk"] == 2
    with pytest.raises(ValueError, match="at least two"):
        jackknife_summary(_fit([2.0]), [_fit([1.0])], [0], ["r1", "r2"])


# ---------------------------------------------------------------- flag
RUN = ["run", "sorting", "variant", "screen.h5ad"]


def test_flag_is_accepted_and_refused_with_n_seeds(capsys):
    from bean_amd.cli.execute import get_parser
    from bean_amd.cli.execute import main as bean_main
    from bean_amd.model.parser import parse_args as reference_table

    parser = get_parser()
    assert parser.parse_args(RUN).jackknife_replicates is False
    assert parser.parse_args(RUN + ["--jackknife-replicates"]).jackknife_replicates is True
    assert parser.parse_args(RUN + ["--jackknife-replicates", "--n-seeds", "1"]).n_seeds == 1
    with pytest.raises(SystemExit) as exc:
        bean_main(RUN + ["--jackknife-replicates", "--n-seeds", "2"])  # refused before anything is read or fitted
    assert exc.value.code == 2
    msg = capsys.readouterr().err
    assert "--jackknife-replicates" in msg and "--n-seeds" in msg
    with pytest.raises(SystemExit) as exc:
        bean_main(RUN + ["--jackknife-replicates", "--load-existing"])  # there are no leave-one-out fits to summarise
    assert exc.value.code == 2
    msg = capsys.readouterr().err
    assert "--jackknife-replicates" in msg and "--load-existing" in msg
    with pytest.raises(SystemExit):
        reference_table().parse_args(RUN[1:] + ["--jackknife-replicates"])  # not in the reference's flag table


# ---------------------------------------------------------------- table
def _write(tmp_path, name, **kw):
    n = 40
    g = torch.Generator().manual_seed(3)
    target_info = pd.DataFrame({"n_guides": 3}, index=pd.Index([f"t{i}" for i in range(n)], name="target"))
    guide_info = pd.DataFrame({"edit_rate": 0.5}, index=pd.Index([f"g{i}" for i in range(3 * n)], name="name"))
    P = {"mu_loc": torch.randn(n, 1, generator=g), "mu_scale": 0.1 + torch.rand(n, 1, generator=g),
         "sd_loc": 0.1 * torch.randn(n, 1, generator=g), "sd_scale": 0.1 + torch.rand(n, 1, generator=g)}
    prefix = str(tmp_path / name) + "."
    readwrite.write_result_table(target_info, guide_info, P, model_label="Normal", prefix=prefix,
                                 adjust_confidence_by_negative_control=False, **kw)
    return prefix, n


def test_element_table_gains_exactly_the_four_columns(tmp_path):
    ref_prefix, n = _write(tmp_path, "plain")
    jk = {"mu_jk_se": torch.linspace(0, 1, n, dtype=torch.float64).reshape(n, 1),
          "mu_jk_max_shift": torch.linspace(1, 2, n, dtype=torch.float64).reshape(n, 1),
          "mu_jk_max_shift_rep": [f"rep{i % 3}" for i in range(n)], "n_jk": 3}
    prefix, _ = _write(tmp_path, "jk", jackknife=jk)
    ref = pd.read_csv(ref_prefix + "bean_element_result.Normal.csv", float_precision="round_trip")
    got = pd.read_csv(prefix + "bean_element_result.Normal.csv", float_precision="round_trip")
    assert set(COLUMNS) <= set(got.columns) and not set(COLUMNS) & set(ref.columns)
    assert [c for c in got.columns if c not in COLUMNS] == list(ref.columns)
    pd.testing.assert_frame_equal(got.drop(columns=COLUMNS), ref, check_exact=True)
    by_target = got.set_index("target")
    for i in (0, 7, n - 1):
        row = by_target.loc[f"t{i}"]
        assert row["mu_jk_se"] == float(jk["mu_jk_se"][i]) and row["mu_jk_max_shift"] == float(jk["mu_jk_max_shift"][i])
        assert row["mu_jk_max_shift_rep"] == f"rep{i % 3}" and row["n_jk"] == 3
    assert (open(prefix + "bean_sgRNA_result.Normal.csv", "rb").read()
            == open(ref_prefix + "bean_sgRNA_result.Normal.csv", "rb").read())
    with pytest.raises(ValueError, match="entries for"):
        _write(tmp_path, "bad", jackknife=dict(jk, mu_jk_se=jk["mu_jk_se"][:-1]))


# ---------------------------------------------------------------- C entry point
def test_entry_point_declared_exported_listed_and_null_handle_rejected():
    _lib.build_library()
    lib = _lib.load()
    name = "bean_hip_bind_member_masks"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bean_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in bean_hip.h"
    assert hasattr(lib, name) and name in {s[0] for s in _lib.SYMBOLS}
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert lib.bean_hip_bind_member_masks(None, None, 0, None, 0) < 0
    msg = lib.bean_hip_last_error().decode()
    assert "bind_member_masks" in msg and "null handle" in msg


# ---------------------------------------------------------------- masked means no data influence (CPU oracle)
def _other_counts(data, r, seed):
    """The screen with replicate r's counts (all three observed sites) replaced by other counts."""
    g = torch.Generator().manual_seed(seed)
    out = copy.copy(data)
    for name in ("X", "X_masked", "X_bcmatch", "X_bcmatch_masked", "allele_counts_control"):
        v = getattr(data, name).clone()
        v[r] = torch.randint(0, 400, v[r].shape, generator=g).to(v.dtype)
        setattr(out, name, v)
    return out


@pytest.mark.parametrize("family,loss_fn", [("MixtureNormal", elbo.mixture_normal_loss), ("Normal", elbo.normal_loss)])
def test_a_masked_replicate_has_no_influence_in_the_oracle(family, loss_fn):
    data = make_sorting_variant_screen(200, 3, seed=11, mask_fraction=0.05)
    masked = leave_out(data, 1)
    swapped = _other_counts(masked, 1, seed=4)
    assert not torch.equal(swapped.X_masked[1], masked.X_masked[1])
    results = {}
    for at in ("initial", "moved"):
        torch.manual_seed(7)
        base = elbo.init_params(family, data)
        if at == "moved":
            g = torch.Generator().manual_seed(8)
            base = {k: (v.detach() + 0.3 * torch.randn(v.shape, generator=g)).requires_grad_(True) for k, v in base.items()}
        noise = {"eps_mu": torch.randn(data.n_targets, 1), "eps_sd": torch.randn(data.n_targets, 1)}
        if family == "MixtureNormal":
            conc = torch.ones(data.n_reps, 1, data.n_guides, 2)
            noise["pi"] = torch.distributions.Dirichlet(conc).sample()
        for what, d in (("masked", masked), ("swapped", swapped), ("full", data)):
            params = {k: v.detach().clone().requires_grad_(True) for k, v in base.items()}
            results[(at, what)] = svi.loss_and_grads(loss_fn, d, params, noise=noise)[:2]
    for at in ("initial", "moved"):
        loss, grads = results[(at, "masked")]
        loss2, grads2 = results[(at, "swapped")]
        assert np.isfinite(loss) and np.isfinite(loss2)
        for k, g in grads.items():
            assert torch.isfinite(g).all(), (at, k)
            assert torch.equal(g, grads2[k]), (at, k, (g - grads2[k]).abs().max())  # changed by exactly 0
        # (the full screen does depend on replicate 1: the check above is not vacuous)
        assert any(not torch.equal(g, results[(at, "full")][1][k]) for k, g in grads.items())
    # the loss changes by a constant only: the same difference wherever the parameters are
    d0 = results[("initial", "swapped")][0] - results[("initial", "masked")][0]
    d1 = results[("moved", "swapped")][0] - results[("moved", "masked")][0]
    # (the oracle sums its likelihood terms in the reference's float32: a constant is the same to that rounding)
    print(f"{family}: loss change through the masked replicate's counts {d0!r} at the initial point, {d1!r} moved")
    assert abs(d0 - d1) <= 1e-6 * abs(results[("moved", "masked")][0]), (d0, d1)
