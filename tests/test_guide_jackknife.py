"""Guide jackknife, the parts that need no GPU: leave_out_guides, the positions and the members' masks, the summary on
hand-computed numbers, the --jackknife-guides flag and its refusals, the added columns of the two tables and - through
the CPU oracle - the independence of the targets that lets one fit with position j masked everywhere stand for every
target's own leave-one-guide-out fit."""
import copy
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.model import readwrite
from bean_amd.model.jackknife import (guide_jackknife_summary, guide_member_masks, guide_positions, leave_out_guides)
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen
from oracle import elbo, svi

ELEMENT_COLUMNS = ["mu_gjk_se", "mu_gjk_max_shift", "mu_gjk_max_shift_guide", "n_gjk"]
GUIDE_COLUMN = "mu_shift_left_out"


@pytest.fixture(scope="module")
def screen():
    """200 guides x 3 replicates, 7 guides per target: 28 targets of 7 and a last one of 4.  Never modified."""
    return make_sorting_variant_screen(200, 3, seed=9, guides_per_target=7, mask_fraction=0.05)


# ---------------------------------------------------------------- leave_out_guides
def test_leave_out_guides_changes_the_named_columns_and_nothing_else(screen):
    data = screen
    before = {k: v.clone() for k, v in data.tensor_items()}
    gone = [3, 64, 199]
    assert all(bool(data.repguide_mask[:, g].any()) for g in gone)
    out = leave_out_guides(data, gone)
    for k, v in data.tensor_items():  # the original is not modified
        assert torch.equal(v, before[k]), k
    assert set(vars(out)) == set(vars(data))
    for k, v in vars(data).items():
        if k == "repguide_mask":
            continue
        w = getattr(out, k)
        assert w is v or (isinstance(v, torch.Tensor) and torch.equal(v, w)), k
    a, b = data.repguide_mask, out.repguide_mask
    assert a.dtype == b.dtype and a.shape == b.shape and a.data_ptr() != b.data_ptr()
    assert not bool(b[:, gone].any())
    rest = [g for g in range(data.n_guides) if g not in gone]
    assert torch.equal(a[:, rest], b[:, rest])
    assert torch.equal(leave_out_guides(data, 64).repguide_mask[:, 65:], a[:, 65:])  # one index, a tensor of indices
    assert torch.equal(leave_out_guides(data, torch.tensor(gone)).repguide_mask, b)
    for bad in (200, -1, [3, 200]):
        with pytest.raises(ValueError, match="of a screen with 200 guides"):
            leave_out_guides(data, bad)


# ---------------------------------------------------------------- positions / member masks
def test_positions_and_member_masks(screen):
    data = screen
    assert data.target_lengths.tolist() == [7] * 28 + [4]
    positions, included = guide_positions(data)
    assert positions == list(range(7))
    assert included.shape == (29, 7) and included.dtype == torch.bool
    alive = data.repguide_mask.any(0)
    assert bool(alive.all())  # (no guide of this screen is masked in all three replicates)
    assert bool(included[:28].all()) and bool(included[-1, :4].all()) and not bool(included[-1, 4:].any())
    rg, sm = guide_member_masks(data, positions)
    assert rg.shape == (8, 3, 200) and rg.dtype == torch.bool and sm.shape == (8, 3, data.n_condits)
    assert torch.equal(rg[0], data.repguide_mask)
    off = data.target_offsets
    for j in positions:
        gone = [int(off[t]) + j for t in range(29) if j < int(data.target_lengths[t])]
        assert len(gone) == (29 if j < 4 else 28)
        assert torch.equal(rg[1 + j], leave_out_guides(data, gone).repguide_mask), j
        assert torch.equal(sm[1 + j], data.sample_mask) and sm.dtype == data.sample_mask.dtype
    # a subset of the positions, in the caller's order
    rg2, _ = guide_member_masks(data, [5, 0])
    assert torch.equal(rg2[1], rg[6]) and torch.equal(rg2[2], rg[1])


def test_a_guide_masked_in_every_replicate_is_not_included(screen):
    g = 7 * 4 + 2  # position 2 of target 4
    data = leave_out_guides(screen, g)
    positions, included = guide_positions(data)
    ref = guide_positions(screen)[1]
    assert positions == list(range(7))
    assert not bool(included[4, 2]) and int(included[4].sum()) == 6
    ref[4, 2] = False
    assert torch.equal(included, ref)
    # and it does not count in n_t
    fits = [{"mu_loc": torch.full((29, 1), float(j))} for j in positions]
    out = guide_jackknife_summary({"mu_loc": torch.zeros(29, 1)}, fits, positions, included, data, [f"g{i}" for i in range(200)])
    assert out["n_gjk"].tolist() == [7] * 4 + [6] + [7] * 23 + [4]
    assert np.isnan(float(out["mu_shift_left_out"][g])) and float(out["mu_shift_left_out"][g + 1]) == 3.0


def test_position_cap(screen):
    with pytest.raises(ValueError, match="at least one guide"):
        guide_positions(screen, max_positions=3)  # every target here is longer: nothing is included
    positions, included = guide_positions(screen, max_positions=4)  # the short last target alone
    assert positions == [0, 1, 2, 3] and not bool(included[:28].any()) and bool(included[28].all())
    assert guide_positions(screen, max_positions=63)[0] == list(range(7))
    for bad in (64, 0):
        with pytest.raises(ValueError, match="1 to 63 positions"):
            guide_positions(screen, max_positions=bad)


# ---------------------------------------------------------------- summary
def _fit(mu):
    return {"mu_loc": torch.tensor(mu, dtype=torch.float32).reshape(-1, 1)}


def test_summary_matches_hand_computed_numbers():
    """Four targets of 3, 2, 1 and 3 guides (guides g0-g2, g3-g4, g5, g6-g8), three positions.

    Target 0: m = (1, 2, 6), mean 3, sum of squares 14, se = sqrt(2/3 * 14); full 2.5: shifts -1.5, -0.5, 3.5 -> g2.
    Target 1 (ragged: no position 2): m = (1, 3.5), mean 2.25, se = sqrt(1/2 * 2 * 1.25^2) = 1.25; full 2: shifts
    -1, 1.5 -> g4.  The member for position 2 holds 99 for it: not read.
    Target 2: one guide, n = 1: NaN, no name; its guide's shift 0.5 - 0.25 is still reported.
    Target 3: position 1 already masked, m = (0, -3): mean -1.5, se = sqrt(1/2 * 2 * 1.5^2) = 1.5; full 0.25: shifts
    -0.25, -3.25 -> g8 (position 2).  The member for position 1 holds 50 for it: not read."""
    data = SimpleNamespace(target_offsets=torch.tensor([0, 3, 5, 6, 9]), n_guides=9)
    included = torch.tensor([[1, 1, 1], [1, 1, 0], [1, 0, 0], [1, 0, 1]], dtype=torch.bool)
    full = _fit([2.5, 2.0, 0.25, 0.25])
    loo = [_fit([1.0, 1.0, 0.5, 0.0]), _fit([2.0, 3.5, 7.0, 50.0]), (_fit([6.0, 99.0, 7.0, -3.0]), {"loss": [], "params": {}})]
    names = [f"g{i}" for i in range(9)]
    out = guide_jackknife_summary(full, loo, [0, 1, 2], included, data, names)
    assert set(out) == set(ELEMENT_COLUMNS) | {GUIDE_COLUMN}
    for k in ("mu_gjk_se", "mu_gjk_max_shift", GUIDE_COLUMN):
        assert out[k].dtype == torch.float64, k
    se, shift = out["mu_gjk_se"].numpy(), out["mu_gjk_max_shift"].numpy()
    assert se.shape == shift.shape == (4,)
    np.testing.assert_allclose(se[[0, 1, 3]], [np.sqrt(2.0 / 3.0 * 14.0), 1.25, 1.5], rtol=1e-15)
    np.testing.assert_allclose(shift[[0, 1, 3]], [3.5, 1.5, 3.25], rtol=1e-15)
    assert np.isnan(se[2]) and np.isnan(shift[2])
    assert out["mu_gjk_max_shift_guide"] == ["g2", "g4", "", "g8"]
    assert out["n_gjk"].tolist() == [3, 2, 1, 2]
    per_guide = out[GUIDE_COLUMN].numpy()
    np.testing.assert_allclose(per_guide[[0, 1, 2, 3, 4, 5, 6, 8]], [-1.5, -0.5, 3.5, -1.0, 1.5, 0.25, -0.25, -3.25], rtol=1e-15)
    assert np.isnan(per_guide[7]) and np.isfinite(per_guide).sum() == 8
    with pytest.raises(ValueError, match="one fit per position"):
        guide_jackknife_summary(full, loo[:2], [0, 1, 2], included, data, names)


# ---------------------------------------------------------------- flag
RUN = ["run", "sorting", "variant", "screen.h5ad"]


def test_flag_parses_and_the_four_refusals(capsys):
    from bean_amd.cli.execute import get_parser
    from bean_amd.cli.execute import main as bean_main
    from bean_amd.model.parser import parse_args as reference_table

    parser = get_parser()
    plain = parser.parse_args(RUN)
    assert plain.jackknife_guides is False and plain.jackknife_guides_max == 63
    got = parser.parse_args(RUN + ["--jackknife-guides", "--jackknife-guides-max", "12"])
    assert got.jackknife_guides is True and got.jackknife_guides_max == 12
    assert parser.parse_args(RUN + ["--jackknife-guides", "--n-seeds", "1"]).n_seeds == 1
    refused = [
        (RUN + ["--jackknife-guides", "--n-seeds", "2"], "--n-seeds"),
        (RUN + ["--jackknife-guides", "--jackknife-replicates"], "--jackknife-replicates"),
        (RUN + ["--jackknife-guides", "--load-existing"], "--load-existing"),
        (["run", "sorting", "tiling", "screen.h5ad", "--jackknife-guides"], "tiling"),
        (RUN + ["--jackknife-guides", "--jackknife-guides-max", "64"], "at most 63"),
    ]
    for argv, word in refused:
        with pytest.raises(SystemExit) as exc:
            bean_main(argv)  # refused before anything is read or fitted
        assert exc.value.code == 2, argv
        msg = capsys.readouterr().err
        assert "--jackknife-guides" in msg and word in msg, (argv, msg)
    with pytest.raises(SystemExit):
        reference_table().parse_args(RUN[1:] + ["--jackknife-guides"])  # not in the reference's flag table


def test_cli_run_refuses_the_combinations_too(monkeypatch):
    """`cli.run.main` called directly (not through the parser) raises on the same four."""
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    class Stop(Exception):
        pass

    def no_fit(*a, **k):
        raise Stop

    base = get_parser().parse_args(RUN + ["--jackknife-guides"])
    for change, word in ((dict(n_seeds=2), "--n-seeds"), (dict(jackknife_replicates=True), "--jackknife-replicates"),
                         (dict(load_existing=True), "--load-existing"), (dict(library_design="tiling"), "tiling")):
        args = copy.copy(base)
        for k, v in change.items():
            setattr(args, k, v)
        with pytest.raises(ValueError, match=word):
            cli_run.check_guide_jackknife_switches(args)
    cli_run.check_guide_jackknife_switches(base)


# ---------------------------------------------------------------- tables
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


def test_tables_gain_exactly_four_element_columns_and_one_guide_column(tmp_path):
    ref_prefix, n = _write(tmp_path, "plain")
    none_prefix, _ = _write(tmp_path, "none", guide_jackknife=None)
    el_name, sg_name = "bean_element_result.Normal.csv", "bean_sgRNA_result.Normal.csv"
    for name in (el_name, sg_name):  # None: byte for byte the tables of today
        assert open(none_prefix + name, "rb").read() == open(ref_prefix + name, "rb").read()
    se = torch.linspace(0, 1, n, dtype=torch.float64)
    se[5] = float("nan")
    per_guide = torch.linspace(-1, 1, 3 * n, dtype=torch.float64)
    per_guide[7] = float("nan")
    gj = {"mu_gjk_se": se, "mu_gjk_max_shift": torch.linspace(1, 2, n, dtype=torch.float64),
          "mu_gjk_max_shift_guide": [f"g{3 * i + i % 3}" for i in range(n)],
          "n_gjk": torch.tensor([3] * (n - 1) + [1]), GUIDE_COLUMN: per_guide}
    prefix, _ = _write(tmp_path, "gjk", guide_jackknife=gj)
    ref = pd.read_csv(ref_prefix + el_name, float_precision="round_trip")
    got = pd.read_csv(prefix + el_name, float_precision="round_trip")
    assert [c for c in got.columns if c not in ref.columns] == ELEMENT_COLUMNS
    assert [c for c in got.columns if c not in ELEMENT_COLUMNS] == list(ref.columns)
    pd.testing.assert_frame_equal(got.drop(columns=ELEMENT_COLUMNS), ref, check_exact=True)
    by_target = got.set_index("target")
    for i in (0, 7, n - 1):
        row = by_target.loc[f"t{i}"]
        assert row["mu_gjk_se"] == float(se[i]) and row["mu_gjk_max_shift"] == float(gj["mu_gjk_max_shift"][i])
        assert row["mu_gjk_max_shift_guide"] == f"g{3 * i + i % 3}" and row["n_gjk"] == (1 if i == n - 1 else 3)
    assert np.isnan(by_target.loc["t5", "mu_gjk_se"])
    assert pd.api.types.is_integer_dtype(got["n_gjk"])
    ref_sg = pd.read_csv(ref_prefix + sg_name, float_precision="round_trip")
    got_sg = pd.read_csv(prefix + sg_name, float_precision="round_trip")
    assert list(got_sg.columns) == list(ref_sg.columns) + [GUIDE_COLUMN]
    pd.testing.assert_frame_equal(got_sg.drop(columns=[GUIDE_COLUMN]), ref_sg, check_exact=True)
    np.testing.assert_array_equal(got_sg[GUIDE_COLUMN].values, per_guide.numpy())
    with pytest.raises(ValueError, match="entries for 40 targets"):
        _write(tmp_path, "bad", guide_jackknife=dict(gj, mu_gjk_se=se[:-1]))
    with pytest.raises(ValueError, match="entries for 120 guides"):
        _write(tmp_path, "bad2", guide_jackknife=dict(gj, **{GUIDE_COLUMN: per_guide[:-1]}))


# ---------------------------------------------------------------- the targets are independent (CPU oracle)
def _other_counts(data, guides, seed):
    """The screen with the counts of `guides` (all three observed sites) replaced by other counts."""
    g = torch.Generator().manual_seed(seed)
    out = copy.copy(data)
    for name, axis in (("X", 2), ("X_masked", 2), ("X_bcmatch", 2), ("X_bcmatch_masked", 2), ("allele_counts_control", 2)):
        v = getattr(data, name).clone()
        index = [slice(None)] * v.dim()
        index[axis] = guides
        v[tuple(index)] = torch.randint(0, 400, v[tuple(index)].shape, generator=g).to(v.dtype)
        setattr(out, name, v)
    return out


PER_TARGET = ("mu_loc", "mu_scale", "sd_loc", "sd_scale")
PER_GUIDE = ("alpha_pi", "noise_loc", "noise_scale")


def _rows_of(data, t):
    """{parameter kind: rows} of target t: its own row of the per-target parameters, its guides' of the per-guide ones."""
    off = data.target_offsets
    return {"target": [t], "guide": list(range(int(off[t]), int(off[t + 1])))}


def _pick(grads, rows):
    out = {}
    for k, g in grads.items():
        assert k in PER_TARGET or k in PER_GUIDE, f"{k}: a parameter that belongs to no target would couple them"
        out[k] = g[rows["target" if k in PER_TARGET else "guide"]]
    return out


@pytest.mark.parametrize("family,loss_fn", [("MixtureNormal", elbo.mixture_normal_loss), ("Normal", elbo.normal_loss)])
def test_position_j_everywhere_is_every_targets_own_single_guide_fit_in_the_oracle(family, loss_fn, screen):
    data = screen
    T, j, t = data.n_targets, 1, 3
    off = data.target_offsets
    everywhere = [int(off[u]) + j for u in range(T)]
    one = int(off[t]) + j
    assert bool(data.repguide_mask[:, one].any())
    screens = {"full": data, "everywhere": leave_out_guides(data, everywhere), "one": leave_out_guides(data, one)}
    screens["swapped"] = _other_counts(screens["everywhere"], everywhere, seed=4)
    assert not torch.equal(screens["swapped"].X_masked, screens["everywhere"].X_masked)
    mine = _rows_of(data, t)
    others = {"target": [u for u in range(T) if u != t], "guide": [g for g in range(data.n_guides) if g not in mine["guide"]]}
    for at in ("initial", "moved"):
        torch.manual_seed(7)
        base = elbo.init_params(family, data)
        if at == "moved":
            g = torch.Generator().manual_seed(8)
            base = {k: (v.detach() + 0.3 * torch.randn(v.shape, generator=g)).requires_grad_(True) for k, v in base.items()}
        noise = {"eps_mu": torch.randn(T, 1), "eps_sd": torch.randn(T, 1)}
        if family == "MixtureNormal":
            noise["pi"] = torch.distributions.Dirichlet(torch.ones(data.n_reps, 1, data.n_guides, 2)).sample()
        grads = {}
        for what, d in screens.items():
            params = {k: v.detach().clone().requires_grad_(True) for k, v in base.items()}
            loss, grads[what] = svi.loss_and_grads(loss_fn, d, params, noise=noise)[:2]
            assert np.isfinite(loss), (at, what)
        for k, g in grads["everywhere"].items():
            assert torch.isfinite(g).all(), (at, k)
            # the masked guides' counts change every gradient by exactly 0
            assert torch.equal(g, grads["swapped"][k]), (at, k, (g - grads["swapped"][k]).abs().max())
        a, b = _pick(grads["everywhere"], mine), _pick(grads["one"], mine)
        for k in a:  # "position j everywhere" is "only guide (t, j)" on target t's rows
            assert torch.equal(a[k], b[k]), (at, k, (a[k] - b[k]).abs().max())
        a, b = _pick(grads["one"], others), _pick(grads["full"], others)
        for k in a:  # masking one guide leaves all other targets' rows those of the unmasked screen
            assert torch.equal(a[k], b[k]), (at, k, (a[k] - b[k]).abs().max())
        # (the checks are not vacuous: target t does feel its guide, the other targets feel theirs)
        assert not torch.equal(_pick(grads["one"], mine)["mu_loc"], _pick(grads["full"], mine)["mu_loc"]), at
        assert not torch.equal(_pick(grads["everywhere"], others)["mu_loc"], _pick(grads["full"], others)["mu_loc"]), at
