"""Seed ensembles, the parts that need no GPU: the three C entry points (declared, exported, listed, null handles
rejected), combine_ensemble's moment match, the --n-seeds flag and the two added columns of the element table."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model import readwrite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("bean_hip_ensemble_supported", "bean_hip_set_members", "bean_hip_svi_run_ensemble")


@pytest.fixture(scope="module")
def lib():
    _lib.build_library()
    return _lib.load()


def test_entry_points_declared_exported_and_listed(lib):
    text = open(os.path.join(ROOT, "include", "bean_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    listed = {s[0] for s in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in bean_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in listed, f"{name} not in _lib.SYMBOLS"
    cap = int(re.search(r"#define\s+BEAN_HIP_MAX_MEMBERS\s+(\d+)", text).group(1))
    assert cap == _lib.MAX_MEMBERS >= 16
    # the shape struct keeps its layout (reserved_ included)
    assert [f[0] for f in _lib.bean_hip_shape._fields_][-3:] == ["n_sample_covariates", "reserved_", "prior_ia_total"]


def test_null_handles_are_rejected_without_a_device(lib):
    seeds = (ctypes.c_uint64 * 2)(101, 102)
    for what, call in (
        ("ensemble_supported", lambda: lib.bean_hip_ensemble_supported(None)),
        ("set_members", lambda: lib.bean_hip_set_members(None, 2)),
        ("svi_run_ensemble", lambda: lib.bean_hip_svi_run_ensemble(None, seeds, 2, 0, 1, 0, None)),
    ):
        assert call() < 0, what
        msg = lib.bean_hip_last_error().decode()
        assert what in msg and "null handle" in msg, (what, msg)


# ---------------------------------------------------------------- combine_ensemble
def _member(shift, t=5, g=7):
    base = torch.arange(t, dtype=torch.float32).reshape(t, 1)
    return {
        "mu_loc": 0.1 * base + shift,
        "mu_scale": 0.5 + 0.01 * base + 0.1 * abs(shift),
        "sd_loc": -0.2 * base + 0.5 * shift,
        "sd_scale": 0.05 + 0.02 * base,
        "alpha_pi": torch.full((g, 2), 1.0 + shift),
        "noise_loc": torch.linspace(-1, 1, g) * (1 + shift),
        "noise_scale": torch.full((g,), 0.655 + 0.1 * shift),
    }


def test_combine_one_member_is_that_member_exactly():
    from bean_amd.model.ensemble import combine_ensemble
    from bean_amd.model.run import ParamStore

    m = _member(0.3)
    store, spread = combine_ensemble([(ParamStore(m), {"loss": [1.0], "params": m})])
    assert set(store.keys()) == set(m)
    for k, v in m.items():
        assert store[k].dtype == v.dtype and torch.equal(store[k], v), k
    assert spread["n_seeds"] == 1 and torch.equal(spread["mu_seed_sd"], torch.zeros_like(m["mu_loc"]))


def test_combine_three_members_is_the_moment_match_of_their_mixture():
    from bean_amd.model.ensemble import combine_ensemble
    from bean_amd.model.run import ParamStore

    members = [_member(s) for s in (-0.4, 0.1, 0.7)]
    store, spread = combine_ensemble([ParamStore(m) for m in members])
    arr = {k: np.stack([m[k].numpy().astype(np.float64) for m in members]) for k in members[0]}
    tol = dict(rtol=4 * np.finfo(np.float64).eps, atol=4 * np.finfo(np.float64).eps)
    np.testing.assert_allclose(store["mu_loc"].numpy(), arr["mu_loc"].mean(0), **tol)
    np.testing.assert_allclose(store["mu_scale"].numpy(),
                               np.sqrt((arr["mu_scale"] ** 2).mean(0) + arr["mu_loc"].var(0)), **tol)
    np.testing.assert_allclose(store["sd_loc"].numpy(), arr["sd_loc"].mean(0), **tol)
    np.testing.assert_allclose(store["sd_scale"].numpy(),
                               np.sqrt((arr["sd_scale"] ** 2).mean(0) + arr["sd_loc"].var(0)), **tol)
    for k in ("alpha_pi", "noise_loc", "noise_scale"):
        np.testing.assert_allclose(store[k].numpy(), arr[k].mean(0), **tol)
    np.testing.assert_allclose(spread["mu_seed_sd"].numpy(), arr["mu_loc"].std(0), **tol)
    assert spread["n_seeds"] == 3 and store["mu_loc"].shape == members[0]["mu_loc"].shape
    # the between-seed spread widens the combined posterior beyond every member's own
    assert (store["mu_scale"].numpy() > arr["mu_scale"].min(0)).all()


def test_identical_members_have_no_seed_spread():
    from bean_amd.model.ensemble import combine_ensemble
    from bean_amd.model.run import ParamStore

    m = _member(0.25)
    store, spread = combine_ensemble([ParamStore({k: v.clone() for k, v in m.items()}) for _ in range(4)])
    assert torch.equal(spread["mu_seed_sd"], torch.zeros_like(spread["mu_seed_sd"]))
    np.testing.assert_allclose(store["mu_scale"].numpy(), m["mu_scale"].double().numpy(), rtol=1e-15)
    assert spread["n_seeds"] == 4


# ---------------------------------------------------------------- the flag
RUN = ["run", "sorting", "variant", "screen.h5ad"]


def test_n_seeds_flag_belongs_to_the_dispatcher_not_to_the_reference_table():
    import argparse

    from bean_amd.cli.execute import get_parser
    from bean_amd.model.parser import parse_args

    parser = get_parser()
    assert parser.parse_args(RUN).n_seeds == 1
    assert parser.parse_args(RUN + ["--n-seeds", "4"]).n_seeds == 4
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        parser.parse_args(RUN + ["--n-seeds", "0"])
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        plain.parse_args(RUN[1:] + ["--n-seeds", "4"])
    assert not hasattr(plain.parse_args(RUN[1:]), "n_seeds")


# ---------------------------------------------------------------- the tables
def _cases():
    src = open(os.path.join(GOLD, "make_readwrite_golden.py")).read()
    ns = {}
    head = src[src.index("CASES = {"):src.index("def main():")]
    exec("import numpy as np, pandas as pd, torch\n" + head, ns)
    return ns["CASES"], ns["build"]


def _write(tmp_path, sub, **extra):
    _, build = _cases()
    target, guide, P, neg, kw = build("plain", 100)
    prefix = os.path.join(str(tmp_path), sub) + "/"
    os.makedirs(prefix)
    with contextlib.redirect_stdout(io.StringIO()):
        readwrite.write_result_table(target.copy(), guide.copy(), P, "M", prefix=prefix, **kw, **extra)
    return prefix, P


def test_tables_without_the_keywords_are_the_bytes_written_before(tmp_path):
    """tests/golden/ensemble_plain_*.csv: write_result_table's files for the `plain` case of
    make_readwrite_golden.py, written by the code as it was before the keywords existed."""
    prefix, _ = _write(tmp_path, "none")
    prefix2, _ = _write(tmp_path, "explicit", seed_sd=None, n_seeds=None)
    for kind in ("element", "sgRNA"):
        want = open(os.path.join(GOLD, f"ensemble_plain_{kind}.csv"), "rb").read()
        assert open(prefix + f"bean_{kind}_result.M.csv", "rb").read() == want, kind
        assert open(prefix2 + f"bean_{kind}_result.M.csv", "rb").read() == want, kind


def test_tables_with_seed_spread_have_the_two_columns_in_row_order(tmp_path):
    _, build = _cases()
    n = len(build("plain", 100)[0])
    sd = np.linspace(0.01, 0.2, n)
    prefix, P = _write(tmp_path, "seeded", seed_sd=torch.as_tensor(sd).reshape(n, 1), n_seeds=5)
    base, _ = _write(tmp_path, "base")
    got = pd.read_csv(prefix + "bean_element_result.M.csv")
    ref = pd.read_csv(base + "bean_element_result.M.csv")
    assert {"mu_seed_sd", "n_seeds"} <= set(got.columns) and not {"mu_seed_sd", "n_seeds"} & set(ref.columns)
    assert [c for c in got.columns if c not in ("mu_seed_sd", "n_seeds")] == list(ref.columns)
    pd.testing.assert_frame_equal(got[list(ref.columns)], ref)  # same rows, same (sorted by |z|) order
    assert (got["n_seeds"] == 5).all()
    # row i of the written table is target got.iloc[i, 0] of the unsorted one: its spread travels with it
    np.testing.assert_allclose(got["mu_seed_sd"].values, sd[got.iloc[:, 0].values], rtol=1e-12)
    assert not np.array_equal(got.iloc[:, 0].values, np.arange(n))  # (the table IS reordered)
    assert open(prefix + "bean_sgRNA_result.M.csv", "rb").read() == open(base + "bean_sgRNA_result.M.csv", "rb").read()
    with pytest.raises(ValueError, match="go together"):
        _write(tmp_path, "half", seed_sd=sd)
