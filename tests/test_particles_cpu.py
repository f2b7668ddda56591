"""Multi-particle SVI, the parts that need no GPU: the two C entry points (declared, listed, exported by all four
libraries, null handles rejected), the particle seed rule, the --num-particles flag and its refusals at the parser and in
cli/run.py, and the float64 mean the engine's defining loop forms."""
import argparse
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bean_hip_set_particles", "bean_hip_svi_run_particles")
RUN = ["run", "sorting", "variant", "screen.h5ad"]


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
    # the shape struct keeps its layout
    assert [f[0] for f in _lib.bean_hip_shape._fields_][-3:] == ["n_sample_covariates", "reserved_", "prior_ia_total"]


def test_null_handles_are_rejected_without_a_device():
    _lib.build_library()
    lib = _lib.load()
    seeds = (ctypes.c_uint64 * 2)(101, 102)
    for what, call in (
        ("set_particles", lambda: lib.bean_hip_set_particles(None, 2)),
        ("svi_run_particles", lambda: lib.bean_hip_svi_run_particles(None, seeds, 2, 0, 1, 0, None)),
    ):
        assert call() < 0, what
        msg = lib.bean_hip_last_error().decode()
        assert what in msg and "null handle" in msg, (what, msg)


def test_particle_seeds_rule():
    from bean_amd.model import run as model_run
    from bean_amd.model.jackknife import particle_seeds

    assert model_run.particle_seeds is particle_seeds
    assert particle_seeds(101, 1) == [101]
    assert particle_seeds(101, 4) == [101, 101 + 1_000_003, 101 + 2_000_006, 101 + 3_000_009]
    assert particle_seeds(7, 64)[63] == 7 + 1_000_003 * 63
    assert all(isinstance(s, int) for s in particle_seeds(np.int64(5), np.int64(3)))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="n_particles"):
            particle_seeds(101, bad)


# ---------------------------------------------------------------- the flag
def test_flag_belongs_to_the_dispatcher_and_defaults_to_one():
    from bean_amd.cli.execute import get_parser
    from bean_amd.model.parser import parse_args

    parser = get_parser()
    assert parser.parse_args(RUN).num_particles == 1
    assert parser.parse_args(RUN + ["--num-particles", "8"]).num_particles == 8
    for bad in ("0", "-2", "two"):
        with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(io.StringIO()):
            parser.parse_args(RUN + ["--num-particles", bad])
        assert exc.value.code == 2
    plain = parse_args(argparse.ArgumentParser(prog="bean run"))
    assert not hasattr(plain.parse_args(RUN[1:]), "num_particles")
    help_text = parser._subparsers._group_actions[0].choices["run"].format_help()
    assert "--num-particles" in help_text and "stays at one particle" in " ".join(help_text.split())


ONE_FIT = "--num-particles averages draws inside one fit and does not combine with {}: particles inside member sets are not batched."
REFUSALS = [
    (["--n-seeds", "2"], ONE_FIT.format("--n-seeds")),
    (["--jackknife-replicates"], ONE_FIT.format("--jackknife-replicates")),
    (["--jackknife-guides"], ONE_FIT.format("--jackknife-guides")),
    (["--jackknife-samples"], ONE_FIT.format("--jackknife-samples")),
    (["--jackknife-conditions"], ONE_FIT.format("--jackknife-conditions")),
    (["--load-existing"], "--num-particles needs the fit itself and does not combine with --load-existing."),
]


@pytest.mark.parametrize("extra,sentence", REFUSALS, ids=[r[0][0] for r in REFUSALS])
def test_refused_combinations_at_the_parser_and_in_cli_run(extra, sentence):
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser, main

    argv = RUN + ["--num-particles", "2"] + extra
    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2
    assert sentence in " ".join(err.getvalue().split())
    args = get_parser().parse_args(argv)
    with pytest.raises(ValueError) as exc:
        cli_run.particle_count(args)
    assert str(exc.value) == sentence
    # one particle combines with all of them
    assert cli_run.particle_count(get_parser().parse_args(RUN + extra)) == 1


def test_more_particles_than_members_are_refused():
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser, main

    sentence = f"--num-particles is at most {_lib.MAX_MEMBERS}."
    argv = RUN + ["--num-particles", str(_lib.MAX_MEMBERS + 1)]
    err = io.StringIO()
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stderr(err):
        main(argv)
    assert exc.value.code == 2 and sentence in " ".join(err.getvalue().split())
    with pytest.raises(ValueError) as exc:
        cli_run.particle_count(get_parser().parse_args(argv))
    assert str(exc.value) == sentence
    assert cli_run.particle_count(get_parser().parse_args(RUN + ["--num-particles", str(_lib.MAX_MEMBERS)])) == _lib.MAX_MEMBERS
    assert cli_run.particle_count(argparse.Namespace()) == 1  # (callers that build their own namespace)


def test_run_inference_refuses_a_particle_count_out_of_range():
    from bean_amd.model.run import run_inference

    for bad in (0, -1, _lib.MAX_MEMBERS + 1):
        with pytest.raises(ValueError, match="num_particles must be in"):
            run_inference(None, None, None, num_particles=bad)


# ---------------------------------------------------------------- the mean of the defining loop
def test_particle_mean_adds_in_particle_order_in_float64():
    from bean_amd.engine import particle_mean

    one, tiny = np.float32(1.0), np.float32(2.0 ** -53)
    t = lambda *v: [torch.tensor([x], dtype=torch.float32) for x in v]  # noqa: E731
    # (1 + 2^-53) is a tie in float64 and rounds to 1: in particle order the small value is lost ...
    got = particle_mean(t(one, tiny, -one))
    assert got.dtype == torch.float32 and got.item() == 0.0
    # ... while another order keeps it
    other = particle_mean(t(one, -one, tiny))
    assert other.item() == float(np.float32(2.0 ** -53 * (1.0 / 3.0))) != 0.0
    # the accumulator is float64: in float32 the first two of these would already have lost the 1
    got = particle_mean(t(np.float32(2.0 ** 25), one, np.float32(-2.0 ** 25)))
    assert got.item() == float(np.float32(1.0 * (1.0 / 3.0)))
    # one multiply by 1 / P, not a division: 1 / 3 is rounded before it meets the sum
    assert particle_mean(t(one, one, one)).item() == float(np.float32(3.0 * (1.0 / 3.0)))
    third = 1.0 / 3.0
    for s in (5.0, 7.0, 49.0):
        assert particle_mean(t(np.float32(s), np.float32(0.0), np.float32(0.0))).item() == float(np.float32(s * third))
    # the inputs are left alone, whatever their dtype
    vals = [torch.tensor([0.5, 1.5], dtype=torch.float64), torch.tensor([1.0, 2.5], dtype=torch.float64)]
    keep = [v.clone() for v in vals]
    out = particle_mean(vals)
    assert out.dtype == torch.float64 and torch.equal(out, torch.tensor([0.75, 2.0], dtype=torch.float64))
    assert all(torch.equal(a, b) for a, b in zip(vals, keep))
    # a NaN in any particle reaches the mean
    assert torch.isnan(particle_mean(t(one, np.float32("nan"), one))).all()


@pytest.mark.parametrize("P", [1, 2, 4, 8, 16, 64])
def test_particle_mean_is_exact_for_a_power_of_two(P):
    from bean_amd.engine import particle_mean

    g = torch.Generator().manual_seed(P)
    # multiples of 2^-10 below 2^10 in size: every partial sum is exact in float64, and so is the division by P
    ints = torch.randint(-(2 ** 20), 2 ** 20, (P, 257), generator=g)
    vals = (ints.double() / 1024.0).to(torch.float32)
    assert torch.equal(vals.double() * 1024.0, ints.double())
    want = (ints.sum(0).double() / 1024.0 / P).to(torch.float32)
    got = particle_mean(list(vals.unbind(0)))
    assert torch.equal(got, want)
    if P == 1:
        assert torch.equal(got, vals[0])
