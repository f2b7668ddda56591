"""The count simulators against recorded draws (tests/golden/simulator_draws.npz, written by
tests/golden/make_simulator_golden.py): every simulator entry point - bean_hip_simulate, _members, _design, _power,
_simulate_survival and _survival_members - draws the same small screens again from their seeds, and every array must be
the recorded one bit for bit: counts, floored concentrations, and the pi and Dirichlet-over-all-guides draws the single
draw dumps.  The other simulator tests compare the simulators with each other or with the law; this one pins the bits,
so a change to the sampler that reaches one kernel and not another, or all of them alike, shows.  The screens reach the
lone last bin of the gamma pairs (odd B), the log branch (a0 = 1e-3), a second tile with invalid lanes, masks, the
survival members' u_g redraw and the injected baseline.  A difference means a changed expression: restore it, do not
record again.  -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_simulator_golden as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with np.load(gen.OUT) as f:
        return {k: f[k] for k in f.files}


def test_the_file_holds_the_cases_and_nothing_else(recorded):
    assert os.path.getsize(gen.OUT) < gen.MAX_BYTES
    assert set(recorded) == {f"{name}/{label}/{part}" for name, label in gen.cases() for part in ("counts", "float64")}


@pytest.mark.parametrize("name,label", gen.cases(), ids=[f"{n}-{lab}" for n, lab in gen.cases()])
def test_draws_are_the_recorded_ones(recorded, name, label):
    got = gen.record(name, label)
    want = gen.unpack({part: recorded[f"{name}/{label}/{part}"] for part in ("counts", "float64")}, got)
    assert set(got) == set(want)
    calls = {k.split("/")[0] for k in got}
    assert calls == ({"simulate", "noise", "members"} | ({"members-eps_u"} if label != "Normal" else set())
                     if name.startswith("survival") else
                     {"simulate", "members", "design", "power"} | ({"noise"} if label != "Normal" else set()))
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), (name, label, k, int((got[k] != want[k]).sum()), "of", got[k].numel())
