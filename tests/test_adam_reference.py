"""The yardstick of tests/test_gpu_adam.py, checked without a GPU: a float32 evaluation of the correct update stays
inside the bounds of tests/adam_reference.py on every case, the same bounds reject each of seven planted errors on at
least 1 % of the cases at every step count, and the float64 reference is the oracle's (torch, float32) ClippedAdam."""
import numpy as np
import pytest
import torch

import adam_reference as ar
from oracle import svi

F32 = np.float32
N_CASES = 200_000
STEPS = (1, 2, 10, 1000, 2000, 5000)
LR0, LRD = 0.01, ar.lrd_of(0.1, 2000)   # run_inference's defaults


@pytest.fixture(scope="module")
def cases():
    return ar.adam_cases(N_CASES, seed=1)


def _fma(a, b, c):
    """float32 fma as a float64 product (exact: 24 + 24 bits) plus add, rounded once more to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def emulate(p, m, v, g, ss, *, clip=10.0, b2=0.999, a2=0.001, eps=1e-8, eps_inside=False):
    """adam_update (csrc/bean_kernels.hpp) in numpy float32, rounding by rounding; the keywords plant the mutants."""
    with np.errstate(all="ignore"):
        gc = g if clip is None else np.clip(g, F32(-clip), F32(clip))
        m9 = m * F32(0.9)
        m1 = _fma(gc, np.full_like(gc, F32(0.1)), m9)
        v9 = v * F32(b2)
        g2 = gc * gc
        v1 = _fma(g2, np.full_like(g2, F32(a2)), v9)
        denom = np.sqrt(v1 + F32(eps)) if eps_inside else np.sqrt(v1) + F32(eps)
        q = m1 / denom
        p1 = _fma(np.full_like(q, -F32(ss)), q, p)
    assert all(a.dtype == F32 for a in (m1, v1, p1))
    return p1, m1, v1


def _bad_fraction(got, p, m, v, g, t):
    ref = ar.clipped_adam_ref(p, m, v, g, t, LR0, LRD)
    bounds = ar.adam_bounds(p, m, v, g, t, LR0, LRD)
    # (the reference and the bounds are finite on every case: +-inf gradients clamp)
    assert all(np.isfinite(a).all() for a in ref + bounds)
    bad = np.zeros(p.shape, dtype=bool)
    worst = []
    for got_x, ref_x, b_x in zip(got, ref, (bounds[2], bounds[0], bounds[1])):
        bad_x, w = ar.violations(got_x, ref_x, b_x)
        bad |= bad_x
        worst.append(w)
    return bad.mean(), worst


def test_constants_are_the_kernels_literals():
    assert F32(1 - 0.9) == F32(0.1) and F32(1 - 0.999) == F32(0.001)
    assert ar.A1 == float(F32(0.1)) and ar.A2 == float(F32(0.001))
    assert ar.B1 == float(F32(0.9)) and ar.B2 == float(F32(0.999)) and ar.EPS == float(F32(1e-8))


def test_case_set_holds_the_grid_and_both_regimes(cases):
    p, m, v, g = cases
    assert p.size == N_CASES > ar.N_GRID == 23 * 6 * 5 * 5
    for grid, col in ((ar.GRID_P, p), (ar.GRID_M, m), (ar.GRID_V, v), (ar.GRID_G, g)):
        assert set(np.asarray(grid, dtype=F32).tolist()) <= set(col[: ar.N_GRID].tolist())
    assert (np.abs(g) <= 10).sum() > N_CASES // 10 and (np.abs(g) > 10).sum() > N_CASES // 10
    assert np.isinf(g).any() and not np.isnan(g).any()
    small = ar.adam_cases(130, seed=2)
    assert all(a.shape == (130,) and a.dtype == F32 for a in small)


@pytest.mark.parametrize("t", STEPS)
def test_float32_update_is_within_the_bounds(cases, t):
    p, m, v, g = cases
    frac, worst = _bad_fraction(emulate(p, m, v, g, ar.step_size(t, LR0, LRD)), p, m, v, g, t)
    print(f"t={t}: worst |err| / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert frac == 0.0, (t, frac, worst)


MUTANTS = {
    "no clip": lambda t: (ar.step_size(t, LR0, LRD), dict(clip=None)),
    "clip at 11": lambda t: (ar.step_size(t, LR0, LRD), dict(clip=11.0)),
    "beta2 = 0.99": lambda t: (ar.step_size(t, LR0, LRD), dict(b2=0.99, a2=0.01)),
    "eps inside the square root": lambda t: (ar.step_size(t, LR0, LRD), dict(eps_inside=True)),
    "eps = 1e-7": lambda t: (ar.step_size(t, LR0, LRD), dict(eps=1e-7)),
    "no bias correction": lambda t: (LR0 * LRD ** t, {}),
    "t + 1 instead of t": lambda t: (ar.step_size(t + 1, LR0, LRD), {}),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_bounds_reject_the_mutant(cases, name):
    p, m, v, g = cases
    for t in STEPS:
        ss, kw = MUTANTS[name](t)
        frac, _ = _bad_fraction(emulate(p, m, v, g, ss, **kw), p, m, v, g, t)
        print(f"{name}, t={t}: outside the bounds on {100 * frac:.1f} % of the cases")
        assert frac >= 0.01, (name, t, frac)


def test_reference_is_the_oracles_clipped_adam(cases):
    """oracle.svi.ClippedAdam (torch, float32) at t = 1 with the cases' moments written into its state."""
    p, m, v, g = cases
    params = {"x": torch.from_numpy(p.copy())}
    opt = svi.ClippedAdam(params, lr=LR0, lrd=LRD)
    opt.state["x"]["m"].copy_(torch.from_numpy(m))
    opt.state["x"]["v"].copy_(torch.from_numpy(v))
    params["x"].grad = torch.from_numpy(g.copy())
    opt.step()
    got = (params["x"].numpy(), opt.state["x"]["m"].numpy(), opt.state["x"]["v"].numpy())
    assert opt.state["x"]["step"] == 1 and all(a.dtype == F32 for a in got)
    frac, worst = _bad_fraction(got, p, m, v, g, 1)
    print(f"torch float32 against the reference: worst |err| / bound  p {worst[0]:.3f}  m {worst[1]:.3f}  v {worst[2]:.3f}")
    assert frac == 0.0, (frac, worst)


def test_nan_gradient_propagates_in_the_reference_and_inf_clamps():
    one = np.ones(3, dtype=F32)
    g = np.array([np.nan, np.inf, -np.inf], dtype=F32)
    p1, m1, v1 = ar.clipped_adam_ref(one, one, one, g, 3, LR0, LRD)
    ten = ar.clipped_adam_ref(one, one, one, np.array([0, 10, -10], dtype=F32), 3, LR0, LRD)
    assert np.isnan([p1[0], m1[0], v1[0]]).all()
    for a, b in zip((p1, m1, v1), ten):
        assert np.array_equal(a[1:], b[1:])
    # ... and torch's clamp_, which Pyro calls, does the same
    t = torch.tensor([float("nan"), float("inf"), -float("inf")]).clamp_(-10, 10)
    assert torch.isnan(t[0]) and t[1] == 10 and t[2] == -10
