"""ClippedAdam on the GPU, element by element: k_adam (bean_hip_adam) against the float64 reference of
tests/adam_reference.py under its per-element rounding bounds (tests/test_adam_reference.py shows what those bounds
accept and reject), over the input grid, at early and late update counts and other schedules; non-finite gradients;
the rejected t = 0; and every fused stepper started LATE in the schedule against the loop
{elbo_grad(step=s); adam(s + 1)}, bit for bit - each of them computes the step size of update s + 1 in a place of its
own.  -m gpu."""
import numpy as np
import pytest
import torch

import adam_reference as ar
import bean_amd  # noqa: F401
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                              make_survival_variant_screen)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 9


# ------------------------------------------------------------------ k_adam against the reference
class _Bound:
    """An engine whose bound tensors (parameters, moments, gradients: caller-owned) are filled with the cases."""

    def __init__(self, family, data, **kw):
        from bean_amd import engine

        self.eng = engine.HipSVI(family, data.to(DEV), **kw)
        self.lr0, self.lrd = self.eng.initial_lr, ar.lrd_of(kw.get("gamma", 0.1), self.eng.num_steps)
        assert self.lrd == self.eng.lrd
        self.cases = {name: ar.adam_cases(t.numel(), seed=100 + i)
                      for i, (name, t) in enumerate(self.eng.unconstrained.items())}

    def fill(self, grads=None):
        e = self.eng
        for name, (p, m, v, g) in self.cases.items():
            if grads is not None:
                g = grads[name]
            for dst, src in ((e.unconstrained[name], p), (e._m[name], m), (e._v[name], v), (e.grads[name], g)):
                dst.copy_(torch.from_numpy(src).reshape(dst.shape))

    def read(self):
        torch.cuda.synchronize()
        e = self.eng
        return {name: tuple(d[name].detach().cpu().numpy().reshape(-1).copy() for d in (e.unconstrained, e._m, e._v))
                for name in self.cases}

    def update(self, t, grads=None):
        self.fill(grads)
        self.eng.adam(t)
        return self.read()

    def check(self, t):
        got = self.update(t)
        worst = {}
        for name, (p, m, v, g) in self.cases.items():
            ref = ar.clipped_adam_ref(p, m, v, g, t, self.lr0, self.lrd)
            bm, bv, bp = ar.adam_bounds(p, m, v, g, t, self.lr0, self.lrd)
            for what, got_x, ref_x, b_x in zip("pmv", got[name], ref, (bp, bm, bv)):
                bad, w = ar.violations(got_x, ref_x, b_x)
                i = int(np.argmax(bad))
                assert not bad.any(), (f"{name}.{what} at t = {t}: {int(bad.sum())} of {bad.size} outside the bounds, "
                                       f"first at {i}: p {p[i]!r} m {m[i]!r} v {v[i]!r} g {g[i]!r} -> {got_x[i]!r}, "
                                       f"reference {ref_x[i]!r} +- {b_x[i]!r}")
                worst[what] = max(worst.get(what, 0.0), w)
        print(f"t = {t}: worst |err| / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


@pytest.fixture(scope="module")
def sorting_screen():
    return make_sorting_variant_screen(4100, 2, seed=31, with_accessibility=True)


@pytest.fixture(scope="module")
def bound_sorting(sorting_screen):
    """G = 4100, R = 2: alpha_pi's 8 200 elements hold the whole grid, 4 100 and 820 are no multiples of 256."""
    b = _Bound("MixtureNormal", sorting_screen, scale_by_accessibility=True, fit_noise=True)
    assert set(b.cases) == {"mu_loc", "mu_scale", "sd_loc", "sd_scale", "alpha_pi", "noise_loc", "noise_scale"}
    assert b.eng.unconstrained["alpha_pi"].numel() == 8200 >= ar.N_GRID
    yield b
    b.eng.close()


@pytest.fixture(scope="module")
def bound_survival():
    """G = 130: the q0 slot, and every array shorter than one block."""
    b = _Bound("MixtureNormal", make_survival_variant_screen(130, 2, seed=32))
    assert set(b.cases) == {"mu_loc", "mu_scale", "alpha_pi", "q0"}
    assert max(t.numel() for name, t in b.eng.unconstrained.items() if name != "alpha_pi") < 256
    yield b
    b.eng.close()


@pytest.mark.parametrize("t", [1, 2, 3, 10, 100, 1000, 2000, 20000])
def test_k_adam_elementwise(bound_sorting, bound_survival, t):
    for b in (bound_sorting, bound_survival):
        g = np.concatenate([c[3] for c in b.cases.values()])
        assert (np.abs(g) <= 10).sum() > 0 and (np.abs(g) > 10).sum() > 0   # both sides of the clamp are there
        b.check(t)


@pytest.mark.parametrize("initial_lr,gamma,num_steps", [(0.01, 0.1, 2000), (0.05, 0.1, 100), (0.001, 1.0, 500)])
def test_schedule_variants(sorting_screen, initial_lr, gamma, num_steps):
    b = _Bound("MixtureNormal", sorting_screen, scale_by_accessibility=True, fit_noise=True, initial_lr=initial_lr,
               gamma=gamma, num_steps=num_steps)
    assert (b.lrd == 1.0) == (gamma == 1.0)
    for t in (1, 7, num_steps // 2, num_steps - 1, num_steps, num_steps + 1, 2 * num_steps):
        b.check(t)
    b.eng.close()


def test_non_finite_gradients(bound_sorting, bound_survival):
    """+-inf gradients act as +-10 (grad.clamp_).  A NaN gradient passes the clamp as it does in torch: that element's
    p, m and v become NaN - the fit then halts at its report window, tests/test_gpu_halt.py - and no other element
    moves by a bit."""
    for b in (bound_sorting, bound_survival):
        with_nan, without, nan_at = {}, {}, {}
        for name, (p, m, v, g) in b.cases.items():
            n = g.size
            at = sorted({0, n - 1, n // 2} | ({255, 256} if n > 257 else set()))
            pinf, ninf = [i + 1 for i in at[:-1]], [i + 2 for i in at[:-1] if i + 2 not in at]
            a, c = g.copy(), g.copy()
            a[pinf], c[pinf] = np.inf, 10.0
            a[ninf], c[ninf] = -np.inf, -10.0
            a[at], c[at] = np.nan, 0.25
            with_nan[name], without[name], nan_at[name] = a, c, at
        t = 12
        got = b.update(t, with_nan)
        want = b.update(t, without)
        for name in b.cases:
            at = nan_at[name]
            keep = np.ones(b.cases[name][3].size, dtype=bool)
            keep[at] = False
            for what, got_x, want_x in zip("pmv", got[name], want[name]):
                assert np.isnan(got_x[at]).all(), (name, what, "a NaN gradient left a finite value", got_x[at])
                assert np.isfinite(want_x).all(), (name, what)
                # (bitwise: the elements with +-inf against +-10, everything else against itself)
                assert np.array_equal(got_x[keep].view(np.uint32), want_x[keep].view(np.uint32)), (name, what)


def test_adam_rejects_t_zero(bound_survival):
    b = bound_survival
    e = b.eng
    b.fill()
    torch.cuda.synchronize()
    bound = [t for d in (e.unconstrained, e._m, e._v, e.grads) for t in d.values()]
    before = [t.clone() for t in bound]
    status = e.lib.bean_hip_adam(e._h, 0, e._sptr())
    assert status < 0
    assert "1-based" in e.lib.bean_hip_last_error().decode()
    with pytest.raises(RuntimeError, match="1-based"):
        e.adam(0)
    torch.cuda.synchronize()
    for t, was in zip(bound, before):
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))


# ------------------------------------------------------------------ fused steppers started late in the schedule
def _state(eng, member=None):
    pick = (lambda t: t) if member is None else (lambda t: t[member])
    return {f"{tag}.{k}": pick(v).detach().clone() for tag, d in (("p", eng.unconstrained), ("m", eng._m), ("v", eng._v))
            for k, v in d.items()}


def _load(eng, start):
    """The start state into the engine's tensors (every member of an ensemble), through torch."""
    for tag, d in (("p", eng.unconstrained), ("m", eng._m), ("v", eng._v)):
        for k, v in d.items():
            v.copy_(start[f"{tag}.{k}"].expand_as(v))


def _assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, (got[k].double() - want[k].double()).abs().max().item())


def _start_state(make_engine):
    eng = make_engine()
    eng.run(5, seed=SEED, graph_chunk=0)
    torch.cuda.synchronize()
    start = _state(eng)
    eng.close()
    return start


def _stepwise(make_engine, start, s0, n):
    eng = make_engine()
    _load(eng, start)
    for s in range(s0, s0 + n):
        eng.elbo_grad(step=s, seed=SEED, loss_index=s)
        eng.adam(s + 1)
    torch.cuda.synchronize()
    want = _state(eng)
    eng.close()
    assert all(torch.isfinite(v).all() for v in want.values())
    assert any(not torch.equal(want[k], start[k]) for k in want if k.startswith("p."))
    return want


def _fused(make_engine, start, what, fit, member=None):
    eng = make_engine()
    _load(eng, start)
    fit(eng)
    torch.cuda.synchronize()
    got = _state(eng, member)
    eng.close()
    return what, got


N_LATE = 9


@pytest.mark.parametrize("s0", [1, 7, 1990])
def test_late_first_step_equals_stepwise(monkeypatch, s0):
    """9 steps from first_step = s0 of a 2000-step schedule, from the state a 5-step run leaves: run (eager and
    graphs), resumed windows, the asynchronous stepper and an ensemble member against the stepwise loop."""
    from bean_amd import engine

    data = make_sorting_variant_screen(600, 3, seed=73, mask_fraction=0.05).to(DEV)
    monkeypatch.setenv("BEAN_HIP_STEP", "pair")

    def make(**kw):
        return engine.HipSVI("MixtureNormal", data, num_steps=2000, **kw)

    start = _start_state(make)
    want = _stepwise(make, start, s0, N_LATE)
    n = N_LATE

    def windows(eng):
        eng.run(4, seed=SEED, first_step=s0, resume=True)
        eng.run(5, seed=SEED, resume=True)
        assert eng.steps_done == s0 + n

    results = [
        _fused(make, start, "run, eager", lambda e: e.run(n, seed=SEED, graph_chunk=0, first_step=s0)),
        _fused(make, start, "run, graphs of 4", lambda e: e.run(n, seed=SEED, graph_chunk=4, first_step=s0)),
        _fused(make, start, "resumed windows 4 + 5", windows),
        _fused(lambda: make(n_members=2), start, "member 1 of an ensemble of 2",
               lambda e: e.run_ensemble(n, (SEED + 1, SEED), graph_chunk=4, first_step=s0), member=1),
    ]
    monkeypatch.setenv("BEAN_HIP_STEP", "async")

    def one_launch(eng):
        assert eng.dominant_kernel == "k_svi_async"
        eng.run(n, seed=SEED, first_step=s0)

    results.append(_fused(make, start, "k_svi_async", one_launch))
    for what, got in results:
        _assert_same(got, want, (s0, what))


def _with_covariates(n_guides, n_reps, n_cov, seed):
    data = make_sorting_variant_screen(n_guides, n_reps, seed=seed, mask_fraction=0.05)
    g = torch.Generator().manual_seed(seed)
    data.sample_covariates = [f"cov{i}" for i in range(n_cov)]
    data.n_sample_covariates = n_cov
    data.rep_by_cov = torch.randint(0, 2, (n_reps, n_cov), generator=g)
    data.rep_by_cov[0, 0], data.rep_by_cov[-1, 0] = 1, 0
    return data


@pytest.mark.parametrize("family,make_data,chunk", [
    ("MultiMixtureNormal", lambda: make_sorting_tiling_screen(300, 2, seed=6, n_max_alleles=6), 6),
    ("MixtureNormal", lambda: make_survival_variant_screen(800, 3, seed=6, frac_effect=0.5), 4),
    ("Normal", lambda: make_survival_variant_screen(600, 3, seed=9, frac_effect=0.5), 4),
    ("Normal", lambda: _with_covariates(600, 4, 2, seed=23), 4),
], ids=["tiling A=6", "survival MixtureNormal", "survival Normal", "sorting Normal + covariates"])
def test_late_first_step_other_families(family, make_data, chunk):
    """The families whose fused loop has a bitwise stepwise test from step 0 (tests/test_gpu_parity.py,
    tests/test_sample_covariates.py): the same from first_step = 1990."""
    from bean_amd import engine

    data = make_data().to(DEV)

    def make():
        return engine.HipSVI(family, data, num_steps=2000)

    start = _start_state(make)
    want = _stepwise(make, start, 1990, N_LATE)
    for c in (0, chunk):
        what, got = _fused(make, start, f"run, graph_chunk {c}",
                           lambda e: e.run(N_LATE, seed=SEED, graph_chunk=c, first_step=1990))
        _assert_same(got, want, (family, what))
