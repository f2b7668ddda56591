"""Every guide kernel against the float64 oracle on the count planes a depth study hands to a refit (tests/count_regimes.py:
bins of up to 2^24 - 1 reads against concentrations the observed screen fixed, bins of 0 ... 12 on both sides of the
mask threshold, both kinds of lane in one wave, the branch edges of lgamma_digamma_diff_inl planted, and screens generated
deep, where a0 is large too): the kernel, the loss to 1e-9 and every gradient element within grad_bounds.py's tolerance,
as test_gpu_grad_elementwise.py holds them at the default depth - its `evaluate` is what runs here.  Then the planes
k_simulate_design itself returns at a depth that reaches its clamp and at depth 0.01, members with these counts, the
asynchronous stepper and a trajectory on them.  -m gpu."""
import copy

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
import count_regimes as cr
import dirichlet_grad_reference as dgr
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen
from members_common import SEED, STEPS, _assert_same, _single, _state
from oracle import elbo
from oracle import svi
from test_gpu_async import _same as async_is_bitwise_the_pair_path
from test_gpu_grad_elementwise import ACC, MAKERS, SWITCHES, evaluate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

VARIANT = dict(n_guides=130, n_reps=2, guides_per_target=3, seed=31)
# the smallest shapes of test_gpu_grad_elementwise.py.  name: (kind, generator arguments, model arguments, kernel,
# family and oracle loss where they are not the mixture family of the kind)
SHAPES = {
    "variant_130x2": ("variant", dict(VARIANT), {}, "k_guide_wave2", None, None),
    "variant_130x2_acc": ("variant", dict(VARIANT, with_accessibility=True), ACC, "k_guide_wave2", None, None),
    "normal_130x2": ("variant", dict(VARIANT), {}, None, "Normal", elbo.normal_loss),
    "tiling_130x2_a5": ("tiling", dict(n_guides=130, n_reps=2, n_max_alleles=5, seed=4, depth_per_guide=30.0), {},
                        "k_guide_tiling_rep", None, None),
    "tiling_70x2_a48": ("tiling", dict(n_guides=70, n_reps=2, n_max_alleles=48, seed=14), {}, "k_guide_tiling_wide",
                        None, None),
    "survival_130x2": ("survival", dict(n_guides=130, n_reps=2, seed=4), {}, "k_guide_survival_wave", None, None),
    "survival_tiling_70x2": ("survival_tiling", dict(n_guides=70, n_reps=2, n_max_alleles=5, seed=5, depth_per_guide=30.0),
                             {}, None, None, None),
}
# every regime at the `init + 0.3 randn` point, `mixed` at the fitted-like point too (the Normal family has no alpha_pi:
# its fitted-like point is the perturbed one)
POINTS = [(r, "perturbed") for r in cr.REGIMES + ("generated_deep",)] + [("mixed", "fitted")]
CASES = [(s, r, p) for s in SHAPES for r, p in POINTS if not (s == "normal_130x2" and p == "fitted")]


@pytest.fixture(scope="module")
def engine():
    from bean_amd import engine as eng

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return eng


@pytest.fixture(autouse=True)
def _default_kernels(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("shape,regime,point", CASES)
def test_every_gradient_element_matches_the_oracle_on_the_plane(engine, shape, regime, point):
    kind, gen_kw, kw, kernel, family, loss_fn = SHAPES[shape]
    data = cr.regime_screen(MAKERS[kind], gen_kw, regime)
    evaluate(engine, f"{shape}@{regime}", point, kind, data, kw, kernel, family=family, loss_fn=loss_fn)


# generated deep with pi_a0 as generated (up to 7e4): above concentrations of 2e3 torch's implicit gradient is up to 3e-7 off
# its own formula, so the oracle takes dirichlet_grad_reference.port64, and each evaluation's share
# of the tolerance is K_dev (2^-52 |g| + budget) at its own inputs - the rule test_dirichlet_grad_matches_its_formula
# (tests/test_gpu_parity.py) holds the device function to - in place of the constants pinned on [1e-3, 2e3]
UNCLAMPED = ("variant_130x2", "tiling_130x2_a5", "survival_130x2")


def constrained_as_the_kernels(params):
    """The parameters at which the float64 oracle constrains `alpha_pi` and `q0` to the values the kernels use: they form
    `(double)expf(theta)`, a float32 exponential - as the reference's float32 parameters do - where the oracle's float64
    mode takes `exp` in float64.  The float32 exponential is taken on the device; its log in float64 is handed to the
    oracle, whose `exp` returns it (d alpha / d theta = alpha on both sides)."""
    out = dict(params)
    for k in ("alpha_pi", "q0"):
        if k in params:
            out[k] = torch.exp(params[k].float().to(DEV)).double().log().cpu()
    return out


@pytest.mark.parametrize("shape", UNCLAMPED)
def test_every_gradient_element_matches_the_oracle_above_2e3(engine, shape):
    """The oracle is evaluated at `constrained_as_the_kernels`.  Measured, one MI355X: every tensor of the three
    cases at 0.40 ... 0.49 of `tol_k` (tiling `alpha_pi` 0.45).  With the oracle's own float64 exponential the
    variant and survival cases are where they are now, and `tiling_130x2_a5` has 3 of its 650 `alpha_pi` elements
    beyond `tol_k`, the worst 3.17 `tol_k` at (51, 2) (ref 249.0511, got 249.0520, in a tensor whose median
    |element| is 4e4): up to a float32 ulp in every alpha, which the gradient `c_k (G_k - sum_a w_a G_a)` of a guide
    with five alleles amplifies by |G| / |G_k - mean| (with two alleles it is one product).
    tests/test_count_regimes.py shows the same on the host.  The pathwise constants absorb it in the clamped cases
    (`generated_deep` tiling needs its tail constant for it); the per-evaluation allowance has no room for it, and
    it is no error of the kernels - the reference's float32 parameters are constrained in float32 too (DESIGN.md
    section 5)."""
    kind, gen_kw, kw, kernel, family, loss_fn = SHAPES[shape]
    data = cr.regime_screen(MAKERS[kind], gen_kw, "generated_deep_unclamped")
    assert float(data.pi_a0.max()) > cr.PI_A0_MAX
    seen = []
    evaluate(engine, f"{shape}@generated_deep_unclamped", "perturbed", kind, data, kw, kernel, family=family, loss_fn=loss_fn,
             oracle_params=constrained_as_the_kernels, dirichlet_grad=dgr.port64_torch,
             path_allowance=dgr.path_allowance(dgr.device_k(), seen))
    al, tot, br = (np.concatenate([s[i] for s in seen]) for i in (1, 2, 3))
    high = np.maximum(al, tot - al) > cr.PI_A0_MAX
    print(f"ABOVE 2e3 {shape}: {int(high.sum())} of {high.size} evaluations hold a concentration above 2e3; branches " +
          ", ".join(f"{b} {int(n)}" for b, n in zip(dgr.BRANCHES, np.bincount(br, minlength=5))))
    assert high.mean() >= 0.25, (shape, float(high.mean()))


def test_edges_with_fifteen_bins(engine):
    """16 conditions: the 16-condition build, whose guide kernel stages its conditions differently."""
    edges = np.linspace(0, 1, 16)
    bins = tuple((float(edges[i]), float(edges[i + 1])) for i in range(15))
    data = cr.rewrite_counts(make_sorting_variant_screen(bins=bins, **VARIANT), "edges")
    assert data.n_condits == 16
    evaluate(engine, "variant_130x2_b16@edges", "perturbed", "variant", data, {}, "k_guide_wave2")


# ---------------------------------------------------------------- the study's own planes
def test_the_planes_simulate_design_returns_match_the_oracle(engine):
    """k_simulate_design on the 203 x 3 screen of test_gpu_design.py at a depth under which the largest pair reaches the
    clamp of 2^24 - 1 reads and at depth 0.01; each plane, put where the study puts it (run_inference_design: the masked
    planes of the observed screen, everything else conditioned on), evaluated by a fresh engine against the oracle."""
    data = make_sorting_variant_screen(203, 3, seed=11, mask_fraction=0.05, depth_per_guide=100.0)
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
    most = max(float(eng._keep[k].double().sum(1).max()) for k in ("X", "X_BC"))
    f_deep = (2.0 ** 24 - 0.25) / most
    assert f_deep * most < 2.0 ** 24 and np.floor(f_deep * most + 0.5) == 2.0 ** 24  # the clamp is reached, the host agrees
    sim = {k: v.cpu() for k, v in eng.simulate_design(0, 1, [f_deep, 0.01], seed=SEED).items()}
    eng.close()
    assert float(cr.pair_totals(sim["X"][0, 0]).max()) == cr.CAP
    assert float(cr.pair_totals(sim["X"][1, 0]).max()) <= 0.01 * most + 1
    for i, what in enumerate(("clamp", "x0.01")):
        redrawn = copy.copy(data)
        redrawn.X = redrawn.X_masked = sim["X"][i, 0].to(data.X_masked.dtype)
        redrawn.X_bcmatch = redrawn.X_bcmatch_masked = sim["X_bcmatch"][i, 0].to(data.X_bcmatch_masked.dtype)
        evaluate(engine, f"design_203x3@{what}", "perturbed", "variant", redrawn, {}, "k_guide_wave2")


# ---------------------------------------------------------------- members, the asynchronous stepper, a trajectory
@pytest.fixture(scope="module")
def screen_640():
    return make_sorting_variant_screen(640, 3, seed=2)


def test_members_with_these_counts_are_the_single_fits(engine, screen_640):
    """The property of test_gpu_sample_jackknife.py at the new counts: member k of one engine bound to
    [observed, deep, shallow, mixed] is, bit for bit, the single fit of plane k - parameters, moments, loss history."""
    data = screen_640.to(DEV)
    screens = [data] + [cr.rewrite_counts(data, r) for r in ("deep", "shallow", "mixed")]
    counts = (torch.stack([s.X_masked for s in screens]), torch.stack([s.X_bcmatch_masked for s in screens]))
    ens = engine.HipSVI("MixtureNormal", data, num_steps=STEPS, n_members=len(screens), member_counts=counts)
    assert ens.ensemble_supported and ens.member_counts
    ens.run_ensemble(30, [SEED] * len(screens))
    torch.cuda.synchronize()
    assert np.isfinite(ens.losses()).all()
    members = [_state(ens, k) for k in range(len(screens))]
    ens.close()
    for k, s in enumerate(screens):
        _assert_same(members[k], _single("MixtureNormal", s, {}, steps=30), f"member {k}")
    assert not torch.equal(members[1]["p.mu_loc"], members[0]["p.mu_loc"])


@pytest.mark.parametrize("regime", ["mixed", "edges"])
def test_async_is_bitwise_the_pair_path_on_the_plane(monkeypatch, screen_640, regime):
    async_is_bitwise_the_pair_path(monkeypatch, "MixtureNormal", cr.rewrite_counts(screen_640, regime), 30)


def test_exact_noise_trajectory_on_the_deep_plane_matches_oracle(engine):
    """20 steps of {ELBO grad -> ClippedAdam} on the same draws as the oracle, the rule and tolerance of
    test_exact_noise_trajectory_matches_oracle (tests/test_gpu_parity.py).  The oracle keeps its float32 parameter
    leaves and ClippedAdam, but reads the screen in float64: in the reference's mixed dtypes the log-factorials
    lgamma(1 + x) of the float32 counts are float32 values - 7.8 off at x = 2^24 - 1 - and that oracle is 6.0e-5 of the
    loss from its own float64 mode on this plane (1.3e-7 at the default depth), thirty times the tolerance."""
    data = cr.rewrite_counts(make_sorting_variant_screen(**VARIANT), "deep")
    d64 = elbo.as_float64(data)
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), dump_noise=True, num_steps=2000)
    params = elbo.init_params("MixtureNormal", data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    for t in range(20):
        loss, _ = eng.elbo_grad(step=t, seed=5, loss_index=t)
        noise = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        eng.adam(t + 1)
        ref = svi.svi_step(elbo.mixture_normal_loss, d64, params, optim, noise=noise)
        assert abs(loss - ref) <= 2e-6 * abs(ref), (t, loss, ref)
    torch.cuda.synchronize()
    for k, v in eng.unconstrained.items():
        ref = params[k].detach()
        err = (v.cpu() - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (k, err)
    eng.close()
