"""The ELBO kernels against the float64 oracle at strong effects and tight scales (tests/effect_regimes.py): mu_loc of
-4 ... 4, target scales of 0.05 ... 2, variational scales of e^-3 ... e^-5, on screens whose count precisions a0 are small
enough for a bin's concentration to sit on its floor because of its PROBABILITY - per lane, in waves that hold floored
and unfloored lanes, with bin probabilities of exactly 0 and 1 and |u| up to 97 in the Phi tables.  The kernel, the
loss to 1e-9 and every gradient element within grad_bounds.py's tolerance, as test_gpu_grad_elementwise.py holds them at
the usual point - its `evaluate` is what runs here; then DevArgs::tot_const on against off, the steppers against the pair
path from that point, the importance weights, and the concentrations the simulator forms from its own Phi tables against
50-digit arithmetic.  -m gpu."""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
import count_regimes as cr
import effect_regimes as er
import importance_common as ic
import test_gpu_async as t_async
import test_gpu_step_fused as t_fused
import test_gpu_tile_svi as t_tile
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen
from oracle import elbo
from test_gpu_count_regimes import constrained_as_the_kernels
from test_gpu_grad_elementwise import LOSS, MAKERS, SWITCHES, evaluate, point_parameters
from test_gpu_power import _check_twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 7

# name: (case of effect_regimes.CASES, kernel, environment, library variant)
GPU_CASES = {
    "variant_130x2": ("variant_130x2", "k_guide_wave2", {}, None),
    "variant_130x2_nobc": ("variant_130x2_nobc", "k_guide_wave2", {}, None),
    "variant_130x2_near_one_pi": ("variant_130x2_near_one_pi", "k_guide_wave2", {}, None),
    "variant_130x2_acc": ("variant_130x2_acc", "k_guide_wave2", {}, None),
    "variant_257x3_long_targets": ("variant_257x3_long_targets", "k_guide_wave2", {}, None),
    "tiling_130x2_a5": ("tiling_130x2_a5", "k_guide_tiling_rep", {}, None),
    "tiling_70x2_a48": ("tiling_70x2_a48", "k_guide_tiling_wide", {}, None),
    "survival_130x2": ("survival_130x2", "k_guide_survival_wave", {}, None),
    "survival_tiling_70x2": ("survival_tiling_70x2", "k_guide_tiling_rep", {}, None),
    # the generic kernels of the A/B library
    "variant_130x2_wave1": ("variant_130x2", "k_guide_wave", {"BEAN_HIP_GUIDE": "wave1"}, "ab"),
    "variant_130x2_split": ("variant_130x2", "k_lik", {"BEAN_HIP_GUIDE": "split"}, "ab"),
}


@pytest.fixture(scope="module")
def engine():
    from bean_amd import engine as eng

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return eng


@pytest.fixture(autouse=True)
def _default_kernels(monkeypatch):
    for k in SWITCHES + ("BEAN_HIP_TOT_CONST",):
        monkeypatch.delenv(k, raising=False)


def _screen(case):
    kind, gen_kw, kw, family, near_one, regime = er.CASES[case]
    return kind, er.with_small_a0(MAKERS[kind](**gen_kw)), kw, family, near_one, regime


def _loss_fn(kind, family):
    return elbo.normal_loss if family == "Normal" else LOSS[kind]


def _near_one(eng):
    R, G = eng.data.n_reps, eng.data.n_guides
    return {"pi": er.near_one_pi((R, 1, G, 2), seed=er.PI_SEED)}


# ---------------------------------------------------------------- every gradient element
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_every_gradient_element_matches_the_oracle_at_the_effect_point(engine, monkeypatch, name):
    """The census of the device's own draws is printed next to the result; where the case is one that must reach the
    regime it is asserted (a tenth of the kept pairs with a floored bin, every full wave mixed, a probability of 0), and
    in every case no raw concentration is within 1e-6 of the floor's threshold: no element is excused.

    The tiling kinds evaluate their oracle at `constrained_as_the_kernels` (tests/test_gpu_count_regimes.py), the
    two-allele kinds at the point itself.  The kernels form alpha_pi and q0 as `(double)expf(theta)`, as the reference's
    float32 parameters do, where the oracle's float64 mode takes the exponential in float64: up to a float32 ulp in every
    alpha.  With two alleles the gradient is one product and moves by that much of itself; with more,
    `c_k (G_k - sum_a w_a G_a)` cancels and amplifies it by |G| / |G_k - mean| - by the mechanism, so the rule is the
    number of alleles, not a case's result, and the variant and survival cases keep the kernels' `expf` against the
    oracle's float64 `exp`.  Measured, one MI355X, with the oracle's own float64 exponential in all eleven cases: ten
    pass (alpha_pi at 0.44 ... 0.95 of `tol_k`), and `survival_tiling_70x2` has 15 of its 350 alpha_pi elements beyond
    `tol_k`, none beyond the tail constant, the worst 3.16 `tol_k` at (42, 2) (ref -2.381724e-05, got -2.381737e-05) - at
    growth rates of +-256 |G| is large.  It is the case of test_every_gradient_element_matches_the_oracle_above_2e3
    again, to the figure (3.17 there), and no error of the kernels; with the mapping the three tiling cases have
    alpha_pi at 0.43 ... 0.45."""
    case, kernel, env, variant = GPU_CASES[name]
    kind, data, kw, family, near_one, regime = _screen(case)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    census = evaluate(engine, name, "effect", kind, data, kw, kernel, variant, family=family,
                      loss_fn=_loss_fn(kind, family), inject=_near_one if near_one else None,
                      oracle_params=constrained_as_the_kernels if kind.endswith("tiling") else None)
    assert census["nearest"] >= 1e-6, (name, census["nearest"])
    if regime:
        er.assert_reaches_the_regime(census, name)


# ---------------------------------------------------------------- the total term as a constant
@pytest.mark.parametrize("case", ["variant_130x2", "variant_130x2_near_one_pi"])
def test_total_term_as_constant_equals_evaluating_it_at_the_effect_point(engine, monkeypatch, case):
    """test_total_term_as_constant_equals_evaluating_it (tests/test_gpu_parity.py), its comparison and its bounds, where
    the correction `d0.d = dt.d - dc.d` is taken lane by lane: BEAN_HIP_TOT_CONST=1 against 0."""
    kind, data, kw, family, near_one, _ = _screen(case)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("BEAN_HIP_TOT_CONST", flag)
        eng = engine.HipSVI(family, data.to(DEV), num_steps=20, **kw)
        assert eng.dominant_kernel == "k_guide_wave2"
        params = point_parameters(kind, data, eng.unconstrained, "effect")
        for k, v in eng.unconstrained.items():
            v.copy_(params[k].to(DEV))
        if near_one:
            eng.set_noise(_near_one(eng))
        out[flag] = eng.elbo_grad(step=2, seed=11)
        eng.close()
    (l1, g1), (l0, g0) = out["1"], out["0"]
    print(f"TOT_CONST {case}: |l1 - l0| / |l0| {abs(l1 - l0) / abs(l0):.2e}; " +
          ", ".join(f"{k} {(g1[k] - g0[k]).abs().max().item() / (g0[k].abs().max().item() + 1e-30):.2e}" for k in g0))
    assert np.isfinite(l0) and abs(l1 - l0) <= 1e-12 * abs(l0), (l1, l0)
    for k in g0:
        scale = g0[k].abs().max().item() + 1e-30
        assert (g1[k] - g0[k]).abs().max().item() <= 2e-6 * scale, k  # float32 outputs: a few ulp


# ---------------------------------------------------------------- the steppers, from the effect point
STEPS = 12


def _stepper_screen(family):
    """The screen, and on the host (torch's draws, the parameters the steppers begin at) what its effect point reaches:
    asserted for the `Normal` family; the `MixtureNormal` steppers draw their own pi, which keeps the wild-type
    component's weight up - they step through the saturated Phi tables (probabilities of exactly 0 and 1), almost no
    floors."""
    data = er.with_small_a0(make_sorting_variant_screen(**er.STEPPER_SCREEN))
    assert data.n_targets >= 64
    params = point_parameters("variant", data, elbo.init_params(family, data), "effect")
    census = er.floor_census(data, params, cr.host_noise("variant", data, params), {}, family)
    print(f"CENSUS steppers {family}: {er.census_line(census)}")
    assert census["nearest"] >= 1e-6 and census["p_zero"] > 0 and census["p_one"] > 0, (family, census)
    if family == "Normal":
        er.assert_reaches_the_regime(census, "steppers")
    return data


def _at_the_effect_point(data):
    def start(eng):
        params = point_parameters("variant", data, eng.unconstrained, "effect")
        for k, v in eng.unconstrained.items():
            v.copy_(params[k].to(DEV))
    return start


@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
def test_host_driven_fused_loop_and_graph_replay_from_the_effect_point(engine, monkeypatch, family):
    """{elbo_grad, adam} stepped from the host, the loop of bean_hip_svi_run (graph_chunk = 0) and its graph replay:
    the same bits in the parameters and in the loss history."""
    monkeypatch.setenv("BEAN_HIP_STEP", "pair")
    data = _stepper_screen(family)
    start = _at_the_effect_point(data)
    fits = {}
    for how in ("host", "eager", "graph"):
        eng = engine.HipSVI(family, data.to(DEV), num_steps=50)
        assert eng.dominant_kernel == "k_guide_wave2"
        start(eng)
        if how == "host":
            for t in range(STEPS):
                eng.elbo_grad(step=t, seed=5, loss_index=t)
                eng.adam(t + 1)
        else:
            eng.run(STEPS, seed=5, graph_chunk=0 if how == "eager" else 4)
        torch.cuda.synchronize()
        fits[how] = ({k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()},
                     eng.loss_hist[:STEPS].cpu().numpy().copy())
        eng.close()
    assert np.isfinite(fits["eager"][1]).all()
    began = er.effect_point("variant", data, fits["eager"][0])["mu_loc"]   # (mu_loc does not depend on what is handed in)
    assert not torch.equal(fits["eager"][0]["mu_loc"], began)              # the 12 steps moved it
    for how in ("host", "graph"):
        for k, v in fits["eager"][0].items():
            assert torch.equal(fits[how][0][k], v), (how, k)
    for how in ("host", "graph"):
        rel = float(np.max(np.abs(fits[how][1] - fits["eager"][1]) / np.abs(fits["eager"][1])))
        print(f"STEPPERS {family} {how}: loss history against the loop's, largest relative difference {rel:.2e}")
    assert np.array_equal(fits["host"][1], fits["eager"][1])
    assert np.array_equal(fits["graph"][1], fits["eager"][1])


@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
def test_fused_step_is_bitwise_the_pair_path_from_the_effect_point(monkeypatch, family):
    data = _stepper_screen(family)
    t_fused._same(monkeypatch, family, data, STEPS, start=_at_the_effect_point(data))


@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
def test_async_is_bitwise_the_pair_path_from_the_effect_point(monkeypatch, family):
    data = _stepper_screen(family)
    t_async._same(monkeypatch, family, data, STEPS, start=_at_the_effect_point(data))


@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
def test_tile_path_equals_two_launch_path_from_the_effect_point(family):
    data = _stepper_screen(family)
    t_tile._compare(family, data, chunks=(1, 4, 7), start=_at_the_effect_point(data))


# ---------------------------------------------------------------- the importance weights
def test_importance_weights_at_the_effect_point(engine):
    """log_weights of 4 draws, Normal 130 x 2: minus the sum over targets is elbo_grad's loss of that draw to 1e-9, and
    every target's weight is the oracle's within 1e-9 x the magnitude of its site terms (tests/test_gpu_importance.py)."""
    kind, data, kw, family, _, _ = _screen("variant_130x2")
    eng = engine.HipSVI(family, data.to(DEV), dump_noise=True, num_steps=20)
    assert eng.predictive_supported
    params = point_parameters(kind, data, eng.unconstrained, "effect")
    for k, v in eng.unconstrained.items():
        v.copy_(params[k].to(DEV))
    out = eng.log_weights(0, 4, seed=SEED)
    logw = out["logw"].cpu()
    assert logw.shape == (4, data.n_targets) and bool(torch.isfinite(logw).all())
    worst = 0.0
    for d in range(4):
        loss, _ = eng.elbo_grad(step=d, seed=SEED)
        noise = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        got = -float(logw[d].sum())
        print(f"IMPORTANCE draw {d}: loss {loss:.9f}, - sum logw {got:.9f}, relative {abs(got - loss) / abs(loss):.2e}")
        assert abs(got - loss) <= 1e-9 * abs(loss), d
        for t in range(data.n_targets):
            want, mag = ic.oracle_logw(family, data, params, noise, t, kw)
            worst = max(worst, abs(float(logw[d, t]) - want) / (1e-9 * mag))
            assert abs(float(logw[d, t]) - want) <= 1e-9 * mag, (d, t, float(logw[d, t]), want)
    eng.close()
    print(f"IMPORTANCE per target: worst |logw - oracle| / (1e-9 magnitude) {worst:.3f}")


# ---------------------------------------------------------------- the device's concentrations against exact arithmetic
def _fixed_sites(eng, data, params, mixture, acc):
    """mu_scale = sd_scale = -20 and every eps handed in as 0: the sites sit at their locations exactly."""
    for k in ("mu_scale", "sd_scale"):
        params[k] = torch.full_like(params[k], -20.0)
    for k, v in eng.unconstrained.items():
        v.copy_(params[k].to(DEV))
    T, G = data.n_targets, data.n_guides
    noise = {"eps_mu": torch.zeros(T, dtype=torch.float64), "eps_sd": torch.zeros(T, dtype=torch.float64)}
    if mixture:
        noise.update(_near_one(eng))
    if acc:
        noise["eps_noise"] = torch.zeros(G, dtype=torch.float64)
    eng.set_noise(noise)
    return noise.get("pi")


def _hold_alpha(what, got, exact, budget, floored):
    worst, on_floor = er.alpha_ratio(got, exact, budget, floored)
    print(f"ALPHA {what}: device worst |err| / budget {worst:.3f} (allowed {er.DEVICE_MARGIN * er.K_HOST:.2f}); "
          f"{int(floored.sum())} of {floored.size} on the floor")
    assert on_floor, what                                   # floored elements are 1e-5 exactly
    assert np.array_equal(got == er.EPS, floored), what     # and nothing else is
    assert worst <= er.DEVICE_MARGIN * er.K_HOST, (what, worst)


@pytest.mark.parametrize("case", ["variant_130x2", "variant_130x2_near_one_pi", "variant_130x2_acc"])
def test_simulated_concentrations_match_exact_arithmetic(engine, case):
    """eng.simulate(alphas=True): every element of both planes against effect_regimes.exact_alpha within 4 K of its float64
    budget, K the multiple torch's own float64 evaluation needs (test_effect_regimes.py)."""
    kind, data, kw, family, _, _ = _screen(case)
    acc = bool(kw.get("scale_by_accessibility"))
    eng = engine.HipSVI(family, data.to(DEV), num_steps=20, **kw)
    assert eng.predictive_supported and eng.use_bcmatch
    params = point_parameters(kind, data, eng.unconstrained, "effect")
    pi = _fixed_sites(eng, data, params, family == "MixtureNormal", acc)
    got = eng.simulate(2, seed=SEED, alphas=True)["alpha"].cpu().numpy()
    eng.close()
    exact, budget, floored = er.exact_alpha(family, data, params, pi=pi, acc_noise=params["noise_loc"] if acc else None)
    assert got.shape == exact.shape == (2, data.n_reps, data.n_condits, data.n_guides)
    _hold_alpha(case, got, exact, budget, floored)
    if er.CASES[case][5]:
        assert floored[:, data.sample_mask.numpy().astype(bool)].any()


POWER_EFFECTS = (-4.0, -2.0, 2.0, 4.0)


@pytest.mark.parametrize("family", ["Normal", "MixtureNormal"])
def test_power_planes_at_strong_planted_effects(engine, family):
    """simulate_power with -4, -2, 2, 4 planted: the planes are the twin engine's launch bit for bit (_check_twin of
    tests/test_gpu_power.py at these effects), and the twin's concentrations with the effect planted on every target
    are within the same allowance of exact arithmetic.  The two steps are at different states: the bitwise one at the
    effect point's variational scales (e^-3 ... e^-5) with eps_sd drawn, the exact one at scales of -20 with every eps
    at 0 - so `planted_phi_entry` is tied to exact arithmetic through the twin's `write_phi_entry`, not compared with
    it at the state of the bitwise check."""
    kind, data, kw, _, _, _ = _screen("variant_130x2")
    eng, twin = (engine.HipSVI(family, data.to(DEV), num_steps=20) for _ in range(2))
    assert eng.predictive_supported
    params = point_parameters(kind, data, eng.unconstrained, "effect")
    for k, v in eng.unconstrained.items():
        v.copy_(params[k].to(DEV))
    _check_twin(eng, twin, 2, effects=POWER_EFFECTS)
    pi = _fixed_sites(twin, data, params, family == "MixtureNormal", False)
    for e in POWER_EFFECTS:
        params["mu_loc"] = torch.full_like(params["mu_loc"], e)
        twin.unconstrained["mu_loc"].copy_(params["mu_loc"].to(DEV))
        got = twin.simulate(2, seed=SEED, alphas=True)["alpha"].cpu().numpy()
        exact, budget, floored = er.exact_alpha(family, data, params, pi=pi)
        _hold_alpha(f"power {family} effect {e:+.0f}", got, exact, budget, floored)
    eng.close()
    twin.close()
