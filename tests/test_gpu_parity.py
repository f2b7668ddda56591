"""Parity of the HIP path (through the C ABI) with the CPU oracle.  -m gpu.

Tolerances: the kernels compute in float64 from float32-stored parameters and
emit float32 gradients (as the reference's autograd does for float32 leaves), so
  * against the oracle in "f64" mode (same arithmetic width): loss rel 1e-9,
    gradients rel 5e-7 of the largest entry (float32 output rounding);
  * against the oracle in the reference's mixed f32/f64 dtypes: loss rel 1e-6,
    gradients rel 2e-5.
"""
import ast
import os

import mpmath
import numpy as np
import pytest
import scipy.special as sp
import scipy.stats as st
import torch

import bean_amd  # noqa: F401
import dirichlet_grad_reference as dgr
from bean_amd.preprocessing.synthetic import DEFAULT_BINS, make_sorting_variant_screen
from oracle import elbo, svi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "elbo_cases.npz"))


@pytest.fixture(scope="module")
def engine():
    from bean_amd import engine as eng

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return eng


# ------------------------------------------------------------ special functions
def test_lgamma_digamma_differences(engine):
    rng = np.random.default_rng(0)
    n = 300_000
    a = np.exp(rng.uniform(np.log(1e-5), np.log(1e5), n))
    x = np.floor(np.exp(rng.uniform(0, np.log(1e5), n))) * (rng.random(n) > 0.1)
    x[:1000] = rng.integers(0, 14, 1000)           # product-form branch
    x[1000:2000] += 0.5                            # non-integer counts take the series branch
    d, dp = engine.test_special(0, a, x)
    ref_d = sp.gammaln(a + x) - sp.gammaln(a)
    ref_dp = sp.digamma(a + x) - sp.digamma(a)
    # the scipy reference is itself a difference of rounded values: allow its
    # cancellation error (a few ulp of the larger term) on top of 1e-12 relative
    eps = np.finfo(float).eps
    tol_d = 1e-12 * np.maximum(1.0, np.abs(ref_d)) + 8 * eps * (np.abs(sp.gammaln(a + x)) + np.abs(sp.gammaln(a)))
    tol_dp = 1e-12 * np.maximum(1.0, np.abs(ref_dp)) + 8 * eps * (np.abs(sp.digamma(a + x)) + np.abs(sp.digamma(a)))
    assert np.all(np.abs(d.cpu().numpy() - ref_d) <= tol_d)
    assert np.all(np.abs(dp.cpu().numpy() - ref_dp) <= tol_dp)
    # small arguments, where no cancellation hides errors, to 1e-13
    small = (a < 50) & (x < 50)
    assert np.max(np.abs(d.cpu().numpy() - ref_d)[small] / np.maximum(1.0, np.abs(ref_d[small]))) < 1e-13


def test_two_chain_difference_is_bitwise_the_one_chain_function(engine):
    """lgamma_digamma_diff2 (two independent chains side by side, csrc/bean_special.hpp) must return exactly
    what lgamma_digamma_diff returns per element: waves mix the two (a wave with a count <= 12 in any lane
    takes the one-chain function), so a lane's result must not depend on which one its wave ran."""
    rng = np.random.default_rng(5)
    n = 1 << 16
    a = np.exp(rng.uniform(np.log(1e-5), np.log(1e5), n))
    x = np.floor(np.exp(rng.uniform(np.log(13.0), np.log(1e5), n)))  # series branch in every lane of most waves
    x[: n // 8] = rng.integers(0, 14, n // 8)                        # waves that fall back to the one-chain form
    x[n // 8: n // 4] += 0.5
    d1, p1 = engine.test_special(0, a, x)
    d2, p2 = engine.test_special(5, a, x)
    assert torch.equal(d1, d2) and torch.equal(p1, p2)


def test_lgamma_digamma_and_phi(engine):
    rng = np.random.default_rng(1)
    a = np.exp(rng.uniform(np.log(1e-5), np.log(1e6), 100_000))
    lg, dg = engine.test_special(1, a)
    assert np.max(np.abs(lg.cpu().numpy() - sp.gammaln(a)) / np.maximum(1.0, np.abs(sp.gammaln(a)))) < 1e-13
    assert np.max(np.abs(dg.cpu().numpy() - sp.digamma(a)) / np.maximum(1.0, np.abs(sp.digamma(a)))) < 1e-13
    u = rng.normal(0, 3, 100_000)
    phi, _ = engine.test_special(3, u)
    assert np.max(np.abs(phi.cpu().numpy() - st.norm.cdf(u))) < 1e-15


# The domain a depth study's refits reach: counts up to the simulator's clamp of 2^24 - 1 per pair
# against concentrations of 1e-5 (get_alpha's clamp) ... 1e7, with the branch edges of lgamma_digamma_diff_inl planted.
CAP = float((1 << 24) - 1)
EDGE_X = (1.0, 2.0, 11.0, 12.0, 13.0, 14.0, CAP)                              # product form | series at 12 | 13
EDGE_A = (1e-5, float(np.nextafter(6.0, 0.0)), 6.0, float(np.nextafter(10.0, 0.0)), 10.0, 1e7)  # kShiftLo, kShift
N_WIDE = 6000
N_DEEP_WAVES = 32  # the first 32 waves of 64 hold x > 12 in every lane: lgamma_digamma_diff2's two-chain form


def wide_domain_inputs():
    """(a, x, sum10): 6 000 points, a log-uniform on [1e-5, 1e7], x an integer log-uniform on [1, 2^24 - 1].  Elements
    0 ... 2047 are whole waves with every x > 12 and hold EDGE_A x {13, 14, 2^24 - 1}; the waves after them mix counts on
    both sides of 12 and hold EDGE_A x EDGE_X and, with non-integer x (the series branch with a second argument that
    needs its shift), pairs whose a + x is the double just below 10 and exactly 10 (`sum10`: their indices)."""
    rng = np.random.default_rng(11)
    n, deep = N_WIDE, 64 * N_DEEP_WAVES
    a = np.exp(rng.uniform(np.log(1e-5), np.log(1e7), n))
    x = np.clip(np.floor(np.exp(rng.uniform(0.0, np.log(CAP), n))), 1.0, CAP)
    x[:deep] = np.maximum(x[:deep], 13.0)
    i = 5
    for av in EDGE_A:
        for xv in EDGE_X[4:]:
            a[i], x[i] = av, xv
            i += 37  # spread over the deep waves, odd and even lanes (op 5 pairs element i with i ^ 1)
    assert i < deep
    i = deep + 3
    for av in EDGE_A:
        for xv in EDGE_X:
            a[i], x[i] = av, xv
            i += 41
    sum10 = []
    for av in (0.37, 3.25, 5.75, 6.5, 7.5):  # shifts of the first argument: six, three, one, none, none
        at = 10.0 - av
        while av + at < 10.0:
            at = float(np.nextafter(at, np.inf))
        assert av + at == 10.0 and at != np.floor(at)
        below = at
        while av + below >= 10.0:
            below = float(np.nextafter(below, 0.0))
        assert av + below == float(np.nextafter(10.0, 0.0))
        for xv in (below, at):
            a[i], x[i] = av, xv
            sum10.append(i)
            i += 41
    assert i < n and x[:deep].min() > 12 and (x[deep:] <= 12).sum() > 500
    return a, x, np.array(sum10)


def mp_differences(a, x, dps=50):
    """lgamma(a + x) - lgamma(a), digamma(a + x) - digamma(a) and |lgamma(a + x)| + |lgamma(a)|, formed at `dps` digits
    from the float64 inputs: exact to float64, so the reference needs no cancellation allowance."""
    d, dp, mag = np.empty(len(a)), np.empty(len(a)), np.empty(len(a))
    with mpmath.workdps(dps):
        for i, (av, xv) in enumerate(zip(a, x)):
            am, zm = mpmath.mpf(float(av)), mpmath.mpf(float(av)) + mpmath.mpf(float(xv))
            l2, l1 = mpmath.loggamma(zm), mpmath.loggamma(am)
            d[i], dp[i], mag[i] = float(l2 - l1), float(mpmath.digamma(zm) - mpmath.digamma(am)), float(abs(l2) + abs(l1))
    return d, dp, mag


def wide_domain_rules(ref_d, ref_dp, mag):
    """The allowances of the two outputs: 1e-13 relative on d plus the rounding of the Stirling head's two products
    (8 eps of their magnitudes: what test_lgamma_digamma_differences grants); 1e-12 relative on dp, the constant
    grad_bounds.C_DIGAMMA rests on, with no allowance at all."""
    eps = np.finfo(float).eps
    return 1e-13 * np.maximum(1.0, np.abs(ref_d)) + 8 * eps * mag, 1e-12 * np.maximum(1.0, np.abs(ref_dp))


def test_lgamma_digamma_differences_on_the_depth_study_domain(engine):
    a, x, sum10 = wide_domain_inputs()
    d, dp = (t.cpu().numpy() for t in engine.test_special(0, a, x))
    ref_d, ref_dp, mag = mp_differences(a, x)
    tol_d, tol_dp = wide_domain_rules(ref_d, ref_dp, mag)
    r_d, r_dp = np.abs(d - ref_d) / tol_d, np.abs(dp - ref_dp) / tol_dp
    i, j = int(np.argmax(r_d)), int(np.argmax(r_dp))
    print(f"WIDE DOMAIN d: worst err / rule {r_d[i]:.4f} at a = {a[i]!r}, x = {x[i]!r}; "
          f"dp: worst err / rule {r_dp[j]:.4f} at a = {a[j]!r}, x = {x[j]!r}; "
          f"at a + x = 10 | just below: d {r_d[sum10].max():.4f}, dp {r_dp[sum10].max():.4f}")
    bad = np.nonzero((r_d > 1) | (r_dp > 1) | ~np.isfinite(d) | ~np.isfinite(dp))[0]
    assert bad.size == 0, [(float(a[k]), float(x[k]), float(r_d[k]), float(r_dp[k])) for k in bad[:20]]


def test_two_chain_difference_is_bitwise_the_one_chain_function_on_the_depth_study_domain(engine):
    """The property of test_two_chain_difference_is_bitwise_the_one_chain_function for counts up to 2^24 - 1: the first
    32 waves hold x > 12 in every lane and take the two-chain form (every planted a among them), the others mix."""
    a, x, _ = wide_domain_inputs()
    waves = x[: 64 * (N_WIDE // 64)].reshape(-1, 64)
    all_deep = (waves > 12).all(1)
    assert all_deep[:N_DEEP_WAVES].all() and (~all_deep[N_DEEP_WAVES:]).sum() >= 50
    d1, p1 = engine.test_special(0, a, x)
    d2, p2 = engine.test_special(5, a, x)
    assert torch.equal(d1.view(torch.int64), d2.view(torch.int64))
    assert torch.equal(p1.view(torch.int64), p2.view(torch.int64))


def test_lgamma_digamma_up_to_the_largest_second_argument(engine):
    """lgamma / digamma (op 1) up to 2e7, the largest a + x, against 50 digits at the 1e-13 relative of
    test_lgamma_digamma_and_phi."""
    rng = np.random.default_rng(12)
    z = np.exp(rng.uniform(np.log(1e-5), np.log(2e7), 4000))
    z[:8] = (1e-5, 6.0, float(np.nextafter(10.0, 0.0)), 10.0, CAP, CAP + 1e-5, 1e7 + CAP, 2e7)
    lg, dg = (t.cpu().numpy() for t in engine.test_special(1, z))
    with mpmath.workdps(50):
        ref_lg = np.array([float(mpmath.loggamma(mpmath.mpf(float(v)))) for v in z])
        ref_dg = np.array([float(mpmath.digamma(mpmath.mpf(float(v)))) for v in z])
    r_lg = np.abs(lg - ref_lg) / np.maximum(1.0, np.abs(ref_lg))
    r_dg = np.abs(dg - ref_dg) / np.maximum(1.0, np.abs(ref_dg))
    print(f"WIDE DOMAIN lgamma: worst relative error {r_lg.max():.3e} at {z[int(np.argmax(r_lg))]!r}; "
          f"digamma: {r_dg.max():.3e} at {z[int(np.argmax(r_dg))]!r}")
    assert r_lg.max() < 1e-13 and r_dg.max() < 1e-13


def test_dirichlet_grad_matches_torch(engine):
    rng = np.random.default_rng(2)
    n = 200_000
    al = np.exp(rng.uniform(np.log(1e-3), np.log(2e3), n))
    be = np.exp(rng.uniform(np.log(1e-3), np.log(2e3), n))
    x = rng.beta(al, be).clip(1e-12, 1 - 1e-12)
    g, _ = engine.test_special(2, al, x, al + be)
    ref = torch._dirichlet_grad(torch.tensor(x), torch.tensor(al), torch.tensor(al + be)).numpy()
    ok = np.isfinite(ref)
    assert ok.mean() > 0.999
    rel = np.abs(g.cpu().numpy()[ok] - ref[ok]) / np.maximum(1e-300, np.abs(ref[ok]))
    # the saddle-point branch cancels near x ~ mean: torch's own value carries the same
    # rounding sensitivity, so bound the tail loosely and the bulk tightly
    assert rel.max() < 1e-6, rel.max()
    assert np.quantile(rel, 0.9) < 1e-12 and np.quantile(rel, 0.999) < 1e-8


# The implicit gradient against its exact formula on tests/golden/dirichlet_grad_cases.npz: concentrations of 1e-5 ... 1e5,
# draws on the kernels' clamps, every branch edge planted (tests/dirichlet_grad_reference.py).
@pytest.fixture(scope="module")
def formula_cases():
    f = dgr.load_fixture()
    return f, dgr.device_k(f)


def held_to_the_formula(what, got, f, k_dev):
    """|got - ref| <= K_dev (2^-52 |ref| + budget) at every fixture point, K_dev four times what torch's float64
    evaluation needs in that branch; a point within 1e-12 of a branch edge may match either of its two branches, one
    planted exactly on an edge only the branch exact arithmetic takes.  Prints the worst ratio per branch."""
    assert np.isfinite(got).all(), (what, np.nonzero(~np.isfinite(got))[0][:10])
    assert (got != 0).all(), (what, np.nonzero(got == 0)[0][:10])  # no isnan -> 0 fallback fired: no reference is zero
    ratio, br = dgr.fixture_ratio(got, f)
    for b, name in enumerate(dgr.BRANCHES):
        idx = np.nonzero(br == b)[0]
        i = idx[int(np.argmax(ratio[idx]))]
        print(f"FORMULA {what} {name}: worst err / (2^-52 |ref| + budget) {ratio[i]:.3f} of K_dev {k_dev[b]:.2f} at "
              f"(x, alpha, total) = ({f['x'][i]!r}, {f['alpha'][i]!r}, {f['total'][i]!r}), relative error "
              f"{abs(got[i] / f['ref'][i] - 1):.2e}, {len(idx)} points")
        first = br[idx] == f["branch"][idx]
        rel = np.abs(got[idx] / np.where(first, f["ref"][idx], f["ref2"][idx]) - 1)
        j = int(np.argmax(rel))
        print(f"FORMULA {what} {name}: largest relative error {rel[j]:.2e} at ({f['x'][idx[j]]!r}, {f['alpha'][idx[j]]!r}, "
              f"{f['total'][idx[j]]!r}), where the budget is "
              f"{np.where(first, f['budget_rel'][idx], f['budget2_rel'][idx])[j]:.2e} of the value")
    bad = np.nonzero(ratio > k_dev[br])[0]
    assert bad.size == 0, [(what, dgr.BRANCHES[br[k]], float(f["x"][k]), float(f["alpha"][k]), float(f["total"][k]),
                            float(ratio[k])) for k in bad[:20]]


@pytest.mark.parametrize("op", [2, 10])
def test_dirichlet_grad_matches_its_formula(engine, formula_cases, op):
    """Op 2 (dirichlet_grad_one) and op 10 (dirichlet_grad_one_pre, the device's own digammas supplied)."""
    f, k_dev = formula_cases
    g, _ = engine.test_special(op, f["alpha"], f["x"], f["total"])
    held_to_the_formula(f"op {op}", g.cpu().numpy(), f, k_dev)


def test_precomputed_digamma_form_is_bitwise_the_plain_function_on_the_whole_domain(engine, formula_cases):
    """The property of test_precomputed_digamma_form_is_bitwise_the_plain_function (tests/test_gpu_grad_elementwise.py)
    on [1e-5, 1e5] and on the clamps."""
    f, _ = formula_cases
    plain, _ = engine.test_special(2, f["alpha"], f["x"], f["total"])
    pre, _ = engine.test_special(10, f["alpha"], f["x"], f["total"])
    assert torch.equal(plain.view(torch.int64), pre.view(torch.int64))


@pytest.mark.parametrize("a,b", [(0.3, 0.7), (0.9, 14.0), (2.5, 2.5), (40.0, 7.0), (1e-5, 3.0)])
def test_dirichlet_sampler_distribution(engine, a, b):
    n = 200_000
    seed = np.zeros(n)
    seed[:1] = np.frombuffer(np.uint64(77 + int(a * 10)).tobytes(), dtype=np.float64)
    p0, p1 = engine.test_special(4, np.full(n, a), seed, np.full(n, b))
    p0, p1 = p0.cpu().numpy(), p1.cpu().numpy()
    assert np.all((p0 > 0) & (p0 < 1) & (p1 > 0) & (p1 < 1))
    np.testing.assert_allclose(p0 + p1, 1.0, atol=1e-15)
    if a >= 0.01:
        ks = st.kstest(p0, st.beta(a, b).cdf)
        assert ks.pvalue > 1e-4, ks
    else:
        # concentration 1e-5 (masked alleles): almost all mass at 0
        assert np.mean(p0 < 1e-100) > 0.99


@pytest.mark.parametrize("a,b", [(1e-5, 1e-5), (1e-5, 0.0), (2e-3, 1e-5), (0.05, 0.3), (0.9, 1e-4), (3.0, 1e-5)])
def test_float32_floor_sampler_returns_the_plain_samplers_values(engine, a, b):
    """The survival q0 site (k_param's q0 blocks) keeps max((float)g, FLT_MIN) of each gamma; its sampler
    leaves the rejection loop out where U^(1/alpha) < FLT_MIN / 128 has decided that already.  Same generator
    position, same values as the plain sampler, draw for draw - including the draws that do NOT end on the
    floor (alpha = 2e-3: 16 %, 0.05: 99 %)."""
    n = 300_000
    seed = np.zeros(n)
    seed[:1] = np.frombuffer(np.uint64(4242).tobytes(), dtype=np.float64)
    g0, g1 = engine.test_special(6, np.full(n, a), seed, np.full(n, b))
    f0, f1 = engine.test_special(7, np.full(n, a), seed, np.full(n, b))
    assert torch.equal(g0, f0) and torch.equal(g1, f1)
    floor = np.float64(np.float32(1.17549435e-38))
    frac = float((g0.cpu().numpy() == floor).mean())
    if a <= 1e-5:
        assert frac > 0.998
    elif a >= 0.05:
        assert frac < 0.05


@pytest.mark.parametrize("a,b", [(1e-6, 1e-6), (5e-7, 1.0), (2e-6, 0.4), (1e-4, 1e-6), (0.01, 1e-5), (0.7, 3e-6), (2.0, 1e-6)])
def test_double_floor_sampler_returns_the_plain_samplers_values(engine, a, b):
    """The wide tiling kernel keeps max(g, DBL_MIN) of each allele gamma; its sampler leaves the rejection loop
    out where U^(1/alpha) has already put the draw below DBL_MIN.  Same generator position, same values as the
    plain sampler, draw for draw, also where only one of the pair - or neither - ends on the floor."""
    n = 300_000
    seed = np.zeros(n)
    seed[:1] = np.frombuffer(np.uint64(977).tobytes(), dtype=np.float64)
    g0, g1 = engine.test_special(8, np.full(n, a), seed, np.full(n, b))
    f0, f1 = engine.test_special(9, np.full(n, a), seed, np.full(n, b))
    assert torch.equal(g0, f0) and torch.equal(g1, f1)
    frac = float((g0.cpu().numpy() == np.finfo(np.float64).tiny).mean())
    if a <= 2e-6:
        assert frac > 0.995  # masked alleles: P(U^(1/a) > DBL_MIN) = 708 a
    elif a >= 0.01:
        assert frac < 1e-3


# ------------------------------------------------------------------ ELBO parity
def _compare(engine, family, data, kw, seed=7, step=3, tol_loss=(1e-9, 1e-6), tol_grad=(5e-7, 2e-5),
             perturb=0.3, eng_kw=None):
    torch.manual_seed(seed)
    eng = engine.HipSVI(family, data.to(DEV), dump_noise=True, num_steps=50, **(eng_kw or kw))
    for v in eng.unconstrained.values():
        v.add_(perturb * torch.randn_like(v))
    loss, grads = eng.elbo_grad(step=step, seed=seed)
    noise = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    assert np.isfinite(loss)
    for mode, tl, tg in (("f64", tol_loss[0], tol_grad[0]), ("ref", tol_loss[1], tol_grad[1])):
        params = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
        d = data
        if mode == "f64":
            params = {k: v.double() for k, v in params.items()}
            d = elbo.as_float64(data)
        params = {k: v.requires_grad_(True) for k, v in params.items()}
        ref_loss, ref_grads, _ = svi.loss_and_grads(elbo.LOSSES[family], d, params, noise=noise, **kw)
        assert abs(loss - ref_loss) <= tl * abs(ref_loss), (mode, loss, ref_loss)
        for k, g in grads.items():
            ref = ref_grads[k].double().reshape(-1)
            err = (g.cpu().double().reshape(-1) - ref).abs().max().item()
            assert err <= tg * (ref.abs().max().item() + 1e-30), (mode, k, err, ref.abs().max().item())
    # injecting the same draws reproduces the evaluation exactly
    eng.set_noise(noise)
    loss_b, grads_b = eng.elbo_grad(step=step, seed=seed)
    assert abs(loss_b - loss) <= 1e-12 * abs(loss)
    for k in grads:
        assert torch.equal(grads[k], grads_b[k])
    eng.close()
    return loss


@pytest.mark.parametrize("family,gen_kw,kw", [
    ("MixtureNormal", dict(n_guides=3000, n_reps=3, mask_fraction=0.05), {}),
    ("MixtureNormal", dict(n_guides=1500, n_reps=2, with_accessibility=True), dict(scale_by_accessibility=True)),
    ("MixtureNormal", dict(n_guides=1500, n_reps=2, with_accessibility=True),
     dict(scale_by_accessibility=True, fit_noise=False)),
    ("Normal", dict(n_guides=2000, n_reps=3, mask_fraction=0.05), {}),
    ("Normal", dict(n_guides=700, n_reps=2), dict(use_bcmatch=False)),
    # targets longer than a 64-guide tile (100 guides each, 70 targets: thin mode): a target's partial sums come
    # from up to three tiles and k_param finds them through the per-target descriptor (DevArgs::tdesc)
    ("MixtureNormal", dict(n_guides=7000, n_reps=3, guides_per_target=100, mask_fraction=0.05), {}),
    ("Normal", dict(n_guides=9100, n_reps=2, guides_per_target=130), {}),
])
def test_elbo_and_gradients_match_oracle(engine, family, gen_kw, kw):
    data = make_sorting_variant_screen(seed=31, **gen_kw)
    _compare(engine, family, data, kw)


def test_control_normal_matches_oracle(engine):
    data = make_sorting_variant_screen(3000, 3, seed=32)
    sub = data[data.negctrl_guide_idx]
    assert sub.n_guides >= 10
    _compare(engine, "ControlNormal", sub, {})


@pytest.mark.parametrize("n_guides,n_reps", [(1, 1), (63, 1), (64, 2), (65, 3), (130, 9), (257, 12)])
def test_ragged_shapes(engine, n_guides, n_reps):
    data = make_sorting_variant_screen(n_guides, n_reps, seed=40 + n_guides, guides_per_target=3)
    _compare(engine, "MixtureNormal", data, {})


@pytest.mark.parametrize("n_bins", [1, 2, 3, 5, 7, 8, 11, 15, 19, 31, 39, 63])  # > 7 bins (+ bulk): the 16-condition build, which stages conditions 17 ... 64 one by one
def test_bin_counts(engine, n_bins):
    edges = np.linspace(0, 1, n_bins + 1)
    bins = tuple((float(edges[i]), float(edges[i + 1])) for i in range(n_bins))
    data = make_sorting_variant_screen(300, 2, bins=bins, seed=50 + n_bins)
    assert data.n_condits == n_bins + 1
    _compare(engine, "MixtureNormal", data, {})


def test_prior_params(engine):
    data = make_sorting_variant_screen(500, 2, seed=61)
    T = data.n_targets
    g = torch.Generator().manual_seed(0)
    prior = {
        "mu_loc": torch.randn((T, 1), generator=g, dtype=torch.float64) * 0.2,
        "mu_scale": torch.rand((T, 1), generator=g, dtype=torch.float64) + 0.5,
        "sd_loc": torch.randn((T, 1), generator=g, dtype=torch.float64) * 0.1,
        "sd_scale": torch.rand((T, 1), generator=g, dtype=torch.float64) * 0.05 + 0.01,
    }
    _compare(engine, "MixtureNormal", data, dict(prior_params=prior))
    _compare(engine, "Normal", data, dict(prior_params={"sd_scale": prior["sd_scale"]}))


def test_all_masked_and_low_count_guides(engine):
    data = make_sorting_variant_screen(200, 2, seed=62, depth_per_guide=2.0)  # sums <= 10 get masked
    assert (data.X_masked.sum(1) <= 10).any()
    _compare(engine, "MixtureNormal", data, {})
    data2 = make_sorting_variant_screen(100, 2, seed=63)
    data2.repguide_mask[:] = False
    _compare(engine, "MixtureNormal", data2, {})


@pytest.mark.parametrize("tag,family,kw", [
    ("mix", "MixtureNormal", {}), ("mixacc", "MixtureNormal", dict(scale_by_accessibility=True)),
    ("normal", "Normal", {}), ("control", "ControlNormal", {}),
])
def test_frozen_golden_cases(engine, tag, family, kw):
    gen_kw = ast.literal_eval(str(GOLD[f"{tag}__gen"]))
    data = make_sorting_variant_screen(**gen_kw)
    eng = engine.HipSVI(family, data.to(DEV), num_steps=10, **kw)
    for k, v in eng.unconstrained.items():
        v.copy_(torch.as_tensor(GOLD[f"{tag}__param__{k}"]).reshape(v.shape))
    noise = {k.split("__")[-1]: torch.as_tensor(GOLD[k]) for k in GOLD.files if k.startswith(f"{tag}__noise__")}
    eng.set_noise(noise)
    loss, grads = eng.elbo_grad()
    want = float(GOLD[f"{tag}__loss"])
    assert abs(loss - want) <= 1e-6 * abs(want)
    for k, g in grads.items():
        ref = torch.as_tensor(GOLD[f"{tag}__grad__{k}"]).double().reshape(-1)
        err = (g.cpu().double().reshape(-1) - ref).abs().max().item()
        assert err <= 2e-5 * ref.abs().max().item(), (k, err)
    eng.close()


# ------------------------------------------------------------------ trajectories
def test_exact_noise_trajectory_matches_oracle(engine):
    """30 steps of {ELBO grad -> ClippedAdam} on the same draws as the oracle."""
    data = make_sorting_variant_screen(400, 2, seed=71)
    n = 30
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), dump_noise=True, num_steps=2000)
    params = elbo.init_params("MixtureNormal", data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    for t in range(n):
        loss, _ = eng.elbo_grad(step=t, seed=5, loss_index=t)
        noise = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        eng.adam(t + 1)
        ref = svi.svi_step(elbo.mixture_normal_loss, data, params, optim, noise=noise)
        assert abs(loss - ref) <= 2e-6 * abs(ref), (t, loss, ref)
    torch.cuda.synchronize()
    for k, v in eng.unconstrained.items():
        ref = params[k].detach()
        err = (v.cpu() - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (k, err)
    eng.close()


def test_fused_loop_equals_stepwise_and_graph_equals_eager(engine):
    data = make_sorting_variant_screen(900, 3, seed=72).to(DEV)
    n = 40
    a = engine.HipSVI("MixtureNormal", data, num_steps=500)
    for t in range(n):
        a.elbo_grad(step=t, seed=9, loss_index=t)
        a.adam(t + 1)
    torch.cuda.synchronize()
    b = engine.HipSVI("MixtureNormal", data, num_steps=500)
    b.run(n, seed=9, graph_chunk=0)
    c = engine.HipSVI("MixtureNormal", data, num_steps=500)
    c.run(n, seed=9, graph_chunk=8)
    lb, lc = b.losses(), c.losses()
    la = a.loss_hist[:n].cpu().tolist()
    np.testing.assert_allclose(lb, la, rtol=1e-12)
    np.testing.assert_allclose(lc, lb, rtol=1e-12)
    for k in a.unconstrained:
        assert torch.equal(a.unconstrained[k], b.unconstrained[k]), k   # same arithmetic, bitwise
        assert torch.equal(b.unconstrained[k], c.unconstrained[k]), k
    # continuing a run in two calls is the same as one call
    d = engine.HipSVI("MixtureNormal", data, num_steps=500)
    d.run(15, seed=9, graph_chunk=4)
    d.run(n - 15, seed=9, graph_chunk=4)
    for k in a.unconstrained:
        assert torch.equal(b.unconstrained[k], d.unconstrained[k]), k
    for e in (a, b, c, d):
        e.close()


def test_run_inference_interface(engine):
    from functools import partial

    from bean_amd.model import model as m
    from bean_amd.model.run import run_inference

    data = make_sorting_variant_screen(500, 2, seed=73, frac_effect=0.5)
    store, out = run_inference(
        partial(m.MixtureNormalModel, use_bcmatch=(True,)), partial(m.MixtureNormalGuide, fit_noise=True),
        data, num_steps=300, verbose=False)
    assert set(store.keys()) == {"mu_loc", "mu_scale", "sd_loc", "sd_scale", "alpha_pi"}
    assert "mu_loc" in store.keys() and store["mu_loc"].dim() == 2
    assert len(out["loss"]) == 300 and isinstance(out["loss"][0], float)
    assert out["loss"][-1] < 0.8 * out["loss"][0]
    assert (store["mu_scale"] > 0).all() and (store["alpha_pi"] > 0).all()
    assert out["params"]["mu_loc"].device.type == "cpu"
    mu = out["params"]["mu_loc"].numpy().ravel()
    truth = data.truth["mu"]
    big = np.abs(truth) > 0.8
    assert np.mean(np.sign(mu[big]) == np.sign(truth[big])) > 0.8


# --------------------------------------------------- full-size (metric shape) properties
@pytest.fixture(scope="module")
def full_screen():
    return make_sorting_variant_screen(50_000, 5, seed=20240502)


def test_full_size_shard_additivity(engine, full_screen):
    """Loss and per-guide gradients of the whole 50k-guide screen equal those of
    two target-aligned shards evaluated on the same draws (guides shard without
    any data-path exchange)."""
    data = full_screen
    T, G, R = data.n_targets, data.n_guides, data.n_reps
    whole = engine.HipSVI("MixtureNormal", data.to(DEV), dump_noise=True, num_steps=10)
    loss, grads = whole.elbo_grad(step=0, seed=3)
    noise = whole.drawn_noise()
    cut_t = T // 3
    cut_g = int(data.target_offsets[cut_t])
    tot = 0.0
    for (g0, g1, t0, t1) in ((0, cut_g, 0, cut_t), (cut_g, G, cut_t, T)):
        sub = data[np.arange(g0, g1)]
        e = engine.HipSVI("MixtureNormal", sub.to(DEV), num_steps=10)
        e.set_noise({"eps_mu": noise["eps_mu"][t0:t1], "eps_sd": noise["eps_sd"][t0:t1],
                     "pi": noise["pi"][:, :, g0:g1]})
        l, g = e.elbo_grad()
        tot += l
        assert torch.equal(g["alpha_pi"], grads["alpha_pi"][g0:g1])
        assert torch.equal(g["mu_loc"], grads["mu_loc"][t0:t1])
        assert torch.equal(g["sd_scale"], grads["sd_scale"][t0:t1])
        e.close()
    assert abs(tot - loss) <= 1e-11 * abs(loss)
    whole.close()


def test_full_size_fit_is_deterministic_and_improves(engine, full_screen):
    data = full_screen.to(DEV)
    runs = []
    for _ in range(2):
        e = engine.HipSVI("MixtureNormal", data, num_steps=2000)
        e.run(200, seed=101)
        runs.append(({k: v.clone() for k, v in e.unconstrained.items()}, e.losses()))
        e.close()
    for k in runs[0][0]:
        assert torch.equal(runs[0][0][k], runs[1][0][k]), k
    losses = runs[0][1]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    np.testing.assert_allclose(runs[0][1], runs[1][1], rtol=1e-12)  # atomically summed, not bitwise


@pytest.mark.parametrize("gen_kw,acc,n_shards", [
    (dict(n_guides=1000, n_reps=3, with_accessibility=True), True, 3),
    # targets of 100 guides: every target spans two or three 64-guide tiles, and the tiles of a shard start
    # wherever its first target does - the per-target sums are cut on the GLOBAL guide index (bean_guide_v2.hpp)
    (dict(n_guides=7000, n_reps=3, guides_per_target=100), False, 3),
    (dict(n_guides=3200, n_reps=2, guides_per_target=7), False, 5),   # 457 targets, shards of ~91 targets
    (dict(n_guides=900, n_reps=2, guides_per_target=300), False, 3),  # three targets: one block per target
])
def test_sharded_engines_reproduce_the_whole_screen_fit(engine, gen_kw, acc, n_shards):
    """Target-aligned shards fitted separately with their global offsets
    reproduce the single-engine fit bit for bit (what makes the N-GPU run
    independent of N)."""
    from bean_amd import parallel

    data = make_sorting_variant_screen(seed=81, **gen_kw)
    kw = dict(scale_by_accessibility=True, num_steps=300) if acc else dict(num_steps=300)
    whole = engine.HipSVI("MixtureNormal", data.to(DEV), **kw)
    whole.run(60, seed=5)
    ref = whole.constrained()
    ref_losses = np.array(whole.losses())
    shards = parallel.plan_shards(data.target_lengths.numpy(), n_shards)
    assert any(sh[0] % 64 for sh in shards)  # a shard that does not start on a tile boundary
    parts, losses = [], np.zeros(60)
    for sh in shards:
        e = engine.HipSVI("MixtureNormal", parallel.shard_screen(data, sh).to(DEV), guide_offset=sh[0],
                          target_offset=sh[2], n_guides_total=data.n_guides, **kw)
        e.run(60, seed=5)
        parts.append(e.constrained())
        losses += np.array(e.losses())
        e.close()
    for k in ref:
        got = torch.cat([p[k] for p in parts], dim=0)
        assert torch.equal(got, ref[k]), k
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-12)
    whole.close()


# ------------------------------------------------------------------- tiling
from bean_amd.preprocessing.synthetic import make_sorting_tiling_screen  # noqa: E402


def _compare_tiling(engine, data, kw, seed=7, step=2):
    torch.manual_seed(seed)
    eng = engine.HipSVI("MultiMixtureNormal", data.to(DEV), dump_noise=True, num_steps=50, **kw)
    for k, v in eng.unconstrained.items():
        noise = 0.3 * torch.randn_like(v)
        if k == "alpha_pi":  # masked alleles keep their fixed log(eps) storage
            noise = noise * data.allele_mask.to(DEV)
        v.add_(noise)
    loss, grads = eng.elbo_grad(step=step, seed=seed)
    draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    # (float64 mode is the parity statement.  "ref" runs the oracle in the reference's float32 / float64 mix; where
    # that mix is itself further from the float64 oracle than the band - ill-conditioned parameter points, seen in
    # 3 of 480 random shapes at up to 3e-4 - the kernels are asked to be as close to it as three times that)
    ref64 = {}
    for mode, tl, tg in (("f64", 1e-9, 5e-7), ("ref", 1e-6, 2e-5)):
        params = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
        d = data
        if mode == "f64":
            params = {k: v.double() for k, v in params.items()}
            d = elbo.as_float64(data)
        params = {k: v.requires_grad_(True) for k, v in params.items()}
        ref_loss, ref_grads, _ = svi.loss_and_grads(elbo.multi_mixture_normal_loss, d, params, noise=draws, **kw)
        assert abs(loss - ref_loss) <= tl * abs(ref_loss), (mode, loss, ref_loss)
        for k, g in grads.items():
            ref = ref_grads[k].double().reshape(-1)
            err = (g.cpu().double().reshape(-1) - ref).abs().max().item()
            own = 0.0
            if mode == "f64":
                ref64[k] = ref
            else:
                own = 3.0 * (ref - ref64[k]).abs().max().item()
            assert err <= tg * (ref.abs().max().item() + 1e-30) + own, (mode, k, err)
    # gradient of masked alleles' alpha is exactly zero (in-place write at model.py:645)
    assert torch.all(grads["alpha_pi"][~data.allele_mask.to(DEV)] == 0)
    eng.set_noise(draws)
    loss_b, grads_b = eng.elbo_grad(step=step, seed=seed)
    assert abs(loss_b - loss) <= 1e-12 * abs(loss)
    for k in grads:
        assert torch.equal(grads[k], grads_b[k])
    eng.close()


@pytest.mark.parametrize("gen_kw,kw", [
    (dict(n_guides=500, n_reps=3, mask_fraction=0.05), {}),
    (dict(n_guides=300, n_reps=2, with_accessibility=True, n_max_alleles=5), dict(scale_by_accessibility=True)),
    (dict(n_guides=130, n_reps=9, n_max_alleles=3), {}),
    (dict(n_guides=65, n_reps=1, n_max_alleles=2), {}),
    (dict(n_guides=200, n_reps=2, n_max_alleles=8, bins=((0.0, 0.3), (0.3, 1.0))), {}),
    (dict(n_guides=150, n_reps=2, n_max_alleles=13), {}),  # > 8 alleles per guide: the 16-allele build
    (dict(n_guides=120, n_reps=2, n_max_alleles=4,
          bins=tuple((i / 10, (i + 1) / 10) for i in range(10))), {}),  # 10 bins + bulk
    (dict(n_guides=100, n_reps=3, n_max_alleles=16, with_accessibility=True), dict(scale_by_accessibility=True)),
    (dict(n_guides=80, n_reps=2, n_max_alleles=4,
          bins=tuple((i / 20, (i + 1) / 20) for i in range(20))), {}),  # 20 bins + bulk (> 16 conditions)
    (dict(n_guides=70, n_reps=2, n_max_alleles=6, with_accessibility=True,
          bins=tuple((i / 31, (i + 1) / 31) for i in range(31))), dict(scale_by_accessibility=True)),  # 32 conditions, > 64 KB LDS
    (dict(n_guides=70, n_reps=2, n_max_alleles=5,
          bins=tuple((i / 39, (i + 1) / 39) for i in range(39))), {}),  # 40 conditions (the reference has no bound)
])
def test_tiling_elbo_and_gradients_match_oracle(engine, gen_kw, kw):
    data = make_sorting_tiling_screen(seed=4, **gen_kw)
    _compare_tiling(engine, data, kw)


def test_tiling_masked_alleles_that_keep_their_edits(engine):
    """k_allele fills the slots whose mask is set OR whose edit list is not empty (the work list of
    bean_hip_prepare): alleles masked out AFTER the table was built keep their edits - mu_a of such a slot is
    still formed, its bin probabilities are 0 - and slots with neither stay at the zeros they start from."""
    data = make_sorting_tiling_screen(400, 3, seed=31, n_max_alleles=7)
    g = torch.Generator().manual_seed(5)
    drop = (torch.rand(data.allele_mask.shape, generator=g) < 0.15) & data.allele_mask
    drop[:, 0] = False  # the unedited allele stays
    data.allele_mask = data.allele_mask & ~drop
    assert int(drop.sum()) > 100
    _compare_tiling(engine, data, {})


def test_tiling_screen_built_from_h5ad_matches_oracle(engine):
    """The reference's tiling mini-screen file through the .h5ad reader and the allele-table
    builder, then ELBO + gradients against the oracle on the same tensors."""
    import warnings

    from bean_amd.framework import h5ad_io, read_h5ad
    from bean_amd.preprocessing.screen_data import DATACLASS_DICT

    assert os.path.exists(h5ad_io.HELPER_PYTHON), "no h5py helper interpreter: .h5ad screens cannot be read here"
    s = read_h5ad(os.path.join(os.path.dirname(__file__), "golden", "tiling_mini_screen.h5ad"))
    s.samples["replicate"] = s.samples["replicate"].astype(str)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        data = DATACLASS_DICT["sorting"]["MultiMixtureNormal"](
            s, sample_mask_column=None, allele_df_key="allele_counts", control_condition="bulk")
    # the unfiltered table: up to 230 edited alleles per guide, kept as they are and fitted by the
    # allele-parallel kernels (csrc/bean_tiling_wide.hpp)
    assert data.n_max_alleles == 231 and data.n_guides == 30 and data.n_alleles_dropped == 0
    _compare_tiling(engine, data, {})


@pytest.mark.parametrize("gen_kw,kw,kernel", [
    # 17 ... 32 alleles per guide: the 32-allele build of the register-resident kernels (libbean_hip_a32.so)
    (dict(n_guides=150, n_reps=3, n_max_alleles=20, mask_fraction=0.05), {}, "k_guide_tiling_rep"),
    (dict(n_guides=65, n_reps=1, n_max_alleles=17, bins=tuple((i / 10, (i + 1) / 10) for i in range(10))), {},
     "k_guide_tiling_rep"),
    (dict(n_guides=90, n_reps=2, n_max_alleles=32, with_accessibility=True), dict(scale_by_accessibility=True),
     "k_guide_tiling_rep"),
    # more: the allele-parallel path (one wave per (replicate, guide), lanes over alleles)
    (dict(n_guides=70, n_reps=2, n_max_alleles=40, with_accessibility=True), dict(scale_by_accessibility=True),
     "k_guide_tiling_wide"),
    (dict(n_guides=40, n_reps=2, n_max_alleles=100), {}, "k_guide_tiling_wide"),  # two alleles per lane
    (dict(n_guides=60, n_reps=3, n_max_alleles=33, mask_fraction=0.05), {}, "k_guide_tiling_wide"),
    # more than 256 alleles per guide: eight alleles per lane, the 16-allele build's copy of the kernels
    (dict(n_guides=24, n_reps=2, n_max_alleles=300), {}, "k_guide_tiling_wide"),
    (dict(n_guides=20, n_reps=2, n_max_alleles=512, with_accessibility=True), dict(scale_by_accessibility=True),
     "k_guide_tiling_wide"),
])
def test_wide_tiling_matches_oracle(engine, gen_kw, kw, kernel):
    """More alleles per guide than the default builds hold (8, 16), against the same oracle."""
    data = make_sorting_tiling_screen(seed=14, **gen_kw)
    assert data.n_max_alleles == gen_kw["n_max_alleles"]
    probe = engine.HipSVI("MultiMixtureNormal", data.to(DEV), num_steps=10, **kw)
    assert probe.dominant_kernel == kernel
    probe.close()
    _compare_tiling(engine, data, kw)


@pytest.mark.parametrize("n_al,kernel", [(24, "k_guide_tiling_rep"), (48, "k_guide_tiling_wide")])
def test_wide_tiling_trajectory_fused_loop_and_shards(engine, n_al, kernel):
    data = make_sorting_tiling_screen(120, 2, seed=15, n_max_alleles=n_al)
    n = 12
    eng = engine.HipSVI("MultiMixtureNormal", data.to(DEV), dump_noise=True, num_steps=2000)
    assert eng.dominant_kernel == kernel
    params = elbo.init_params("MultiMixtureNormal", data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    for t in range(n):
        loss, _ = eng.elbo_grad(step=t, seed=5, loss_index=t)
        draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        eng.adam(t + 1)
        ref = svi.svi_step(elbo.multi_mixture_normal_loss, data, params, optim, noise=draws)
        assert abs(loss - ref) <= 2e-6 * abs(ref), (t, loss, ref)
    torch.cuda.synchronize()
    for k, v in eng.unconstrained.items():
        ref = params[k].detach()
        err = (v.cpu() - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (k, err)
    fused = engine.HipSVI("MultiMixtureNormal", data.to(DEV), num_steps=2000)
    fused.run(n, seed=5, graph_chunk=4)
    for k in eng.unconstrained:
        assert torch.equal(eng.unconstrained[k], fused.unconstrained[k]), k
    longer = engine.HipSVI("MultiMixtureNormal", data.to(DEV), num_steps=300)
    longer.run(300)
    ls = longer.losses()
    assert np.isfinite(ls).all() and ls[-1] < ls[0]
    for e in (eng, fused, longer):
        e.close()


def test_tiling_trajectory_and_fused_loop(engine):
    data = make_sorting_tiling_screen(250, 2, seed=6, n_max_alleles=6)
    n = 20
    eng = engine.HipSVI("MultiMixtureNormal", data.to(DEV), dump_noise=True, num_steps=2000)
    params = elbo.init_params("MultiMixtureNormal", data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    for t in range(n):
        loss, _ = eng.elbo_grad(step=t, seed=5, loss_index=t)
        draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        eng.adam(t + 1)
        ref = svi.svi_step(elbo.multi_mixture_normal_loss, data, params, optim, noise=draws)
        assert abs(loss - ref) <= 2e-6 * abs(ref), (t, loss, ref)
    torch.cuda.synchronize()
    for k, v in eng.unconstrained.items():
        ref = params[k].detach()
        err = (v.cpu() - ref).abs().max().item()
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (k, err)
    fused = engine.HipSVI("MultiMixtureNormal", data.to(DEV), num_steps=2000)
    fused.run(n, seed=5, graph_chunk=6)
    for k in eng.unconstrained:
        assert torch.equal(eng.unconstrained[k], fused.unconstrained[k]), k
    np.testing.assert_allclose(fused.losses(), eng.loss_hist[:n].cpu().tolist(), rtol=1e-12)
    eng.close()
    fused.close()


def test_tiling_run_inference_recovers_edit_effects(engine):
    from types import SimpleNamespace

    from bean_amd.model.run import identify_model_guide, run_inference

    args = SimpleNamespace(selection="sorting", library_design="tiling", scale_by_acc=False,
                           ignore_bcmatch=False, dont_fit_noise=False, uniform_edit=False, const_pi=False,
                           guide_activity_col=None)
    label, model, guide = identify_model_guide(args)
    assert label == "MultiMixtureNormal"
    data = make_sorting_tiling_screen(2000, 3, seed=8)
    store, out = run_inference(model, guide, data, num_steps=400, verbose=False)
    assert store["mu_loc"].shape == (data.n_edits,) and store["alpha_pi"].shape == (2000, 8)
    assert out["loss"][-1] < 0.8 * out["loss"][0]
    mu, truth = out["params"]["mu_loc"].numpy(), data.truth["mu_edits"]
    big = np.abs(truth) > 1.0
    assert big.sum() > 10 and np.mean(np.sign(mu[big]) == np.sign(truth[big])) > 0.8


# ------------------------------------------------------------------ survival
from bean_amd.preprocessing.synthetic import make_survival_variant_screen  # noqa: E402
from oracle import survival as osurv  # noqa: E402


def _compare_survival(engine, family, data, kw, seed=7, step=2):
    torch.manual_seed(seed)
    eng = engine.HipSVI(family, data.to(DEV), dump_noise=True, num_steps=50, **kw)
    for v in eng.unconstrained.values():
        v.add_(0.3 * torch.randn_like(v))
    loss, grads = eng.elbo_grad(step=step, seed=seed)
    draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    # (float64 mode is the parity statement.  "ref" runs the oracle in the reference's float32 / float64 mix: its own
    # rounding against float64 is 1e-6 ... 3e-6 of the loss for the survival NormalModel - 2 of 1 200 random shapes
    # were above 2e-6 - hence 5e-6 there)
    for mode, tl, tg in (("f64", 1e-9, 5e-7), ("ref", 5e-6, 2e-5)):
        params = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
        d = data
        if mode == "f64":
            params = {k: v.double() for k, v in params.items()}
            d = elbo.as_float64(data)
        params = {k: v.requires_grad_(True) for k, v in params.items()}
        ref_loss, ref_grads, _ = svi.loss_and_grads(osurv.LOSSES[family], d, params, noise=draws, **kw)
        # (the reference's float32 terms do not shrink with the total: on a screen of a hundred guides, whose loss is
        # a few thousand, their rounding is what 2e-6 of a loss of 3e4 is - seen once in 96 random shapes)
        scale = abs(ref_loss) if mode == "f64" else max(abs(ref_loss), 3e4)
        assert abs(loss - ref_loss) <= tl * scale, (mode, loss, ref_loss)
        for k, g in grads.items():
            ref = ref_grads[k].double().reshape(-1)
            err = (g.cpu().double().reshape(-1) - ref).abs().max().item()
            # torch evaluates the implicit gradient of the float32 Dirichlet(q0) site in float32 (the float64
            # pass above holds the same gradient to 5e-7; 2.1e-4 at 2 600 guides)
            tol = 3e-4 if (k in ("q0", "initial_abundance") and mode == "ref") else tg
            assert err <= tol * (ref.abs().max().item() + 1e-30), (mode, k, err)
    eng.set_noise(draws)
    loss_b, grads_b = eng.elbo_grad(step=step, seed=seed)
    assert abs(loss_b - loss) <= 1e-12 * abs(loss)
    for k in grads:
        assert torch.equal(grads[k], grads_b[k]), k
    eng.close()


@pytest.mark.parametrize("gen_kw,kw", [
    (dict(n_guides=700, n_reps=3, mask_fraction=0.05), {}),
    (dict(n_guides=400, n_reps=2, with_accessibility=True), dict(scale_by_accessibility=True)),
    (dict(n_guides=130, n_reps=9, times=(0.0, 7.0, 14.0)), {}),
    (dict(n_guides=300, n_reps=2), dict(mu_negctrl=(0.05, 0.2))),
    (dict(n_guides=65, n_reps=1, times=(0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0)), {}),
    (dict(n_guides=120, n_reps=2, times=tuple(float(t) for t in range(0, 22, 2))), {}),  # 11 timepoints
    (dict(n_guides=90, n_reps=2, times=tuple(float(t) for t in range(0, 23))), {}),  # 23 timepoints (> 16)
    (dict(n_guides=90, n_reps=2, times=tuple(0.5 * t for t in range(0, 40))), {}),  # 40 timepoints (> 32)
    # 37 guides x 4 replicates = 148 rows per target: k_param's 4 lanes per target loop over them ten times
    (dict(n_guides=2600, n_reps=4, guides_per_target=37), {}),
])
def test_survival_mixture_matches_oracle(engine, gen_kw, kw):
    data = make_survival_variant_screen(seed=4, **gen_kw)
    assert data.n_condits == len(gen_kw.get("times", range(6)))
    _compare_survival(engine, "MixtureNormal", data, kw)


def test_survival_control_normal_matches_oracle(engine):
    data = make_survival_variant_screen(3000, 3, seed=5)
    _compare_survival(engine, "ControlNormal", data[data.negctrl_guide_idx], {})


@pytest.mark.parametrize("gen_kw,drop_idx", [
    (dict(n_guides=700, n_reps=3, mask_fraction=0.05), False),
    (dict(n_guides=130, n_reps=5, times=(0.0, 7.0, 14.0)), False),
    (dict(n_guides=65, n_reps=1), False),
    (dict(n_guides=300, n_reps=2), True),
])
def test_survival_normal_matches_oracle(engine, gen_kw, drop_idx):
    """survival NormalModel (--uniform-edit): the Dirichlet-over-guides draw q_0 multiplies the growth
    term, negative-control guides have mu forced to 0; without an index the reference's
    `mu[None, :] = 0.0` zeroes every guide, which is kept."""
    data = make_survival_variant_screen(seed=8, **gen_kw)
    if drop_idx:
        data.negctrl_guide_idx = None
    _compare_survival(engine, "Normal", data, {})


def test_survival_normal_with_initial_abundance_prior(engine):
    """prior_params["initial_abundance"] (survival_model.py:38-49): a per-guide prior concentration of the
    Dirichlet-over-guides site instead of ones / G."""
    data = make_survival_variant_screen(400, 3, seed=10)
    g = torch.Generator().manual_seed(2)
    prior = {"initial_abundance": (torch.rand(400, generator=g) + 0.2) / 400,
             "mu_loc": torch.randn((data.n_targets, 1), generator=g) * 0.1,
             "mu_scale": torch.rand((data.n_targets, 1), generator=g) + 0.5}
    _compare_survival(engine, "Normal", data, dict(prior_params=prior))


def test_survival_normal_trajectory_and_fused_loop(engine):
    data = make_survival_variant_screen(600, 3, seed=9, frac_effect=0.5)
    n = 12
    eng = engine.HipSVI("Normal", data.to(DEV), dump_noise=True, num_steps=2000)
    params = osurv.init_params("Normal", data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    for t in range(n):
        loss, _ = eng.elbo_grad(step=t, seed=5, loss_index=t)
        draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        eng.adam(t + 1)
        ref = svi.svi_step(osurv.normal_loss, data, params, optim, noise=draws)
        assert abs(loss - ref) <= 5e-6 * abs(ref), (t, loss, ref)
    torch.cuda.synchronize()
    for k, v in eng.unconstrained.items():
        ref = params[k].detach()
        err = (v.cpu() - ref).abs().max().item()
        assert err <= 2e-4 * max(1.0, ref.abs().max().item()), (k, err)
    fused = engine.HipSVI("Normal", data.to(DEV), num_steps=2000)
    fused.run(n, seed=5, graph_chunk=4)
    for k in eng.unconstrained:
        assert torch.equal(eng.unconstrained[k], fused.unconstrained[k]), k
    longer = engine.HipSVI("Normal", data.to(DEV), num_steps=300)
    longer.run(300)
    torch.cuda.synchronize()
    ls = longer.losses()
    assert np.isfinite(ls).all() and ls[-1] < ls[0]
    for e in (eng, fused, longer):
        e.close()


def test_survival_trajectory_fused_loop_and_interface(engine):
    from types import SimpleNamespace

    from bean_amd.model.run import identify_model_guide, identify_negctrl_model_guide, run_inference

    data = make_survival_variant_screen(800, 3, seed=6, frac_effect=0.5)
    n = 15
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), dump_noise=True, num_steps=2000)
    params = osurv.init_params("MixtureNormal", data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    for t in range(n):
        loss, _ = eng.elbo_grad(step=t, seed=5, loss_index=t)
        draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        eng.adam(t + 1)
        ref = svi.svi_step(osurv.mixture_normal_loss, data, params, optim, noise=draws)
        assert abs(loss - ref) <= 5e-6 * abs(ref), (t, loss, ref)
    torch.cuda.synchronize()
    for k, v in eng.unconstrained.items():
        ref = params[k].detach()
        err = (v.cpu() - ref).abs().max().item()
        assert err <= 2e-4 * max(1.0, ref.abs().max().item()), (k, err)
    fused = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=2000)
    fused.run(n, seed=5, graph_chunk=4)
    for k in eng.unconstrained:
        assert torch.equal(eng.unconstrained[k], fused.unconstrained[k]), k
    eng.close()
    fused.close()
    # the bean run sequence for survival: neg-ctrl fit feeds mu_negctrl into the main model
    args = SimpleNamespace(selection="survival", library_design="variant", scale_by_acc=False,
                           ignore_bcmatch=False, dont_fit_noise=False, uniform_edit=False, const_pi=False,
                           guide_activity_col=None)
    label, model, guide = identify_model_guide(args)
    nm, ng = identify_negctrl_model_guide(args, True)
    assert label == "MixtureNormal"
    store_n, _ = run_inference(nm, ng, data[data.negctrl_guide_idx], num_steps=200, verbose=False)
    from functools import partial
    model = partial(model, mu_negctrl=(store_n["mu_loc"].detach().mean(), store_n["mu_scale"].detach().mean()))
    store, out = run_inference(model, guide, data, num_steps=400, verbose=False)
    assert set(store.keys()) == {"mu_loc", "mu_scale", "alpha_pi", "q0"}
    assert out["loss"][-1] < out["loss"][0]
    mu, truth = out["params"]["mu_loc"].numpy().ravel(), data.truth["mu"]
    big = np.abs(truth) > 1.0
    assert big.sum() > 5 and np.mean(np.sign(mu[big]) == np.sign(truth[big])) > 0.8


# ---------------------------------------------------------- tiling survival
from bean_amd.preprocessing.synthetic import make_survival_tiling_screen  # noqa: E402


def _compare_survival_tiling(engine, data, kw, seed=7, step=2):
    torch.manual_seed(seed)
    eng = engine.HipSVI("MultiMixtureNormal", data.to(DEV), dump_noise=True, num_steps=50, **kw)
    for k, v in eng.unconstrained.items():
        noise = 0.3 * torch.randn_like(v)
        if k == "alpha_pi":
            noise = noise * data.allele_mask.to(DEV)
        v.add_(noise)
    loss, grads = eng.elbo_grad(step=step, seed=seed)
    draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    assert set(draws) >= {"eps_mu", "pi", "mu_negctrl"}
    for mode, tl, tg in (("f64", 1e-9, 5e-7), ("ref", 2e-6, 2e-5)):
        params = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
        d = data
        if mode == "f64":
            params = {k: v.double() for k, v in params.items()}
            d = elbo.as_float64(data)
        params = {k: v.requires_grad_(True) for k, v in params.items()}
        ref_loss, ref_grads, _ = svi.loss_and_grads(osurv.multi_mixture_normal_loss, d, params, noise=draws, **kw)
        assert abs(loss - ref_loss) <= tl * abs(ref_loss), (mode, loss, ref_loss)
        for k, g in grads.items():
            ref = ref_grads[k].double().reshape(-1)
            err = (g.cpu().double().reshape(-1) - ref).abs().max().item()
            assert err <= tg * (ref.abs().max().item() + 1e-30), (mode, k, err)
    assert torch.all(grads["alpha_pi"][~data.allele_mask.to(DEV)] == 0)
    eng.close()


@pytest.mark.parametrize("gen_kw,kw", [
    (dict(n_guides=400, n_reps=3, mask_fraction=0.05), {}),
    (dict(n_guides=300, n_reps=2, with_accessibility=True, n_max_alleles=5), dict(scale_by_accessibility=True)),
    (dict(n_guides=130, n_reps=4, n_max_alleles=3, times=(0.0, 3.0, 6.0, 9.0, 12.0)), {}),
    (dict(n_guides=200, n_reps=2, n_max_alleles=8), dict(mu_negctrl=(0.05, 0.2))),
    (dict(n_guides=90, n_reps=2, n_max_alleles=30), {}),  # the 32-allele build
    (dict(n_guides=80, n_reps=2, n_max_alleles=45, with_accessibility=True), dict(scale_by_accessibility=True)),  # allele-parallel path
])
def test_survival_tiling_matches_oracle(engine, gen_kw, kw):
    data = make_survival_tiling_screen(seed=11, **gen_kw)
    _compare_survival_tiling(engine, data, kw)


def test_survival_tiling_trajectory_fused_loop_and_store(engine):
    from functools import partial

    from bean_amd.model import survival_model as vm
    from bean_amd.model.run import run_inference

    data = make_survival_tiling_screen(250, 2, seed=12, n_max_alleles=6)
    n = 12
    eng = engine.HipSVI("MultiMixtureNormal", data.to(DEV), dump_noise=True, num_steps=2000)
    params = osurv.init_params("MultiMixtureNormal", data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    for t in range(n):
        loss, _ = eng.elbo_grad(step=t, seed=5, loss_index=t)
        draws = {k: v.cpu() for k, v in eng.drawn_noise().items()}
        eng.adam(t + 1)
        ref = svi.svi_step(osurv.multi_mixture_normal_loss, data, params, optim, noise=draws)
        assert abs(loss - ref) <= 5e-6 * abs(ref), (t, loss, ref)
    torch.cuda.synchronize()
    for k, v in eng.unconstrained.items():
        ref = params[k].detach()
        err = (v.cpu() - ref).abs().max().item()
        assert err <= 2e-4 * max(1.0, ref.abs().max().item()), (k, err)
    fused = engine.HipSVI("MultiMixtureNormal", data.to(DEV), num_steps=2000)
    fused.run(n, seed=5, graph_chunk=4)
    for k in eng.unconstrained:
        assert torch.equal(eng.unconstrained[k], fused.unconstrained[k]), k
    eng.close()
    fused.close()
    store, out = run_inference(partial(vm.MultiMixtureNormalModel), partial(vm.MultiMixtureNormalGuide), data,
                               num_steps=150, verbose=False)
    # the reference's guide registers an unused `initial_abundance` parameter: it stays 1 / G
    assert set(store.keys()) == {"mu_loc", "mu_scale", "alpha_pi", "initial_abundance"}
    assert torch.allclose(store["initial_abundance"].cpu(), torch.full((250,), 1 / 250))
    assert np.isfinite(out["loss"]).all() and out["loss"][-1] < out["loss"][0]


# ------------------------------------------------- total term of the Dirichlet-Multinomial sites
@pytest.mark.parametrize("which", ["variant", "variant_masked", "survival", "survival_masked", "tiling"])
def test_total_term_as_constant_equals_evaluating_it(engine, which, monkeypatch):
    """get_alpha normalises (utils.py:10-31): without a floored bin sum_b alpha_b = a0[g] is data, so the
    kernels leave lgamma(A0 + n) - lgamma(A0) to the constant (DevArgs::tot_const) and add the difference
    where a bin sits on its floor (masked samples).  BEAN_HIP_TOT_CONST=0 evaluates it every step."""
    from bean_amd.preprocessing.synthetic import make_sorting_tiling_screen

    if which.startswith("variant"):
        data = make_sorting_variant_screen(1500, 3, seed=91, mask_fraction=0.05 if which.endswith("masked") else 0.0)
        family = "MixtureNormal"
    elif which.startswith("survival"):
        data = make_survival_variant_screen(1500, 3, seed=92, mask_fraction=0.05 if which.endswith("masked") else 0.0)
        family = "MixtureNormal"
    else:
        data = make_sorting_tiling_screen(600, 2, seed=93)
        family = "MultiMixtureNormal"
    if which.endswith("masked"):
        assert (data.sample_mask == 0).any()
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("BEAN_HIP_TOT_CONST", flag)
        torch.manual_seed(3)
        eng = engine.HipSVI(family, data.to(DEV), num_steps=20)
        for v in eng.unconstrained.values():
            v.add_(0.3 * torch.randn_like(v))
        out[flag] = eng.elbo_grad(step=2, seed=11)
        eng.close()
    (l1, g1), (l0, g0) = out["1"], out["0"]
    assert abs(l1 - l0) <= 1e-12 * abs(l0), (l1, l0)
    for k in g0:
        scale = g0[k].abs().max().item() + 1e-30
        assert (g1[k] - g0[k]).abs().max().item() <= 2e-6 * scale, k  # float32 outputs: a few ulp
