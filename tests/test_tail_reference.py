"""The Gauss-Jacobi rule for the pairs section 21's predicate leaves out, on the CPU in float64:
its nodes against Beta-function ratios, the rule against a 160-node rule and against QUADPACK, where it checks itself and
where it refuses - the table of section 23 is this file's output."""
import math

import numpy as np
import pytest
import torch

from bean_amd.preprocessing.synthetic import make_sorting_variant_screen
from oracle import elbo

import marginal_reference as mr
import tail_common as tc
import tail_reference as tr
from members_common import _mini
from test_marginal_reference import BOUND, ROWS, _override

SETTINGS = ((0.0, 1.0), (0.5, 1.0), (2.0, 1.3), (-3.0, 0.7))  # (mu, sd) of every target
# the unresolved rows of test_marginal_reference.ROWS, and three more of the same kind
TABLE = [(cp, counts) for cp, counts, ok in ROWS if not ok] + [((5.0, 0.01), (1000.0, 0.0)), ((0.5, 0.5), (0.0, 0.0)),
                                                                ((0.08, 0.08), (0.0, 0.0))]
CONFLICT = ((0.08, 40.0), (0.0, 300.0))  # the Beta factor puts its mass where the sorting counts put none


@pytest.fixture(scope="module")
def first_target():
    screen = make_sorting_variant_screen(40, 3, seed=3)
    return elbo.as_float64(screen[list(range(int(screen.target_offsets[0]), int(screen.target_offsets[1])))])


@pytest.fixture(scope="module")
def fixture_with_emulated_rates(tmp_path_factory):
    """tests/golden/var_mini_screen.h5ad with alpha_pi = (log 4, log 1/32) on the guides whose a1' is then small: the
    editing rates a fit reaches there, emulated."""
    data = _mini(tmp_path_factory.mktemp("mini"))
    alpha = elbo.init_params("MixtureNormal", data)["alpha_pi"].detach().clone().reshape(data.n_guides, 2).float()
    unedited = torch.tensor(tc.UNEDITED)
    trial = mr.model_conc(data, {"alpha_pi": unedited.expand(data.n_guides, 2)})
    small = (mr.beta_exponents(elbo.as_float64(data), trial)[..., 1] < mr.MARG_MIN_CONC).any(0)
    alpha[small] = unedited
    return data, alpha


def _log_beta(a, b):
    return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)


@pytest.mark.parametrize("a,b", [(425.0, 0.064), (440.0, 0.08), (40.0, 1.0), (1.0, 1.0), (0.08, 0.08), (1000.0, 1.99)])
def test_nodes_integrate_monomials_against_beta_ratios(a, b):
    """int z^k w(z) dz / int w(z) dz = B(b + k, a) / B(b, a): exact for k <= 2 Q - 1.  1e-10 relative: the moments are
    sums of Q positive terms of nodes and weights that carry the eigensolver's and the recurrence's rounding, a few
    hundred eps each at the exponents of a deep guide (measured 1.2e-12 at worst)."""
    for Q in (tr.TAIL_CHECK_NODES, tr.TAIL_NODES, 160):
        z, lw = tr.gauss_jacobi(a, b, Q)
        assert z.shape == (Q,) and bool((np.diff(z) > 0).all()) and z[0] > 0 and z[-1] < 1
        w = np.exp(lw)
        worst = 0.0
        for k in (0, 1, 2, 5, 20, Q, 2 * Q - 1):
            want = math.exp(_log_beta(b + k, a) - _log_beta(b, a))
            worst = max(worst, abs(float((w * z ** k).sum()) / want - 1.0))
        print(f"a = {a}, b = {b}, Q = {Q}: smallest node {z[0]:.3e}; largest relative error of a moment {worst:.1e}")
        assert worst < 1e-10


def _jacobi_errors(data, c_p, ctrl, nodes=(32, 48, 64), ref_nodes=160, with_today=True):
    """Largest |rule - the ref_nodes-node Jacobi rule| over the pairs under the repguide mask and the SETTINGS, per Q;
    the same of today's rule at Q = 64; and the largest |J64 - J48|."""
    a_prime = mr.beta_exponents(data, c_p, ctrl)
    worst = {Q: 0.0 for Q in nodes}
    today = check = 0.0
    rg = data.repguide_mask
    for mu, sd in SETTINGS:
        T = data.n_targets
        h = mr.PairIntegrand(data, torch.full((T,), mu), torch.full((T,), sd), c_p, ctrl=ctrl)
        want = tr.jacobi_rule(h, a_prime, ref_nodes)
        assert bool(torch.isfinite(want[rg]).all())
        J = {Q: tr.jacobi_rule(h, a_prime, Q) for Q in nodes}
        for Q in nodes:
            worst[Q] = max(worst[Q], float((J[Q] - want).abs()[rg].max()))
        check = max(check, float((J[64] - J[48]).abs()[rg].max()))
        if with_today:
            today = max(today, float((mr.mode_centred_rule(h, a_prime, 64) - want).abs()[rg].max()))
    return worst, today, check


@pytest.mark.parametrize("row", TABLE, ids=lambda r: f"cp={r[0]}-counts={r[1]}")
def test_rule_on_the_unresolved_rows(first_target, row):
    """One target's 15 pairs with c_p and the control counts set by hand, at four (mu, sd): Q = 64 is within section
    21's BOUND of the 160-node rule, and the rule's own check |J64 - J48| is below BOUND."""
    cp, counts = row
    c_p, ctrl = _override(first_target, cp, counts)
    assert not bool(mr.resolved(first_target, c_p, ctrl).any())
    w, today, check = _jacobi_errors(first_target, c_p, ctrl)
    print(f"c_p = {cp}, control counts {counts}: " + " | ".join(f"Jacobi Q = {Q}: {e:.1e}" for Q, e in w.items())
          + f" | today's rule, Q = 64: {today:.1e} | |J64 - J48| {check:.1e}")
    assert w[64] <= BOUND and check <= BOUND


def test_rule_checks_itself_under_prior_data_conflict(first_target):
    """c_p = (0.08, 40) with control counts (0, 300): the peak lies far out in the weight's tail, no node count of this
    size finds it, and the two rules disagree by tens of nats - the check fires."""
    c_p, ctrl = _override(first_target, *CONFLICT)
    w, _, check = _jacobi_errors(first_target, c_p, ctrl, with_today=False)
    print(f"conflict row c_p = {CONFLICT[0]}, control counts {CONFLICT[1]}: "
          + " | ".join(f"Q = {Q}: {e:.1e}" for Q, e in w.items()) + f" | |J64 - J48| {check:.1e}")
    assert check > BOUND


def test_rule_on_the_fixture_with_emulated_rates(fixture_with_emulated_rates):
    """The one real screen: on its unresolved pairs Q = 64 is within BOUND of the 160-node rule (and 32, 48, 64, 128 agree
    far below it) where today's rule is off by tenths of a nat; on its resolved pairs the Jacobi rule at Q = 64 and
    today's rule at Q = 32 - two rules that share nothing - agree within BOUND."""
    data, alpha = fixture_with_emulated_rates
    d64 = elbo.as_float64(data)
    c_p = mr.model_conc(data, {"alpha_pi": alpha})
    a_prime = mr.beta_exponents(d64, c_p)
    ok = mr.resolved(d64, c_p)
    tail, res = (~ok) & data.repguide_mask, ok & data.repguide_mask
    n_un = mr.n_unresolved(data, {"alpha_pi": alpha})
    print(f"fixture: {int(tail.sum())} unresolved pairs in {int((n_un > 0).sum())} of {data.n_targets} targets; min a' "
          f"{float(a_prime[tail].min()):.3f}, the other exponent up to {float(a_prime[tail].max()):.0f}")
    assert int(tail.sum()) >= 10 and int(res.sum()) >= 10
    spread = today32 = today64 = both = 0.0
    for mu, sd in SETTINGS:
        T = data.n_targets
        h = mr.PairIntegrand(d64, torch.full((T,), mu), torch.full((T,), sd), c_p)
        want = tr.jacobi_rule(h, a_prime, 160)
        J = {Q: tr.jacobi_rule(h, a_prime, Q) for Q in (32, 48, 64, 128)}
        gh32, gh64 = mr.mode_centred_rule(h, a_prime, 32), mr.mode_centred_rule(h, a_prime, 64)
        spread = max(spread, max(float((J[Q] - want).abs()[tail].max()) for Q in J))
        today32 = max(today32, float((gh32 - want).abs()[tail].max()))
        today64 = max(today64, float((gh64 - want).abs()[tail].max()))
        both = max(both, float((J[64] - gh32).abs()[res].max()))
        assert float((J[64] - want).abs()[tail].max()) <= BOUND
        assert float((J[64] - J[48]).abs()[tail].max()) <= BOUND
    print(f"fixture, unresolved pairs: Jacobi Q = 32, 48, 64, 128 within {spread:.1e} of Q = 160; today's rule off by up to "
          f"{today32:.2g} (Q = 32), {today64:.2g} (Q = 64)")
    print(f"fixture, resolved pairs: |Jacobi Q = 64 - today's rule Q = 32| at most {both:.1e}")
    assert both <= BOUND and today32 > BOUND


QUAD_PAIRS = [((40.0, 0.08), (400.0, 0.0)), ((5.0, 0.01), (1000.0, 0.0))]


@pytest.mark.parametrize("row", QUAD_PAIRS, ids=lambda r: f"cp={r[0]}-counts={r[1]}")
def test_rule_against_quadpack(first_target, row):
    """An independent integral of one pair: QUADPACK (scipy.integrate.quad) in t = log pi_1 below pi_1 = 1/2 and in
    s = log pi_0 above it, panel by panel - the algebraic factor becomes exp(a1' t), nothing singular is left.  Q = 64
    (and 48, 160) within BOUND of it.  The prototype measured 7e-12."""
    from scipy import integrate
    cp, counts = row
    c_p, ctrl = _override(first_target, cp, counts)
    a_prime = mr.beta_exponents(first_target, c_p, ctrl)
    R, G = a_prime.shape[:2]
    r, g = 0, int(torch.nonzero(first_target.repguide_mask[0])[0])
    T = first_target.n_targets
    worst = {Q: 0.0 for Q in (48, 64, 160)}
    for mu, sd in SETTINGS[:2]:
        h = mr.PairIntegrand(first_target, torch.full((T,), mu), torch.full((T,), sd), c_p, ctrl=ctrl)

        def h_at(u):
            return float(h(torch.full((1, R, G), float(u), dtype=torch.float64))[0, r, g])

        peak = max(h_at(u) for u in np.linspace(-40.0, 10.0, 501))
        # int exp(h(u)) du, u = logit(pi_1):  du = dt / pi_0 (t = log pi_1),  du = - ds / pi_1 (s = log pi_0)
        def in_t(t):
            p1 = math.exp(t)
            return math.exp(h_at(t - math.log1p(-p1)) - peak) / (1.0 - p1)

        def in_s(s):
            p0 = math.exp(s)
            return math.exp(h_at(math.log1p(-p0) - s) - peak) / (1.0 - p0)

        edges = [-700.0, -300.0, -100.0, -50.0, -30.0, -20.0, -14.0, -10.0, -7.0, -5.0, -3.0, -2.0, -1.0, math.log(0.5)]
        total = 0.0
        for f in (in_t, in_s):
            for lo, hi in zip(edges[:-1], edges[1:]):
                total += integrate.quad(f, lo, hi, epsabs=0.0, epsrel=1e-13, limit=400)[0]
        # below t = -700 (pi_1 < 1e-304) every factor but pi_1^a1' is constant in double precision: the rest of the
        # t side is exp(h(-700)) int_(-inf)^(-700) exp(a1' (t + 700)) dt = exp(h(-700)) / a1'  (at a1' = 0.01 that is
        # 1e-3 of the integral: not to be cut off)
        total += in_t(edges[0]) / float(a_prime[r, g, 1])
        want = peak + math.log(total)
        for Q in worst:
            worst[Q] = max(worst[Q], abs(float(tr.jacobi_rule(h, a_prime, Q)[r, g]) - want))
    print(f"c_p = {cp}, control counts {counts}, pair (0, {g}): against QUADPACK "
          + " | ".join(f"Q = {Q}: {e:.1e}" for Q, e in worst.items()))
    assert worst[64] <= BOUND and worst[48] <= BOUND


@pytest.mark.parametrize("scale", [10.0, 100.0])
def test_rule_at_deeper_counts(first_target, scale):
    """All counts of the target multiplied by 10 and by 100: Q = 64 stays within BOUND of the 160-node rule on every
    row of the table."""
    import copy

    deep = copy.copy(first_target)
    deep.X_masked = first_target.X_masked * scale
    deep.X_bcmatch_masked = first_target.X_bcmatch_masked * scale
    worst = 0.0
    for cp, counts in TABLE:
        c_p, ctrl = _override(first_target, cp, tuple(scale * c for c in counts))
        w, _, _ = _jacobi_errors(deep, c_p, ctrl, nodes=(48, 64), with_today=False)
        worst = max(worst, w[64])
    print(f"counts x {scale:g}: Jacobi Q = 64 within {worst:.1e} of Q = 160 on every row")
    assert worst <= BOUND
