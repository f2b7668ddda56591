"""The quadrature rule of the marginal importance weights against a dense composite rule, on the
CPU in float64: where it holds, by how much, and where it does not - the table of section 21 is this file's output."""
import pytest
import torch

from bean_amd.preprocessing.synthetic import make_sorting_variant_screen
from oracle import elbo

import marginal_reference as mr

SETTINGS = ((0.0, 1.0), (0.5, 1.0), (2.0, 1.3))  # (mu, sd) of every target
BOUND = 1e-3  # nat per pair at Q = 32: 15 pairs of a target then stay below 0.015 nat, under the Monte-Carlo error of a
#               self-normalised weight at S of a few thousand (and only the variation across draws enters it)


@pytest.fixture(scope="module")
def screen():
    return make_sorting_variant_screen(40, 3, seed=3)


@pytest.fixture(scope="module")
def first_target(screen):
    return elbo.as_float64(screen[list(range(int(screen.target_offsets[0]), int(screen.target_offsets[1])))])


def _errors(data, c_p, ctrl, newton=True, nodes=mr.NODES):
    """The largest |rule - dense| over the pairs under the repguide mask and the SETTINGS, per Q."""
    worst = {Q: 0.0 for Q in nodes}
    a_prime = mr.beta_exponents(data, c_p, ctrl)
    for mu, sd in SETTINGS:
        T = data.n_targets
        h = mr.PairIntegrand(data, torch.full((T,), mu), torch.full((T,), sd), c_p, ctrl=ctrl)
        want = mr.dense_rule(h, a_prime)
        assert bool(torch.isfinite(want).all())
        for Q in nodes:
            err = (mr.mode_centred_rule(h, a_prime, Q, newton=newton) - want).abs()[data.repguide_mask]
            worst[Q] = max(worst[Q], float(err.max()))
    return worst


def _override(data, cp, counts):
    G, R, C = data.n_guides, data.n_reps, data.allele_counts_control.shape[1]
    c_p = torch.tensor(cp, dtype=torch.float64).expand(G, 2).clone()
    ctrl = torch.zeros((R, C, G, 2), dtype=torch.float64)
    ctrl[:, 0] = torch.tensor(counts, dtype=torch.float64)
    return c_p, ctrl


def _fmt(w):
    return " | ".join(f"Q = {Q}: {e:.1e}" for Q, e in w.items())


def test_rule_on_the_screen_as_generated(screen):
    """Every pair of the 40 x 3 screen has min(a') >= 2: the recentred rule meets the bound at every Q, and the Beta
    centre alone does not at Q = 16 once the effect moves the mode."""
    data = elbo.as_float64(screen)
    c_p = mr.model_conc(data, elbo.init_params("MixtureNormal", screen))
    a_prime = mr.beta_exponents(data, c_p)
    print(f"c_p {float(c_p.min()):.1f} .. {float(c_p.max()):.1f}; control counts "
          f"{[round(float(v), 1) for v in data.allele_counts_control.sum(1).mean((0, 1))]}; min a' {float(a_prime.min()):.1f}")
    assert bool(mr.resolved(data, c_p).all())
    w = _errors(data, c_p, None)
    print("as generated:", _fmt(w))
    assert w[32] <= BOUND and w[16] <= BOUND and w[64] <= BOUND
    w0 = _errors(data, c_p, None, newton=False)
    print("as generated, Beta centre and scale (no Newton):", _fmt(w0))
    assert w0[16] > BOUND


ROWS = [  # (c_p, control counts, resolved)
    ((40.0, 5.0), (400.0, 0.0), True),
    ((40.0, 2.0), (400.0, 0.0), True),
    ((40.0, 2.0), (0.0, 0.0), True),
    ((2.0, 2.0), (0.0, 0.0), True),
    ((40.0, 1.0), (400.0, 0.0), False),
    ((40.0, 1.0), (0.0, 0.0), False),
    ((1.0, 1.0), (0.0, 0.0), False),
    ((40.0, 0.08), (400.0, 0.0), False),
    ((40.0, 0.08), (0.0, 0.0), False),
]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"cp={r[0]}-counts={r[1]}")
def test_rule_at_the_edge_of_the_predicate(first_target, row):
    """One target's 15 pairs with c_p and the control counts set by hand.  Resolved pairs (min(a') >= 2) meet the bound
    at Q = 32; the essentially unedited guide - c_p = (40, 0.08), no control reads - misses it at every Q: the predicate
    leaves out something real."""
    cp, counts, is_resolved = row
    c_p, ctrl = _override(first_target, cp, counts)
    assert bool(mr.resolved(first_target, c_p, ctrl).all()) == is_resolved
    assert bool(mr.resolved(first_target, c_p, ctrl).any()) == is_resolved
    w = _errors(first_target, c_p, ctrl)
    print(f"c_p = {cp}, control counts {counts}:", _fmt(w))
    if is_resolved:
        assert w[32] <= BOUND
    if cp == (40.0, 0.08) and counts == (0.0, 0.0):
        assert min(w.values()) > BOUND


def test_nodes_integrate_polynomials():
    for Q in mr.NODES:
        x, lw = mr.gauss_hermite(Q)
        # int exp(-x^2) x^2k dx = Gamma(k + 1/2), with the weights exp(lw - x^2)
        w = (lw - x * x).exp()
        for k in (0, 1, 5):
            want = torch.lgamma(torch.tensor(k + 0.5, dtype=torch.float64)).exp()
            assert abs(float((w * x ** (2 * k)).sum() / want) - 1.0) < 1e-12
