"""The exact Dirichlet-Multinomial tables of dm_reference.py against scipy, and the power of the checks that
tests/test_gpu_simulator_law.py applies to the device's draws: at that file's own sample sizes and threshold, the plain host
sampler passes every assertion on three seeds, and each planted fault fails the assertion meant to see it on all three.
No GPU."""
import functools

import numpy as np
import pytest
from scipy import stats

import dm_reference as dm

HOST_SEEDS = (20261, 20262, 20263)


# ------------------------------------------------------------------ exact tables
ALPHAS = [
    [1e-5, 1e-5],
    [1e-5, 3.0, 0.4],
    [0.09, 0.09, 0.09, 0.44, 0.09],
    [1e-3, 1e-3, 5e-3],
    [10.0, 1e-5, 25.0, 7.5],
    [1e7, 2e6, 5e6],
    [1e7, 1e-5],
    [5.0, 5.0, 5.0, 25.0, 1e-5],
]


def _scipy_tolerance(n, alpha):
    """What scipy's own formula leaves: betabinom.pmf and dirichlet_multinomial.pmf exponentiate sums of lgamma / betaln
    at arguments up to A0 + n, each rounded to an ulp of its value (~ x log x 2^-52); a handful of them, so relative
    16 (A0 + n) log(A0 + n + 2) 2^-52 + 1e-12."""
    top = float(np.sum(alpha)) + n
    return 16 * top * np.log(top + 2) * 2.0 ** -52 + 1e-12


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 40, 600])
def test_marginal_pmf_is_the_beta_binomial(n, alpha):
    alpha = np.asarray(alpha)
    pmf = dm.marginal_pmf(n, alpha)
    assert pmf.shape == (alpha.size, n + 1) and pmf.dtype == np.float64
    assert np.abs(pmf.sum(1) - 1).max() <= 1e-12
    k = np.arange(n + 1)
    rel = _scipy_tolerance(n, alpha)
    for b, a in enumerate(alpha):
        want = stats.betabinom.pmf(k, n, a, alpha.sum() - a)
        assert np.abs(pmf[b] - want).max() <= rel * max(want.max(), 1e-300) + 1e-300, (b, np.abs(pmf[b] - want).max())


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 6])
def test_joint_pmf_is_the_dirichlet_multinomial(n, alpha):
    alpha = np.asarray(alpha)
    comp, pmf = dm.joint_pmf(n, alpha)
    B = alpha.size
    from math import comb

    assert comp.shape == (comb(n + B - 1, B - 1), B) and (comp.sum(1) == n).all() and (comp >= 0).all()
    assert len({tuple(c) for c in comp.tolist()}) == len(comp)
    assert abs(pmf.sum() - 1) <= 1e-12
    # (scipy takes no n = 0: the one composition there has probability 1)
    want = stats.dirichlet_multinomial.pmf(comp, alpha, n) if n else np.ones(1)
    assert np.abs(pmf - want).max() <= _scipy_tolerance(n, alpha) * want.max()
    # the marginals of the joint table are the marginal tables
    marg = dm.marginal_pmf(n, alpha)
    for b in range(B):
        got = np.bincount(comp[:, b], weights=pmf, minlength=n + 1)
        assert np.abs(got - marg[b]).max() <= 1e-12


def test_a_large_table_sums_to_one():
    for n, alpha in ((600, [1e7, 1e7, 3e6]), (600, [1e-5, 1e-5, 1e-5]), (20000, [2e6, 2e6, 2e6, 1e7, 2e6])):
        assert np.abs(dm.marginal_pmf(n, alpha).sum(1) - 1).max() <= 1e-12


def test_the_count_of_p_values():
    assert dm.N_P == 200 and dm.P_MIN == 1e-3 / 200


# ------------------------------------------------------------------ the host sampler under the GPU tests' assertions
# (regime, the likelihoods whose marginals are tested, whether the concentrations differ per pair)
CASES = {
    "sparse": ("sparse", ("X",), False),
    "near-floor": ("near-floor", ("X",), False),
    "floor": ("floor", ("X",), False),
    "moderate-Normal": ("moderate", ("X", "X_bcmatch"), False),
    "moderate-MixtureNormal": ("moderate", ("X", "X_bcmatch"), True),
    "conditions-2": ("conditions-2", ("X",), False),
    "conditions-3": ("conditions-3", ("X",), False),
    "conditions-4": ("conditions-4", ("X",), False),
    "conditions-64": ("conditions-64", ("X",), False),
    "near-multinomial": ("near-multinomial", ("X",), False),
}


@functools.lru_cache(maxsize=None)
def _report(case, seed, fault=None):
    regime, liks, per_pair = CASES[case]
    rng = np.random.default_rng(seed)
    alpha2 = dm.regime_alpha(regime, rng if per_pair else None)
    n = dm.regime_totals(regime)
    draws = dm.host_screens(n, alpha2, dm.REGIMES[regime]["draws"], rng, fault)
    rep = dm.evaluate(regime, draws, n, alpha2, rng, liks, family_label=f"{case} seed {seed} fault {fault}")
    print(dm.describe(rep))
    return rep


@pytest.mark.parametrize("seed", HOST_SEEDS)
@pytest.mark.parametrize("case", list(CASES))
def test_the_reference_passes_every_assertion(case, seed):
    rep = _report(case, seed)
    assert len(rep["p"]) == dm.N_PVALUES[case], len(rep["p"])  # the count the threshold was set with
    assert dm.failures(rep) == []
    if case in ("sparse", "moderate-Normal"):
        assert len(rep["corr"]) == 5 and len(rep["cov_z"]) == 2
    if case == "floor":
        assert rep["floor"] is not None


def _kinds(rep):
    return {text.split(" ")[0] for text in dm.failures(rep)}


# fault -> [(case, the kind of assertion that must fail)]
SEEN_BY = {
    "no_boost": [("sparse", "p-value")],
    "no_dirichlet": [("sparse", "p-value"), ("moderate-Normal", "p-value")],
    "conc_x1.25": [("sparse", "p-value"), ("moderate-Normal", "p-value")],
    "shift": [("sparse", "p-value"), ("near-multinomial", "p-value")],
    "shared_uniforms": [("sparse", "correlation"), ("moderate-Normal", "correlation")],
    "last_pair": [("conditions-3", "p-value"), ("sparse", "p-value"), ("moderate-Normal", "p-value")],
    # what the simulator was before it normalised such pairs in logs: the near-floor regime's occupancy count sees it
    "floor_only": [("near-floor", "occupancy:")],
}


@pytest.mark.parametrize("seed", HOST_SEEDS)
@pytest.mark.parametrize("fault,case,kind", [(f, c, k) for f, seen in SEEN_BY.items() for c, k in seen])
def test_a_planted_fault_fails_its_assertion(fault, case, kind, seed):
    rep = _report(case, seed, fault)
    assert kind in _kinds(rep), (fault, case, dm.describe(rep))
    if fault == "shared_uniforms":  # the correlation of the two likelihoods is the check that sees it
        label, r, bound = rep["corr"][0]
        assert label.startswith("X and X_bcmatch") and abs(r) > bound


def test_the_covariance_check_sees_a_sampler_without_its_dirichlet():
    """-n (n + A0) / (1 + A0) p_a p_b is the Dirichlet-Multinomial's; a plain multinomial's is -n p_a p_b."""
    for seed in HOST_SEEDS:
        assert "covariance" in _kinds(_report("moderate-Normal", seed, "no_dirichlet"))
