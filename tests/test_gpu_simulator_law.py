"""The count simulator's draws (k_simulate_wave2 / k_simulate_members, csrc/bean_predictive.hpp) against the exact
Dirichlet-Multinomial law of the concentrations the kernel itself exports: the beta-binomial marginal of every bin, joint
tables at totals 2 and 3, the bins on the 1e-5 floor, the independence of streams that must not share randomness.  The
regimes, the checks and the threshold live in dm_reference.py; tests/test_dm_reference.py shows on the host that a correct
sampler passes them at these sizes and that each planted fault fails them.  The draws are deterministic (SEED), so a test
passes or fails for good.  -m gpu."""
import time

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401

import dm_reference as dm
from members_common import DEV

pytestmark = pytest.mark.gpu
SEED = 101       # fixed before the first run on a device; a failing check is not answered by another seed
PER_LAUNCH = 64  # bean_hip_simulate_members takes 64 draws per launch
assert dm.N_P == 200  # the p-values this file computes; adding a test moves the threshold 1e-3 / N_P knowingly

# every label under which a test of this file computes p-values (each test asserts its own count against dm.N_PVALUES)
LABELS = ["sparse", "sparse-wave2", "near-floor", "floor", "moderate-Normal", "moderate-MixtureNormal",
          "moderate-MixtureNormal+Acc", "conditions-2", "conditions-3", "conditions-4", "conditions-64", "near-multinomial"]


def _engine(regime, family="Normal", acc=False):
    from bean_amd import engine

    data = dm.regime_screen(regime, with_accessibility=acc)
    kw = dict(scale_by_accessibility=True, fit_noise=True) if acc else {}
    eng = engine.HipSVI(family, data.to(DEV), num_steps=50, **kw)
    assert eng.predictive_supported and eng.use_bcmatch
    for k in ("mu_scale", "sd_scale") + (("noise_scale",) if acc else ()):
        eng.unconstrained[k].fill_(-20.0)  # the latent sites are fixed: the same concentrations at every draw
    if regime not in ("sparse", "near-floor"):
        # (there the pairs of one total must share their concentrations.)  Elsewhere every target has its own effect:
        # the concentrations differ from guide to guide, and a mixture's weights matter (at mu = 0, sd = 1 its two
        # components are the same)
        g = torch.Generator().manual_seed(3)
        eng.unconstrained["mu_loc"].copy_(0.7 * torch.randn(eng.unconstrained["mu_loc"].shape, generator=g))
    if family == "MixtureNormal":
        g = torch.Generator().manual_seed(2)
        p1 = 0.1 + 0.8 * torch.rand((data.n_reps, data.n_guides), generator=g, dtype=torch.float64)
        eng.set_noise({"pi": torch.stack([1 - p1, p1], -1)})
    return eng


def _draws(eng, n_draws):
    """(draws {"X", "X_bcmatch"} (D, R, B, G) numpy, totals (R, G), concentrations (2, R, B, G), seconds on the device):
    draw 64 j + k is plane k of simulate_members(first_draw=64 j, 64)."""
    assert n_draws % PER_LAUNCH == 0
    t0 = time.perf_counter()
    alpha = eng.simulate(0, seed=SEED, alphas=True)["alpha"].clone()
    planes = {"X": [], "X_bcmatch": []}
    for j in range(n_draws // PER_LAUNCH):
        now = eng.simulate(PER_LAUNCH * j, seed=SEED, alphas=True)["alpha"]
        assert float(((now - alpha).abs() / alpha).max()) < 1e-7  # (every concentration is at least 1e-5)
        out = eng.simulate_members(PER_LAUNCH * j, PER_LAUNCH, seed=SEED)
        for k in planes:
            planes[k].append(out[k].cpu().numpy())
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    n = eng._keep["X"].double().sum(1).cpu().numpy().astype(np.int64)
    assert np.array_equal(n, eng._keep["X_BC"].double().sum(1).cpu().numpy().astype(np.int64))
    return {k: np.concatenate(v) for k, v in planes.items()}, n, alpha.cpu().numpy(), seconds


def _hold_to_the_law(regime, label, eng, likelihoods, independent=False, t0=None):
    t0 = time.perf_counter() if t0 is None else t0
    draws, n, alpha2, seconds = _draws(eng, dm.REGIMES[regime]["draws"])
    assert np.array_equal(n, dm.regime_totals(regime))
    rep = dm.evaluate(regime, draws, n, alpha2, np.random.default_rng(SEED), likelihoods, family_label=label,
                      independent=independent)
    print(f"{dm.describe(rep)}; N_P = {dm.N_P}; {seconds:.2f} s on the device, {time.perf_counter() - t0:.2f} s in all")
    for text, r, bound in rep["corr"]:
        print(f"    {text}: {r:+.4f} (bound {bound:.4f})")
    assert label in LABELS
    assert len(rep["p"]) == dm.N_PVALUES[label], len(rep["p"])
    assert dm.failures(rep) == []
    return draws, n, alpha2, rep


def test_sparse_totals_and_concentrations_below_one():
    """Totals 0 ... 13 (every tail of the four-uniforms-per-block loop), concentrations 0.09 ... 0.44 (the alpha < 1 boost,
    U-shaped marginals): the marginals total by total, the joint tables at totals 2 and 3, the independence of the
    streams - and k_simulate_wave2 alone draws the same planes."""
    t0 = time.perf_counter()
    eng = _engine("sparse")
    # every Normal site injected as well: plane k of a launch is simulate(first_draw + k) bit for bit
    eng.set_noise({"eps_mu": torch.zeros(eng.T, dtype=torch.float64), "eps_sd": torch.zeros(eng.T, dtype=torch.float64)})
    draws, n, alpha2, rep = _hold_to_the_law("sparse", "sparse", eng, ("X",), independent=True, t0=t0)
    assert set(n.reshape(-1).tolist()) == set(dm.SPARSE_TOTALS)
    assert 0.08 < alpha2[0].min() and alpha2.max() < 0.5
    assert len(rep["corr"]) == 5 and len(rep["cov_z"]) == 2
    singles = [eng.simulate(d, seed=SEED) for d in range(PER_LAUNCH)]
    torch.cuda.synchronize()
    for key in ("X", "X_bcmatch"):
        alone = np.stack([s[key].cpu().numpy() for s in singles])
        assert np.array_equal(alone, draws[key][:PER_LAUNCH]), key
    eng.close()


def test_concentrations_of_a_thousandth():
    """a0 = 0.01: nearly all mass on "all reads in one bin"; every gamma of a pair can underflow at once."""
    eng = _engine("near-floor")
    _, _, alpha2, rep = _hold_to_the_law("near-floor", "near-floor", eng, ("X",))
    assert alpha2[0].max() < 0.01
    assert rep["occupancy"] is not None
    eng.close()


def test_bins_on_the_floor():
    """One masked sample per replicate, once the last condition (the lone bin of the last gamma pair): its
    concentrations are 1e-5 exactly, and the number of reads that land there is the law's."""
    eng = _engine("floor")
    _, _, alpha2, rep = _hold_to_the_law("floor", "floor", eng, ("X",))
    seen, expect, tail = rep["floor"]
    assert expect < 5.0 and tail >= 1e-5
    eng.close()


@pytest.mark.parametrize("family,acc", [("Normal", False), ("MixtureNormal", False), ("MixtureNormal", True)])
def test_moderate_totals_in_every_family(family, acc):
    """The three template instances; (n, alpha) differ per pair."""
    label = f"moderate-{family}{'+Acc' if acc else ''}"
    eng = _engine("moderate", family, acc)
    _, n, alpha2, rep = _hold_to_the_law("moderate", label, eng, ("X", "X_bcmatch"), independent=family == "Normal")
    assert bool((n % 4 != 0).any())
    assert float(np.ptp(alpha2[0][:, 0, :])) > 1.0  # the concentrations differ from pair to pair
    if family == "Normal":
        assert len(rep["corr"]) == 5 and len(rep["cov_z"]) == 2
    eng.close()


@pytest.mark.parametrize("B", [2, 3, 4, 64])
def test_every_number_of_conditions(B):
    """A single pair of bins, the odd tail with its dummy second concentration, every pair slot of the gamma windows."""
    eng = _engine(f"conditions-{B}")
    assert eng.data.n_condits == B
    _hold_to_the_law(f"conditions-{B}", f"conditions-{B}", eng, ("X",))
    eng.close()


def test_totals_far_below_the_concentrations():
    """a0 = 1e7: p is nearly fixed and the inversion on the cumulative is what is tested; one pair of 20 000 reads in a
    wave of totals near 1000."""
    eng = _engine("near-multinomial")
    _, n, alpha2, _ = _hold_to_the_law("near-multinomial", "near-multinomial", eng, ("X",))
    assert int(n[dm.DEEP_AT]) == dm.DEEP and int(np.median(n)) < 1200 and alpha2[0].sum(1).min() > 9e6
    eng.close()


def test_the_count_of_p_values():
    """The threshold was set for N_P p-values: the tests of this file compute exactly those."""
    assert set(LABELS) == set(dm.N_PVALUES) and len(LABELS) == len(dm.N_PVALUES)
    assert sum(dm.N_PVALUES[k] for k in LABELS) == dm.N_P and dm.N_PVALUES["sparse-wave2"] == 0
    print(f"N_P = {dm.N_P}, threshold {dm.P_MIN:.3e}")
