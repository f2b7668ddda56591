"""The implicit Dirichlet gradient with its x-free factors tabulated (dirichlet_grad_one_tab and dirgrad_tab_make,
csrc/bean_special.hpp; DevArgs::dgt): bean_hip_test_special op 11 forms the table in the kernel with the device function
the finish uses and evaluates the call the guide kernels make.  It must give the bits of op 10 (dirichlet_grad_one_pre,
every factor formed in the call) at every point: concentrations on a log grid from 1e-5 (the c_q clamp) to 1e5, draws
inside the +-0.1 sd window of the Taylor sub-branch, on both of its edges, an ulp to either side of them and just outside,
below and above the mean, at 0.5, and in the three other branches, where the table changes nothing.  Both calls a guide
makes are covered: component 0 (x, c_0, c_0 + c_1) and component 1 (1 - x, c_1, c_0 + c_1) - the second sees
beta = fl(total - c_1), which need not be c_0, so it reads factors of its own.  -m gpu."""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401

pytestmark = pytest.mark.gpu

DBL_MIN = float(np.finfo(np.float64).tiny)
ONE_MINUS = float(np.nextafter(1.0, 0.0))
N_GRID = 17
_cache = {}


def _points():
    """(x, c0, c1): every pair of the concentration grid with the draws listed in the module docstring."""
    if "pts" in _cache:
        return _cache["pts"]
    grid = np.logspace(-5.0, 5.0, N_GRID)
    grid[0], grid[-1] = 1e-5, 1e5
    # between the decades too: concentrations whose sum is not exact
    grid = np.concatenate([grid, [6.0, np.nextafter(6.0, 7.0), 7.3, 10.5, 72.0, 133.7]])
    c0, c1 = [g.reshape(-1) for g in np.meshgrid(grid, grid, indexing="ij")]
    tot = c0 + c1
    mean = c0 / tot
    sd = np.sqrt(c0 * c1 / (tot + 1.0)) / tot
    lo, hi = mean - 0.1 * sd, mean + 0.1 * sd
    xs = [mean, lo, hi, np.nextafter(lo, 0.0), np.nextafter(lo, 1.0), np.nextafter(hi, 0.0), np.nextafter(hi, 1.0),
          mean - 0.05 * sd, mean + 0.05 * sd, mean - 0.11 * sd, mean + 0.11 * sd, mean - sd, mean + sd, mean - 3.0 * sd,
          mean + 3.0 * sd, np.full_like(mean, 0.5), np.full_like(mean, 0.1), np.full_like(mean, 0.9),
          np.full_like(mean, 1e-3), np.full_like(mean, 1.0 - 1e-3), np.full_like(mean, DBL_MIN),
          np.full_like(mean, ONE_MINUS)]
    x = np.clip(np.concatenate(xs), DBL_MIN, ONE_MINUS)
    n = len(xs)
    _cache["pts"] = (x, np.tile(c0, n), np.tile(c1, n))
    return _cache["pts"]


def _branch(x, alpha, total):
    """The branch of dirichlet_grad_one_t by the header's comparisons in numpy float64 (for the coverage counts only:
    a point an ulp from an edge may be counted on the other side)."""
    beta = total - alpha
    boundary = total * x * (1.0 - x)
    small_a = (x <= 0.5) & (boundary < 2.5)
    small_b = ~small_a & (x >= 0.5) & (boundary < 0.75)
    mid = ~small_a & ~small_b & (alpha > 6.0) & (beta > 6.0)
    with np.errstate(all="ignore"):
        t = alpha + beta
        mean = alpha / t
        sd = np.sqrt(alpha * beta / (t + 1.0)) / t
    taylor = mid & (mean - 0.1 * sd <= x) & (x <= mean + 0.1 * sd)
    return small_a, small_b, taylor, mid & ~taylor, ~small_a & ~small_b & ~mid


@pytest.mark.parametrize("component", [0, 1])
def test_tabulated_call_gives_the_bits_of_the_plain_call(component):
    from bean_amd import engine

    x, c0, c1 = _points()
    total = c0 + c1
    if component == 1:  # the guide's second call: the other component, the same total
        x, alpha = np.clip(1.0 - x, DBL_MIN, ONE_MINUS), c1
    else:
        alpha = c0
    assert 3000 < len(x) < 20000
    counts = [int(b.sum()) for b in _branch(x, alpha, total)]
    print("points", len(x), "small_alpha / small_beta / taylor / saddle / rational:", counts)
    assert min(counts) >= 50, counts
    plain, _ = engine.test_special(10, alpha, x, total)
    tab, _ = engine.test_special(11, alpha, x, total)
    plain, tab = plain.cpu(), tab.cpu()
    mid = torch.from_numpy(_branch(x, alpha, total)[2] | _branch(x, alpha, total)[3])
    assert torch.isfinite(plain[mid]).all()
    # bit for bit, NaN (0 * inf in the series branches at the ends of the range) included
    differ = plain.view(torch.int64) != tab.view(torch.int64)
    n_bad = int(differ.sum())
    if n_bad:
        i = int(torch.nonzero(differ)[0])
        print("first difference at x, alpha, total =", x[i], alpha[i], total[i], "plain", plain[i].item(), "tab", tab[i].item())
    assert n_bad == 0, f"{n_bad} of {len(x)} points differ"
    nan = torch.isnan(plain)
    print("NaN in the plain call (series branches at the ends of the range):", int(nan.sum()))
    assert torch.equal(plain[~nan], tab[~nan])
