"""The exact Dirichlet-Multinomial law, and the checks that hold the count simulator's draws to it.

Host only: numpy and scipy.  Nothing here is code under test, and nothing here looks at a device.  The module is imported
by bare name (as grad_bounds.py is) by tests/test_gpu_simulator_law.py, which feeds it the device's draws, and by
tests/test_dm_reference.py, which feeds it the draws of ``host_dm`` - a plain numpy sampler of the same construction as the
kernel - at the same sizes: without a fault it must pass every check, and with each planted fault it must fail the check
that is meant to see that fault.  That is what sets the number of draws of every regime; the threshold is fixed.

Bin b of DM(n, alpha) is BetaBinomial(n, alpha_b, A0 - alpha_b), A0 = sum alpha.

Layout: a set of draws is ``x`` (D, R, B, G) as the simulator's planes are, with totals ``n`` (R, G) and concentrations
``alpha`` (R, B, G) of that likelihood.
"""
from __future__ import annotations

import copy
from itertools import combinations

import numpy as np
from scipy import stats

DBL_MIN = np.finfo(np.float64).tiny
LOG_BELOW = 1e-290  # csrc/bean_predictive.hpp::kSimLogBelow
# host_dm's planted faults: Gamma(alpha + 1) without U^(1 / alpha) below 1 | p = alpha / A0 | concentrations 25 % too
# large | bin k counted as (k + 1) % B | the second likelihood reuses the first one's uniforms | the last bin of an odd B
# drawn with the dummy's concentration 1.0 | no normalisation in logs where every gamma underflows
FAULTS = ("no_boost", "no_dirichlet", "conc_x1.25", "shift", "shared_uniforms", "last_pair", "floor_only")

# ---------------------------------------------------------------------------------------------------------------------
# the threshold.  Every chi-square / KS p-value of tests/test_gpu_simulator_law.py must exceed P_MIN = 1e-3 / N_P, N_P the
# number of p-values that file computes (the sum of N_PVALUES, asserted there against the counts it sees): the family-wise
# false-alarm rate of the file is then at most 1e-3.
N_PVALUES = {
    "sparse": 47,            # 9 totals x 5 bins + 2 joint tables
    "sparse-wave2": 0,       # (the same planes, bit for bit)
    "near-floor": 40,        # 7 totals x 5 bins + 5 PIT
    "floor": 5,
    "moderate-Normal": 10,   # 5 bins x 2 likelihoods
    "moderate-MixtureNormal": 10,
    "moderate-MixtureNormal+Acc": 10,
    "conditions-2": 2,
    "conditions-3": 3,
    "conditions-4": 4,
    "conditions-64": 64,
    "near-multinomial": 5,
}
N_P = sum(N_PVALUES.values())
P_MIN = 1e-3 / N_P
SIGMAS = 5.0  # the independence and covariance bounds


# ---------------------------------------------------------------------------------------------------------------------
# exact tables
def marginal_pmf(n, alpha):
    """(B, n + 1) float64: row b is BetaBinomial(n, alpha_b, A0 - alpha_b).  By the ratio recurrence from
    pmf(0) = prod_i (b + i) / (a + b + i), all in logs: no lgamma of a large argument, so the rows sum to 1 within 1e-12
    at concentrations of 1e-5 as at 1e7."""
    n = int(n)
    wide = np.longdouble  # the sums below run over n terms of size log n: accumulated in extended precision where there is one
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1).astype(wide)
    a = alpha[:, None]
    # (the others' sum, not A0 - alpha_b: a bin of 1e-5 beside one of 1e7 would be lost in the difference)
    b = np.asarray([np.delete(alpha, k).sum() for k in range(alpha.size)], dtype=wide)[:, None]
    i = np.arange(n, dtype=wide)[None, :]
    with np.errstate(divide="ignore"):
        log0 = np.where(a < 0.5 * (b + i), np.log1p(-a / (a + b + i)), np.log((b + i) / (a + b + i))).sum(1, keepdims=True)
    # pmf(k + 1) / pmf(k) = (n - k) (k + a) / ((k + 1) (n - k - 1 + b))
    ratio = np.log(n - i) + np.log(i + a) - np.log(i + 1) - np.log(n - i - 1 + b)
    logp = np.concatenate([log0, log0 + np.cumsum(ratio, 1)], 1)
    return np.exp(logp).astype(np.float64)


def compositions(n, B):
    """Every composition of n into B parts, (M, B) int64, M = C(n + B - 1, B - 1)."""
    out = []
    for bars in combinations(range(n + B - 1), B - 1):
        edges = (-1,) + bars + (n + B - 1,)
        out.append([edges[k + 1] - edges[k] - 1 for k in range(B)])
    return np.asarray(out, dtype=np.int64)


def joint_pmf(n, alpha):
    """(compositions (M, B), pmf (M,)) of DM(n, alpha): n! / (A0)_n prod_b (alpha_b)_{x_b} / x_b!, rising factorials
    as sums of logs - for small n and B."""
    n = int(n)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    comp = compositions(n, alpha.size)
    i = np.arange(n, dtype=np.float64)
    rise = np.concatenate([np.zeros((alpha.size, 1)), np.cumsum(np.log(alpha[:, None] + i[None, :]), 1)], 1)  # (B, n + 1)
    fact = np.concatenate([[0.0], np.cumsum(np.log(i + 1.0))])  # log k!
    logp = fact[n] - np.log(alpha.sum() + i).sum() + (rise[np.arange(alpha.size)[None, :], comp] - fact[comp]).sum(1)
    return comp, np.exp(logp)


def dm_moments(n, alpha, b):
    """Exact mean and variance of bin b: n (R, G), alpha (R, B, G) -> two (R, G) arrays."""
    A0 = alpha.sum(1)
    p = alpha[:, b, :] / A0
    return n * p, n * p * (1 - p) * (n + A0) / (1 + A0)


# ---------------------------------------------------------------------------------------------------------------------
# goodness of fit
def _merge_small(expected, observed, least=5.0):
    """Cells in order; a cell whose expected count is below `least` is merged into its neighbour (the next one; what is
    left at the end into the one before)."""
    e_out, o_out = [], []
    e_acc = o_acc = 0.0
    for e, o in zip(expected, observed):
        e_acc += e
        o_acc += o
        if e_acc >= least:
            e_out.append(e_acc)
            o_out.append(o_acc)
            e_acc = o_acc = 0.0
    if e_acc > 0 or o_acc > 0:
        if e_out:
            e_out[-1] += e_acc
            o_out[-1] += o_acc
        else:
            e_out.append(e_acc)
            o_out.append(o_acc)
    return np.asarray(e_out), np.asarray(o_out)


def _chi2_p(expected, observed):
    if len(expected) < 2:
        return None
    stat = float((((observed - expected) ** 2) / expected).sum())
    return float(stats.chi2.sf(stat, len(expected) - 1))


def gof_marginals(x, n, alpha):
    """Samples x (N, B) that share one (n, alpha): a chi-square test of every bin against its beta-binomial marginal,
    cells of fewer than 5 expected merged into their neighbour, a bin with one cell left skipped.  Returns
    [(bin, p-value)]."""
    x = np.asarray(x)
    N = x.shape[0]
    pmf = marginal_pmf(n, alpha)
    out = []
    for b in range(pmf.shape[0]):
        obs = np.bincount(x[:, b].astype(np.int64), minlength=int(n) + 1).astype(np.float64)
        assert obs.size == int(n) + 1, "a count above its total"
        p = _chi2_p(*_merge_small(N * pmf[b], obs))
        if p is not None:
            out.append((b, p))
    return out


def gof_joint(x, n, alpha):
    """Samples x (N, B) of one (n, alpha) against the joint table: cells of fewer than 5 expected are pooled into one
    (the table has no order to merge along).  Returns the p-value, or None with one cell left."""
    x = np.asarray(x).astype(np.int64)
    N = x.shape[0]
    comp, pmf = joint_pmf(n, alpha)
    base = (int(n) + 1) ** np.arange(comp.shape[1])
    code = {int(c): k for k, c in enumerate(comp @ base)}
    obs = np.zeros(len(pmf))
    for c, cnt in zip(*np.unique(x @ base, return_counts=True)):
        obs[code[int(c)]] += cnt  # (a KeyError is a draw that does not add up to n)
    exp = N * pmf
    small = exp < 5.0
    e = np.concatenate([exp[~small], [exp[small].sum()]]) if small.any() else exp
    o = np.concatenate([obs[~small], [obs[small].sum()]]) if small.any() else obs
    if small.any() and e[-1] < 5.0 and len(e) > 1:  # the pool itself is small: into the smallest of the others
        k = int(np.argmin(e[:-1]))
        e[k] += e[-1]
        o[k] += o[-1]
        e, o = e[:-1], o[:-1]
    return _chi2_p(e, o)


def pit_marginals(x, n, alpha, rng, keep=None):
    """Samples whose (n, alpha) differ per (replicate, guide): x (D, R, B, G), n (R, G), alpha (R, B, G).  The randomised
    probability transform u = F(x - 1) + v (F(x) - F(x - 1)), v uniform from `rng`, F from the pair's own pmf table (built
    once per pair), is uniform under the law; a KS test of the pooled u per bin.  `keep` (R, B) leaves samples out.
    Returns [(bin, p-value)]."""
    x = np.asarray(x).astype(np.int64)
    D, R, B, G = x.shape
    u = np.full((D, R, B, G), np.nan)
    v = rng.random((D, R, B, G))
    for r in range(R):
        for g in range(G):
            pmf = marginal_pmf(n[r, g], alpha[r, :, g])          # (B, n + 1)
            below = np.cumsum(pmf, 1) - pmf                       # F(x - 1)
            xs = x[:, r, :, g]                                    # (D, B)
            rows = np.arange(B)[None, :]
            u[:, r, :, g] = below[rows, xs] + v[:, r, :, g] * pmf[rows, xs]
    out = []
    for b in range(B):
        sel = u[:, :, b, :] if keep is None else u[:, np.asarray(keep)[:, b].astype(bool), b, :]
        if sel.size:
            out.append((b, float(stats.kstest(sel.reshape(-1), "uniform").pvalue)))
    return out


def independence(z_a, z_b):
    """The correlation of two arrays of counts standardised with their exact means and variances, and its bound: under
    independence the mean of z_a z_b has standard deviation 1 / sqrt(N) whatever the shape of the law, so 5 / sqrt(N)."""
    z_a, z_b = np.asarray(z_a, dtype=np.float64).reshape(-1), np.asarray(z_b, dtype=np.float64).reshape(-1)
    ok = np.isfinite(z_a) & np.isfinite(z_b)
    N = int(ok.sum())
    return float((z_a[ok] * z_b[ok]).mean()), SIGMAS / np.sqrt(N)


def _raw_mixed(n, a, b, A0, i, j):
    """E[x_a^i x_b^j], i, j <= 2, of two bins of DM(n, .) from the factorial moments
    E[x_a^(i) x_b^(j)] = n^(i+j) a^[i] b^[j] / A0^[i+j] (falling n, rising a, b, A0)."""
    def fall(v, k):
        out = np.ones_like(v)
        for t in range(k):
            out = out * (v - t)
        return out

    def rise(v, k):
        out = np.ones_like(v)
        for t in range(k):
            out = out * (v + t)
        return out

    def fm(p, q):
        return fall(n, p + q) * rise(a, p) * rise(b, q) / rise(A0, p + q)

    # x^0 = 1, x^1 = x^(1), x^2 = x^(2) + x^(1)
    parts = {0: [0], 1: [1], 2: [2, 1]}
    return sum(fm(p, q) for p in parts[i] for q in parts[j])


def pair_covariance_z(x, n, alpha):
    """The within-pair covariance of the two bins with the largest concentrations, against the exact
    -n (n + A0) / (1 + A0) p_a p_b: each sample's (x_a - m_a)(x_b - m_b), less that expectation, in units of its own
    exact standard deviation (mixed moments up to order four, closed form), averaged: a z score, N(0, 1) under the law.
    Pairs of fewer than 2 reads are left out."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[0]
    order = np.argsort(alpha, 1)
    ia, ib = order[:, -1, :], order[:, -2, :]                       # (R, G)
    al = np.take_along_axis(alpha, ia[:, None, :], 1)[:, 0, :]
    be = np.take_along_axis(alpha, ib[:, None, :], 1)[:, 0, :]
    A0 = alpha.sum(1)
    nn = np.asarray(n, dtype=np.float64)
    m = {(i, j): _raw_mixed(nn, al, be, A0, i, j) for i in range(3) for j in range(3)}
    ma, mb = m[1, 0], m[0, 1]
    cov = m[1, 1] - ma * mb
    assert np.allclose(cov, -nn * (nn + A0) / (1 + A0) * (al / A0) * (be / A0), rtol=1e-9, atol=1e-12)
    # E[(xa - ma)^2 (xb - mb)^2], expanded
    ca = {0: ma * ma, 1: -2 * ma, 2: np.ones_like(ma)}
    cb = {0: mb * mb, 1: -2 * mb, 2: np.ones_like(mb)}
    second = sum(ca[i] * cb[j] * m[i, j] for i in range(3) for j in range(3))
    var = second - cov * cov
    ok = (nn >= 2) & (var > 0)
    xa = np.take_along_axis(x, np.broadcast_to(ia[None, :, None, :], (D,) + ia.shape[:1] + (1,) + ia.shape[1:]), 2)[:, :, 0, :]
    xb = np.take_along_axis(x, np.broadcast_to(ib[None, :, None, :], (D,) + ib.shape[:1] + (1,) + ib.shape[1:]), 2)[:, :, 0, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = ((xa - ma) * (xb - mb) - cov) / np.sqrt(var)
    t = t[:, ok]
    return float(t.mean() * np.sqrt(t.size))


# ---------------------------------------------------------------------------------------------------------------------
# the host sampler
def host_dm(n, alpha, size, rng, fault=None, alpha_bc=None):
    """`size` draws of DM(n_p, alpha_p) for every pair p: n (P,), alpha (P, B) -> (size, P, B) int64.  Built as the kernel
    builds it: float64 gammas (Gamma(alpha + 1) U^(1 / alpha) below 1), floored at DBL_MIN, normalised (in logs where the
    floored gammas of a pair add up to less than LOG_BELOW: "floor_only" is the sampler without that, which hands a pair
    whose gammas all underflow to its bins in equal shares), then n categorical draws by inversion on the cumulative, the
    last bin taking what the cumulative leaves.  With `alpha_bc` a second likelihood of the same totals is drawn and
    (x, x_bc) returned.  `fault` plants one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    n = np.asarray(n, dtype=np.int64).reshape(-1)
    P = n.size

    def probabilities(al):
        al = np.asarray(al, dtype=np.float64)
        B = al.shape[1]
        if fault == "no_dirichlet":
            return np.broadcast_to((al / al.sum(1, keepdims=True))[None], (size, P, B))
        used = al * 1.25 if fault == "conc_x1.25" else al.copy()
        if fault == "last_pair" and B % 2 == 1:
            used[:, -1] = 1.0
        low = used < 1.0
        g = rng.standard_gamma(np.broadcast_to(np.where(low, used + 1.0, used)[None], (size, P, B)))
        u = rng.random((size, P, B))
        inv = (1.0 / np.where(low, used, 1.0))[None]
        boosted = low[None] & (fault != "no_boost")
        with np.errstate(under="ignore"):
            floored = np.maximum(np.where(boosted, g * u ** inv, g), DBL_MIN)
        p = floored / floored.sum(-1, keepdims=True)
        if fault != "floor_only":
            # where every gamma of a pair sits at or near the floor, the same draws in logs (the kernel's kSimLogBelow)
            rows = floored.sum(-1) < LOG_BELOW
            if rows.any():
                log_scale = np.where(np.broadcast_to(boosted, g.shape), np.log(u) * inv, 0.0)  # log U / alpha
                lg = np.log(g[rows]) + log_scale[rows]
                w = np.exp(lg - lg.max(-1, keepdims=True))
                p[rows] = w / w.sum(-1, keepdims=True)
        return p

    def uniforms(lo, hi, nmax):
        return rng.random((size, hi - lo, nmax))

    def categorical(p, u_of):
        """u_of(lo, hi, nmax): the uniforms of pairs lo..hi (in the order of `by_n`)."""
        B = p.shape[-1]
        cum = np.cumsum(p, -1)[..., : B - 1]
        x = np.zeros((size, P, B), dtype=np.int64)
        for lo in range(0, P, 32):
            idx = by_n[lo: lo + 32]
            nmax = int(n[idx].max())
            if nmax == 0:
                continue
            u = u_of(lo, lo + len(idx), nmax)
            live = np.arange(nmax)[None, None, :] < n[idx][None, :, None]
            k = np.zeros(u.shape, dtype=np.int8 if B <= 127 else np.int16)
            for b in range(B - 1):
                k += u >= cum[:, idx, b][:, :, None]
            for b in range(B):
                x[:, idx, b] = ((k == b) & live).sum(-1)
        return x

    by_n = np.argsort(n, kind="stable")  # blocks of pairs of similar totals: one deep pair costs its block alone
    kept = {}

    def fresh(lo, hi, nmax):
        kept[lo] = uniforms(lo, hi, nmax)
        return kept[lo]

    x = categorical(probabilities(alpha), fresh if (fault == "shared_uniforms" and alpha_bc is not None) else uniforms)
    if fault == "shift":
        x = np.roll(x, 1, -1)  # what the sampler drew as bin k is counted as bin (k + 1) % B
    if alpha_bc is None:
        return x
    again = (lambda lo, hi, nmax: kept[lo]) if fault == "shared_uniforms" else uniforms
    x_bc = categorical(probabilities(alpha_bc), again)
    if fault == "shift":
        x_bc = np.roll(x_bc, 1, -1)
    return x, x_bc


def host_screens(n, alpha2, draws, rng, fault=None):
    """host_dm in the simulator's layout: n (R, G), alpha2 (2, R, B, G) -> {"X", "X_bcmatch"}, each (draws, R, B, G)."""
    _, R, B, G = alpha2.shape
    flat = lambda a: np.moveaxis(a, 1, 2).reshape(R * G, B)  # noqa: E731  (R, B, G) -> (R G, B)
    x, x_bc = host_dm(n.reshape(-1), flat(alpha2[0]), draws, rng, fault, alpha_bc=flat(alpha2[1]))
    back = lambda a: np.moveaxis(a.reshape(draws, R, G, B), 3, 2)  # noqa: E731
    return {"X": back(x), "X_bcmatch": back(x_bc)}


# ---------------------------------------------------------------------------------------------------------------------
# the regimes: what tests/test_gpu_simulator_law.py draws on the device and tests/test_dm_reference.py on the host
SPARSE_TOTALS = (0, 1, 2, 3, 4, 5, 6, 7, 9, 13)
NEAR_FLOOR_TOTALS = (5, 8, 12, 17, 23, 30, 40)
DEEP = 20000
DEEP_AT = (1, 70)  # (replicate, guide): in the second tile of replicate 1

REGIMES = {
    # name: guides, replicates, conditions, a0, draws, the masked samples [(replicate, condition)]
    "sparse": dict(G=128, R=2, B=5, a0=0.8, draws=512, masked=()),
    "near-floor": dict(G=128, R=2, B=5, a0=0.01, draws=256, masked=()),
    "floor": dict(G=128, R=2, B=5, a0=50.0, draws=64, masked=((0, 1), (1, 4))),
    "moderate": dict(G=128, R=2, B=5, a0=50.0, draws=64, masked=()),
    "conditions-2": dict(G=64, R=1, B=2, a0=20.0, draws=64, masked=()),
    "conditions-3": dict(G=64, R=1, B=3, a0=20.0, draws=64, masked=()),
    "conditions-4": dict(G=64, R=1, B=4, a0=20.0, draws=64, masked=()),
    "conditions-64": dict(G=64, R=1, B=64, a0=20.0, draws=64, masked=()),
    "near-multinomial": dict(G=128, R=2, B=5, a0=1e7, draws=64, masked=()),
}


def regime_bins(B):
    """B - 1 sorting bins of equal width (the bulk sample is the B-th condition); None: the generator's own four."""
    if B == 5:
        return None
    if B == 2:
        return ((0.5, 1.0),)
    return tuple((i / (B - 1), (i + 1) / (B - 1)) for i in range(B - 1))


def regime_totals(name):
    """(R, G) int64 totals of a regime."""
    spec = REGIMES[name]
    R, G = spec["R"], spec["G"]
    idx = np.arange(R * G).reshape(R, G)
    if name == "sparse":
        return np.asarray(SPARSE_TOTALS)[idx % len(SPARSE_TOTALS)]
    if name == "near-floor":
        return np.asarray(NEAR_FLOOR_TOTALS)[idx % len(NEAR_FLOOR_TOTALS)]
    if name in ("moderate", "floor"):
        return np.random.default_rng(8).integers(400, 601, (R, G))  # what the moments test of test_gpu_predictive.py uses
    if name.startswith("conditions"):
        return np.random.default_rng(9).integers(150, 251, (R, G))
    if name == "near-multinomial":
        n = np.random.default_rng(10).integers(900, 1101, (R, G))
        n[DEEP_AT] = DEEP
        return n
    raise KeyError(name)


def regime_alpha(name, rng=None):
    """(2, R, B, G) concentrations of the same magnitudes as the device's in this regime, for the host sampler: a0 times
    the shares of equal-width bins and a bulk sample that holds every cell; 1e-5 where the sample is masked.  With `rng`
    the shares differ per pair and likelihood (as a mixture's do)."""
    spec = REGIMES[name]
    R, G, B = spec["R"], spec["G"], spec["B"]
    e = np.full(B, 0.2 if B == 5 else 1.0 / (B - 1))
    e[B - 2] = 1.0  # the bulk sample sorts in front of the last bin
    al = np.broadcast_to((spec["a0"] * e / e.sum())[None, None, :, None], (2, R, B, G)).copy()
    if rng is not None:
        w = np.exp(0.3 * rng.standard_normal((2, R, B, G)))
        al = spec["a0"] * (al * w) / (al * w).sum(2, keepdims=True)
    for r, b in spec["masked"]:
        al[:, r, b, :] = 1e-5
    return al


def flat_screen(n_guides=128, n_reps=2, bins=None, totals=None, a0=50.0, masked=(), with_accessibility=False):
    """A generated variant sorting screen with its fields overwritten: no guide masks, unit size factors, one a0, the
    given totals (R, G) split over the conditions (the bulk sample five times a bin's share), the same counts for both
    likelihoods; the samples `masked` [(replicate, condition)] are masked and hold no counts.  The defaults are 128
    guides x 2 replicates x 5 conditions, totals 400 ... 600 (not all multiples of 4), a0 = 50."""
    import torch

    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    kw = {} if bins is None else dict(bins=bins)
    data = make_sorting_variant_screen(n_guides, n_reps, seed=4, with_accessibility=with_accessibility, **kw)
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    n = np.random.default_rng(8).integers(400, 601, (R, G)) if totals is None else np.asarray(totals, dtype=np.int64)
    assert n.shape == (R, G)
    share = np.array([0.2 if not (lo == 0 and hi == 1) else 1.0
                      for lo, hi in zip(data.lower_bounds.tolist(), data.upper_bounds.tolist())])
    mask = np.ones((R, B), dtype=np.int64)
    for r, b in masked:
        mask[r, b] = 0
    w = share[None, :] * mask
    x = np.floor(n[:, None, :] * (w / w.sum(1, keepdims=True))[:, :, None])
    first = np.argmax(mask, 1)  # the first sample that is not masked takes what the rounding left
    for r in range(R):
        x[r, first[r], :] += n[r] - x[r].sum(0)
    x = torch.as_tensor(x, dtype=torch.float32)
    out = copy.copy(data)
    out.X = out.X_masked = x
    out.X_bcmatch = out.X_bcmatch_masked = x.clone()
    out.size_factor = torch.ones((R, B), dtype=torch.float64)
    out.size_factor_bcmatch = torch.ones((R, B), dtype=torch.float64)
    out.a0 = torch.full((G,), float(a0), dtype=torch.float64)
    out.a0_bcmatch = torch.full((G,), float(a0), dtype=torch.float64)
    out.repguide_mask = torch.ones((R, G), dtype=torch.bool)
    out.sample_mask = torch.as_tensor(mask, dtype=data.sample_mask.dtype)
    return out


def regime_screen(name, with_accessibility=False):
    spec = REGIMES[name]
    return flat_screen(spec["G"], spec["R"], regime_bins(spec["B"]), regime_totals(name), spec["a0"], spec["masked"],
                       with_accessibility)


# ---------------------------------------------------------------------------------------------------------------------
# the assertions, as functions of a set of draws: the GPU tests and the host tests call the same ones
def law_pvalues(name, x, n, alpha, rng):
    """Every p-value that regime `name` takes of the draws x (D, R, B, G) of one likelihood: [(label, p)]."""
    D, R, B, G = x.shape
    out = []
    if name in ("sparse", "near-floor"):
        # pairs of one total share their concentrations: the exact marginals, total by total
        for t in sorted(set(n.reshape(-1).tolist())):
            rr, gg = np.nonzero(n == t)
            al = alpha[rr[0], :, gg[0]]
            assert np.allclose(alpha[rr, :, gg], al[None, :], rtol=1e-6, atol=0), "pairs of one total share alpha"
            xs = x[:, rr, :, gg]  # (pairs, D, B)
            xs = xs.reshape(-1, B)
            out += [(f"total {t} bin {b}", p) for b, p in gof_marginals(xs, t, al)]
            if name == "sparse" and t in (2, 3):
                out.append((f"total {t} joint", gof_joint(xs, t, al)))
        if name == "near-floor":
            out += [(f"PIT bin {b}", p) for b, p in pit_marginals(x, n, alpha, rng)]
        return out
    keep = None
    if name == "floor":
        keep = np.ones((R, B), dtype=bool)
        for r, b in REGIMES["floor"]["masked"]:
            keep[r, b] = False
    return [(f"PIT bin {b}", p) for b, p in pit_marginals(x, n, alpha, rng, keep)]


def floor_count(x, n, alpha):
    """The floor regime's masked samples: (observed number of non-zero counts there over all draws, its exact
    expectation sum (1 - pmf(0)), P(Poisson(expectation) >= observed))."""
    D = x.shape[0]
    seen, expect = 0, 0.0
    for r, b in REGIMES["floor"]["masked"]:
        assert (alpha[r, b, :] == 1e-5).all(), "a masked sample's concentrations are on the floor exactly"
        seen += int((x[:, r, b, :] != 0).sum())
        for g in range(x.shape[3]):
            expect += D * (1.0 - marginal_pmf(n[r, g], alpha[r, :, g])[b, 0])
    return seen, expect, float(stats.poisson.sf(seen - 1, expect))


def occupancy_pmf(n, alpha):
    """P(exactly k bins hold a read), k = 0 ... B, of DM(n, alpha): all n reads fall inside a set S of bins with
    probability prod_i (A_S + i) / (A0 + i); inclusion-exclusion over the subsets gives "exactly S"."""
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    B, n = alpha.size, int(n)
    i = np.arange(n, dtype=np.float64)
    inside = np.zeros(1 << B)
    for s in range(1, 1 << B):
        a_s = alpha[[b for b in range(B) if s >> b & 1]].sum()
        inside[s] = np.exp((np.log(a_s + i) - np.log(alpha.sum() + i)).sum())
    inside[0] = 1.0 if n == 0 else 0.0
    out = np.zeros(B + 1)
    for s in range(1 << B):
        exactly, t = 0.0, s
        while True:  # the subsets t of s
            exactly += (-1) ** (bin(s).count("1") - bin(t).count("1")) * inside[t]
            if t == 0:
                break
            t = (t - 1) & s
        out[bin(s).count("1")] += exactly
    return out


def occupancy_count(x, n, alpha, least=3):
    """Pairs of one total share alpha (the near-floor regime): (observed number of draws with reads in `least` bins or
    more, its exact expectation, P(Poisson(expectation) >= observed)).  With concentrations of 1e-3 nearly every draw
    puts all its reads into one bin; a sampler that loses the order of its gammas where they all underflow spreads such a
    draw over every bin."""
    D = x.shape[0]
    seen = int(((x > 0).sum(2) >= least).sum())
    expect = 0.0
    for t in sorted(set(n.reshape(-1).tolist())):
        rr, gg = np.nonzero(n == t)
        expect += D * len(rr) * occupancy_pmf(t, alpha[rr[0], :, gg[0]])[least:].sum()
    return seen, expect, float(stats.poisson.sf(seen - 1, expect))


def standardised(x, n, alpha, b=0):
    """(D, R, G) counts of bin b less their exact mean over their exact standard deviation; nan where the total is 0."""
    m, v = dm_moments(n.astype(np.float64), alpha, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x[:, :, b, :] - m[None]) / np.sqrt(np.where(v > 0, v, np.nan))[None]


def independence_checks(x, x_bc, n, alpha2):
    """[(label, correlation, bound)] between streams that must be independent, on bin 0."""
    z = standardised(x, n, alpha2[0])
    z_bc = standardised(x_bc, n, alpha2[1])
    out = [("X and X_bcmatch of one pair", *independence(z, z_bc)),
           ("guide g and g + 1", *independence(z[:, :, :-1], z[:, :, 1:])),
           ("draw d and d + 1", *independence(z[:-1], z[1:])),
           ("lane 63 of one tile and lane 0 of the next", *independence(z[:, :, 63], z[:, :, 64]))]
    if z.shape[1] > 1:
        out.append(("replicate 0 and 1 of one guide", *independence(z[:, 0], z[:, 1])))
    return out


INDEPENDENT = ("sparse", "moderate")  # (with the Normal family on the device: no shared pi links anything)


def evaluate(name, draws, n, alpha2, rng, likelihoods=("X",), family_label=None, independent=True):
    """Everything regime `name` asserts of a set of draws {"X": (D, R, B, G), "X_bcmatch": ...}: a report
    {"p": [(label, p)], "corr": [(label, r, bound)], "cov_z": [(label, z)], "floor": (seen, expectation, tail) or None}."""
    n = np.asarray(n, dtype=np.int64)
    report = {"name": family_label or name, "p": [], "corr": [], "cov_z": [], "floor": None, "occupancy": None}
    for key in likelihoods:
        x = np.asarray(draws[key]).astype(np.int64)
        al = alpha2[0 if key == "X" else 1]
        assert (x >= 0).all() and (x.sum(2) == n[None]).all(), "every pair keeps its total"
        report["p"] += [(f"{key} {label}", p) for label, p in law_pvalues(name, x, n, al, rng)]
    if name == "floor":
        report["floor"] = floor_count(np.asarray(draws["X"]), n, alpha2[0])
    if name == "near-floor":
        report["occupancy"] = occupancy_count(np.asarray(draws["X"]), n, alpha2[0])
    if independent and name in INDEPENDENT and "X_bcmatch" in draws:
        x, x_bc = np.asarray(draws["X"], dtype=np.float64), np.asarray(draws["X_bcmatch"], dtype=np.float64)
        report["corr"] = independence_checks(x, x_bc, n, alpha2)
        report["cov_z"] = [("X", pair_covariance_z(x, n, alpha2[0])), ("X_bcmatch", pair_covariance_z(x_bc, n, alpha2[1]))]
    return report


def failures(report):
    """The assertions of a report that do not hold, as text; empty when the draws follow the law."""
    bad = [f"p-value {label}: {p:.3e} <= {P_MIN:.3e}" for label, p in report["p"] if not p > P_MIN]
    bad += [f"correlation {label}: {r:+.4f} beyond {bound:.4f}" for label, r, bound in report["corr"] if not abs(r) <= bound]
    bad += [f"covariance {label}: z = {z:+.2f}" for label, z in report["cov_z"] if not abs(z) <= SIGMAS]
    if report["floor"] is not None:
        seen, expect, tail = report["floor"]
        if not expect < 5.0:
            bad.append(f"floor: expectation {expect:.3f} is not below 5")
        if not tail >= 1e-5:
            bad.append(f"floor: {seen} non-zero counts where {expect:.3f} are expected, Poisson tail {tail:.3e}")
    if report["occupancy"] is not None:
        seen, expect, tail = report["occupancy"]
        if not tail >= 1e-5:
            bad.append(f"occupancy: {seen} draws with reads in three bins or more where {expect:.3f} are expected, "
                       f"Poisson tail {tail:.3e}")
    return bad


def describe(report):
    p = [v for _, v in report["p"]]
    text = f"{report['name']}: {len(p)} p-values, smallest {min(p):.3e} (threshold {P_MIN:.3e})" if p else f"{report['name']}:"
    if report["corr"]:
        text += "; correlations " + ", ".join(f"{r:+.4f}/{b:.4f}" for _, r, b in report["corr"])
    if report["cov_z"]:
        text += "; covariance z " + ", ".join(f"{z:+.2f}" for _, z in report["cov_z"])
    if report["floor"] is not None:
        text += "; floor bins: %d non-zero, %.3f expected, tail %.3e" % report["floor"]
    if report["occupancy"] is not None:
        text += "; three bins or more occupied: %d draws, %.3f expected, tail %.3e" % report["occupancy"]
    return text
