"""What the depth-study tests share (test_design_cpu.py on the host, test_gpu_design.py on the device): the law a screen
drawn at depth f must follow - DM(floor(f n + 0.5), alpha) pair by pair, with the checks of dm_reference.py - the number of
p-values that takes, and the threshold that number sets.  A plain module imported by bare name; nothing here is code
under test and nothing here looks at a device."""
import numpy as np

import dm_reference as dm

LAW_DEPTHS = (0.5, 3.0)
LAW_DRAWS = 64  # one call: D = 1, K = 64
# sparse: the totals 0 ... 13 of dm.SPARSE_TOTALS become {0, 1, 2, 3, 4, 5, 7} at depth 0.5 (every odd total is rounded
# UP: truncation would give {0, 1, 2, 3, 4, 6}) and {0, 3, ..., 39} at depth 3; a total of 0 has one cell and no test.
# Every bin of every other total has at least the cells {0, >= 1} with 5 expected draws or more (N = 64 draws x >= 25
# pairs, a bin's share of the concentrations >= 0.1), so the number of chi-square tests does not depend on the draws.
N_PVALUES = {
    "moderate@0.5": 5,   # PIT per bin
    "moderate@3": 5,
    "sparse@0.5": 35,    # PIT per bin + 6 totals x 5 bins
    "sparse@3": 50,      # PIT per bin + 9 totals x 5 bins
}
N_P = sum(N_PVALUES.values())
P_MIN = 1e-3 / N_P  # the rule of dm_reference.py: the family-wise false-alarm rate of the file is at most 1e-3


def label(regime, depth):
    return f"{regime}@{depth:g}"


def scaled_totals(n, depth):
    """floor(depth * n + 0.5) in float64, (R, G) int64: what the kernel's design_total computes."""
    return np.floor(float(depth) * np.asarray(n, dtype=np.float64) + 0.5).astype(np.int64)


def law_report(regime, depth, x, n_obs, alpha, rng):
    """Draws x (D, R, B, G) of one likelihood at `depth` of the observed totals n_obs (R, G), concentrations alpha
    (R, B, G): {"totals": number of (draw, pair) whose counts do not add up to floor(depth n + 0.5), "p": [(label, p)]}.
    The p-values are computed only where every total is right (the tables are indexed by them)."""
    x = np.asarray(x).astype(np.int64)
    n = scaled_totals(n_obs, depth)
    wrong = int((x.sum(2) != n[None]).sum()) + int((x < 0).sum())
    report = {"name": label(regime, depth), "totals": wrong, "p": []}
    if wrong:
        return report
    report["p"] = [(f"PIT bin {b}", p) for b, p in dm.pit_marginals(x, n, alpha, rng)]
    if regime == "sparse":
        B = x.shape[2]
        for t in sorted(set(n.reshape(-1).tolist())):
            rr, gg = np.nonzero(n == t)
            al = alpha[rr[0], :, gg[0]]
            assert np.allclose(alpha[rr, :, gg], al[None, :], rtol=1e-6, atol=0), "pairs of one total share alpha"
            xs = x[:, rr, :, gg].reshape(-1, B)
            report["p"] += [(f"total {t} bin {b}", p) for b, p in dm.gof_marginals(xs, t, al)]
    return report


def failures(report):
    bad = [f"{report['totals']} (draw, pair) totals are not floor(f n + 0.5)"] if report["totals"] else []
    if not report["totals"] and len(report["p"]) != N_PVALUES[report["name"]]:
        bad.append(f"{len(report['p'])} p-values where {N_PVALUES[report['name']]} were counted")
    return bad + [f"p-value {text}: {p:.3e} <= {P_MIN:.3e}" for text, p in report["p"] if not p > P_MIN]


def describe(report):
    p = [v for _, v in report["p"]]
    tail = f"{len(p)} p-values, smallest {min(p):.3e} (threshold {P_MIN:.3e})" if p else "no p-values"
    return f"{report['name']}: {report['totals']} wrong totals; {tail}"


def host_alpha(regime):
    """(R, B, G) concentrations for the host sampler: per pair in the moderate regime, shared in the sparse one (its
    chi-square tests pool the pairs of one total)."""
    rng = np.random.default_rng(77) if regime == "moderate" else None
    return dm.regime_alpha(regime, rng)


def host_draws(regime, totals, seed, draws=LAW_DRAWS):
    """`draws` host screens (draws, R, B, G) of the regime's concentrations at the totals given."""
    al = host_alpha(regime)
    return dm.host_screens(np.asarray(totals, dtype=np.int64), al, draws, np.random.default_rng(seed))["X"], al[0]
