"""The implicit Dirichlet gradient ``-(dF / d alpha) / pdf / (1 - x)`` as the piecewise formula of
``dirichlet_grad_one_t`` (csrc/bean_special.hpp; torch's ATen/native/Distributions.h holds the same formulas), evaluated
exactly, and an error budget for a float64 evaluation of it that is derived from the formula alone.

Host only: numpy, scipy and mpmath.  Nothing here is code under test and nothing here looks at a device.  Imported by bare
name (as grad_bounds.py and dm_reference.py are).

* ``port(x, alpha, total)``: the formula at ``DPS`` digits from the float64 inputs - the value a float64 evaluation
  approximates.  Every intermediate in which a float64 evaluation loses something is passed through ``n(name, value)``;
  ``perturb=name`` scales that one by ``1 + 2^-52``.
* ``budget(x, alpha, total)``: ``sum_k |port(perturb=k) - port()|`` over the names of the branch taken - the first-order
  move of the result when each named intermediate is wrong by one ulp.  A float64 evaluation is held to

      |value - port| <= K (2^-52 |port| + budget)

  ``2^-52 |port|`` stands for the roundings that no cancellation amplifies.  K per branch is measured for torch's own
  evaluation and for ``port64`` (tests/test_dirichlet_grad_reference.py) and recorded in DESIGN.md section 5.
* ``classify(x, alpha, total)``: the branch by the header's comparisons in exact arithmetic, and the set of branches a
  point within ``EDGE_REL`` of an edge can fall into (the device forms ``mean`` and ``sd`` with its own reciprocal).
* ``port64``: the same formulas in numpy float64 with true division and libm ``log`` - a working-precision evaluation on
  the host, with switches for the three planted errors of the tests, and the oracle's implicit gradient where torch's
  cannot serve (concentrations above 2e3).
"""
from __future__ import annotations

import os
from fractions import Fraction
from itertools import product

import mpmath
import numpy as np
from scipy import special as sp

DPS = 60
ULP = 2.0 ** -52
EDGE_REL = 1e-12
DBL_MIN = float(np.finfo(np.float64).tiny)       # csrc/bean_kernels.hpp::kDblMin
ONE_MINUS = float(np.nextafter(1.0, 0.0))         # kOneMinus
BRANCHES = ("small_alpha", "small_beta", "near_mean", "saddle", "rational")
SMALL_ALPHA, SMALL_BETA, NEAR_MEAN, SADDLE, RATIONAL = range(5)
N_SMALL_ALPHA, N_SMALL_BETA = 10, 8              # terms of the two series

# kDirGradC restated: c[num/den][u^i][a^j][b^k].  test_coefficients_are_the_headers holds it to the header.
DIR_GRAD_C = np.array([
    [[[1.003668233, -0.01061107488, -0.0657888334, 0.01201642863],
      [0.6336835991, -0.3557432599, 0.05486251648, -0.001465281033],
      [-0.03276231906, 0.004474107445, 0.002429354597, -0.0001557569013]],
     [[0.221950385, -0.3187676331, 0.01799915743, 0.01074823814],
      [-0.2951249643, 0.06219954479, 0.01535556598, 0.001550077057],
      [0.02155310298, 0.004170831599, 0.001292462449, 6.976601077e-05]],
     [[-0.05980841433, 0.008441916499, 0.01085618172, 0.002319392565],
      [0.02911413504, 0.01400243777, -0.002721828457, 0.000751041181],
      [0.005900514878, -0.001936558688, -9.495446725e-06, 5.385558597e-05]]],
    [[[1, -0.02924021934, -0.04438342661, 0.007285809825],
      [0.6357567472, -0.3473456711, 0.05454656494, -0.002407477521],
      [-0.03301322327, 0.004845219414, 0.00231480583, -0.0002307248149]],
     [[0.5925320577, -0.1757678135, 0.01505928619, 0.000564515273],
      [0.1014815858, -0.06589186703, 0.01272886114, -0.0007316646956],
      [-0.007258481865, 0.001096195486, 0.0003934994223, -4.12701925e-05]],
     [[0.06469649321, -0.0236701437, 0.002902096474, -5.896963079e-05],
      [0.001925008108, -0.002869809258, 0.0008000589141, -6.063713228e-05],
      [-0.0003477407336, 6.959756487e-05, 1.097287507e-05, -1.650964693e-06]]],
], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the branch
def _near(v, edge):
    return abs(v - edge) <= EDGE_REL * abs(edge)


def classify(x, alpha, total):
    """``(branch, near_edge, reachable)``: the branch of the header's comparisons in exact arithmetic (rationals; the
    near-mean window, which holds a square root, at ``DPS`` digits), whether the point lies within ``EDGE_REL`` relative
    of one of the edges ``x = 0.5``, ``boundary = 2.5``, ``boundary = 0.75``, ``alpha = 6``, ``beta = 6``,
    ``x = mean +/- 0.1 sd`` - and which branches it reaches when every comparison that close whose operand an evaluation
    has to form (the boundary, beta, the window) is decided either way."""
    xf, af, tf = Fraction(float(x)), Fraction(float(alpha)), Fraction(float(total))
    bf = tf - af
    boundary = tf * xf * (1 - xf)
    half = Fraction(1, 2)
    with mpmath.workdps(DPS):
        xm, am, bm = mpmath.mpf(float(x)), mpmath.mpf(float(alpha)), mpmath.mpf(float(total)) - mpmath.mpf(float(alpha))
        tm = am + bm
        mean = am / tm
        sd = mpmath.sqrt(am * bm / (tm + 1)) / tm
        lo, hi = mean - mpmath.mpf(0.1) * sd, mean + mpmath.mpf(0.1) * sd
        in_lo, in_hi = bool(lo <= xm), bool(xm <= hi)
        near_lo, near_hi = bool(abs(xm - lo) <= EDGE_REL * abs(xm)), bool(abs(xm - hi) <= EDGE_REL * abs(xm))

    # each comparison: (its exact outcome, whether it is within EDGE_REL of its edge, whether an evaluation forms what it
    # compares - x and alpha are inputs, which every evaluation compares exactly)
    side = (xf > half) - (xf < half)  # -1, 0, 1
    comps = [(boundary < Fraction(5, 2), _near(boundary, Fraction(5, 2)), True),
             (boundary < Fraction(3, 4), _near(boundary, Fraction(3, 4)), True),
             (af > 6, _near(af, 6), False), (bf > 6, _near(bf, 6), True), (in_lo, near_lo, True), (in_hi, near_hi, True)]

    def branch_of(b25, b075, a6, b6, wlo, whi):
        if side <= 0 and b25:
            return SMALL_ALPHA
        if side >= 0 and b075:
            return SMALL_BETA
        if a6 and b6:
            return NEAR_MEAN if (wlo and whi) else SADDLE
        return RATIONAL

    exact = branch_of(*(c for c, _, _ in comps))
    options = [((c, not c) if (nr and formed) else (c,)) for c, nr, formed in comps]
    reach = {branch_of(*combo) for combo in product(*options)}
    near = _near(xf, half) or any(nr for _, nr, _ in comps)
    return exact, bool(near), tuple(sorted(reach))


# ---------------------------------------------------------------------------------------------------------------------
# the formula at DPS digits
class _Names:
    """``n(name, value)`` records the name and scales the value of the one that is perturbed."""

    def __init__(self, perturb=None):
        self.perturb, self.seen = perturb, []

    def __call__(self, name, value):
        self.seen.append(name)
        return value * (1 + mpmath.mpf(ULP)) if name == self.perturb else value


def _digamma(n, label, z):
    """digamma(z) as every float64 evaluation forms it below 10 (torch's ``digamma_one``, the device's ``shift_up``):
    the asymptotic value at z + m >= 10 less the shift sum ``1 / z + ... + 1 / (z + m - 1)`` - two intermediates, whose
    difference cancels at small z (the sum is 1 / z) and next to digamma's root at 1.4616."""
    m = max(0, int(mpmath.ceil(10 - z)))
    if m == 0:
        return n(label, mpmath.digamma(z))
    shift = mpmath.fsum(1 / (z + i) for i in range(m))
    return n(label + ": asymptotic part", mpmath.digamma(z + m)) - n(label + ": shift sum", shift)


def _small_alpha(n, x, alpha, beta):
    factor = _digamma(n, "digamma(alpha)", alpha) - _digamma(n, "digamma(alpha + beta)", alpha + beta) \
        - n("log x", mpmath.log(x))
    ra = n("1 / alpha", 1 / alpha)
    numer = mpmath.mpf(1)
    series = numer * ra * (factor + ra)
    for i in range(1, N_SMALL_ALPHA + 1):
        numer = n(f"numer_{i}", numer * (i - beta) * x / i)
        rd = n(f"1 / (alpha + {i})", 1 / (alpha + i))
        series += numer * rd * (factor + rd)
    return x * n("(1 - x)^(-beta)", mpmath.power(n("1 - x", 1 - x), -beta)) * series


def _small_beta(n, x, alpha, beta):
    factor = _digamma(n, "digamma(alpha + beta)", alpha + beta) - _digamma(n, "digamma(beta)", beta)
    numer, betas, dbetas = mpmath.mpf(1), mpmath.mpf(1), mpmath.mpf(0)
    series = factor * n("1 / alpha", 1 / alpha)
    for i in range(1, N_SMALL_BETA + 1):
        numer = n(f"numer_{i}", numer * -x / i)
        dbetas = n(f"dbetas_{i}", dbetas * (beta - i) + betas)
        betas = n(f"betas_{i}", betas * (beta - i))
        series += numer * n(f"1 / (alpha + {i})", 1 / (alpha + i)) * (dbetas + factor * betas)
    return -n("(1 - x)^(1 - beta)", mpmath.power(1 - x, 1 - beta)) * series


def _near_mean(n, x, alpha, beta):
    total = alpha + beta
    b2 = beta * beta
    poly = 47 * x * b2 * b2 + alpha * ((43 + 20 * (16 + 27 * beta) * x) * b2 * beta + alpha * (
        3 * (59 + 180 * beta - 90 * x) * b2 + alpha * (
            (453 + 1620 * beta * (1 - x) - 455 * x) * beta + alpha * (8 * (1 - x) * (135 * beta - 11)))))
    pre_num = n("pre_num", (1 + 12 * alpha) * (1 + 12 * beta) / (total * total))
    pre_den = n("pre_den", 12960 * alpha * alpha * alpha * beta * beta * (1 + 12 * total))
    return pre_num * n("poly", poly) / ((1 - x) * pre_den)


def _saddle(n, x, alpha, beta, c288=288):
    total = alpha + beta
    mean = alpha / total
    prefactor = -x / mpmath.sqrt(2 * alpha * beta / total)
    st = lambda z: 1 + 1 / (12 * z) + 1 / (c288 * z * z)  # noqa: E731
    stirling = st(alpha) * st(beta) / st(total)
    term1_num = 2 * (alpha * alpha) * (x - 1) + alpha * beta * (x - 1) - x * (beta * beta)
    axbx = n("axbx: alpha (x - 1)", alpha * (x - 1)) + n("axbx: beta x", beta * x)
    term1_den = mpmath.sqrt(2 * alpha / beta) * (total * mpmath.sqrt(total)) * axbx * axbx
    term1 = n("term1", term1_num / term1_den)
    la = n("la", mpmath.log(n("la: alpha / (total x)", alpha / (total * x))))
    lb = n("lb", mpmath.log(n("lb: beta / (total (1 - x))", beta / (total * (1 - x)))))
    term2 = la / 2
    term3 = mpmath.sqrt(8 * alpha * beta / total) / axbx
    term4_base = n("term4_base: beta lb", beta * lb) + n("term4_base: alpha la", alpha * la)
    term4 = 1 / (term4_base * mpmath.sqrt(term4_base))
    t23 = n("term2 term3", term2 * term3)
    t24 = n("term2 term4", term2 * term4)
    return stirling * prefactor * (term1 + t23 + (t24 if x < mean else -t24))


def _rational(n, x, alpha, total, beta, coef=DIR_GRAD_C):
    u = n("log x", mpmath.log(x))
    a = n("log alpha", mpmath.log(alpha)) - u
    b = n("log total", mpmath.log(total)) - a
    pow_u, pow_a = (1, u, u * u), (1, a, a * a)
    p = q = mpmath.mpf(0)
    c = [[[[mpmath.mpf(float(v)) for v in r] for r in m] for m in h] for h in coef]
    for i in range(3):
        for j in range(3):
            ua = pow_u[i] * pow_a[j]
            p += ua * (c[0][i][j][0] + b * (c[0][i][j][1] + b * (c[0][i][j][2] + b * c[0][i][j][3])))
            q += ua * (c[1][i][j][0] + b * (c[1][i][j][1] + b * (c[1][i][j][2] + b * c[1][i][j][3])))
    dd = _digamma(n, "digamma(total)", total) - _digamma(n, "digamma(alpha)", alpha)
    return n("p", p) * (x * dd / beta) / n("q", q)


def _port(x, alpha, total, branch, names):
    x, alpha, total = (mpmath.mpf(float(v)) for v in (x, alpha, total))
    beta = names("beta", total - alpha)
    if branch == SMALL_ALPHA:
        return _small_alpha(names, x, alpha, beta)
    if branch == SMALL_BETA:
        return -_small_beta(names, 1 - x, beta, alpha)
    if branch == NEAR_MEAN:
        return _near_mean(names, x, alpha, beta)
    if branch == SADDLE:
        return _saddle(names, x, alpha, beta)
    return _rational(names, x, alpha, total, beta)


def port(x, alpha, total, branch=None, perturb=None):
    """``(value, branch)``: the formula of ``branch`` (default: the one ``classify`` gives) at ``DPS`` digits, as an
    ``mpmath.mpf``; ``perturb`` names the intermediate that is scaled by ``1 + 2^-52``."""
    if branch is None:
        branch = classify(x, alpha, total)[0]
    with mpmath.workdps(DPS):
        return +_port(x, alpha, total, branch, _Names(perturb)), branch


def names_of(x, alpha, total, branch=None):
    """The named intermediates of the branch taken."""
    if branch is None:
        branch = classify(x, alpha, total)[0]
    names = _Names()
    with mpmath.workdps(DPS):
        _port(x, alpha, total, branch, names)
    return list(names.seen)


def budget(x, alpha, total, branch=None):
    """``sum_k |port(perturb=k) - port()|`` over every named intermediate of the branch, as an ``mpmath.mpf``."""
    ref, branch = port(x, alpha, total, branch)
    with mpmath.workdps(DPS):
        out = mpmath.mpf(0)
        for k in names_of(x, alpha, total, branch):
            out += abs(port(x, alpha, total, branch, perturb=k)[0] - ref)
        return +out


def reference_point(x, alpha, total):
    """What the fixture stores of a point: ``(branch, near_edge, ref, budget / |ref|, branch2, ref2, budget2 / |ref2|)``,
    all floats; the second branch (NaN where the point is not near an edge) is the other one the point reaches.  The
    budget is stored relative to the value because a value of 1e-300 (a draw on the DBL_MIN floor) has a budget that is
    not a normal double."""
    br, near, reach = classify(x, alpha, total)
    assert len(reach) <= 2, (x, alpha, total, reach)

    def one(b):
        ref, _ = port(x, alpha, total, b)
        with mpmath.workdps(DPS):
            return float(ref), float(budget(x, alpha, total, b) / abs(ref))

    ref, rel = one(br)
    if len(reach) == 2:
        other = reach[0] if reach[1] == br else reach[1]
        ref2, rel2 = one(other)
    else:
        other, ref2, rel2 = np.nan, np.nan, np.nan
    return float(br), float(near), ref, rel, float(other), ref2, rel2


def rule_ratio(value, ref, budget_rel):
    """``|value - ref| / (2^-52 |ref| + budget)``: the K a value needs (float64 arrays; the budget relative to |ref|)."""
    value, ref, budget_rel = (np.asarray(v, dtype=np.float64) for v in (value, ref, budget_rel))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(value / ref - 1.0) / (ULP + budget_rel)


# ---------------------------------------------------------------------------------------------------------------------
# the formula in float64
def branch64(x, alpha, total):
    """The branch by the header's comparisons in float64, same operations in the same order (true division)."""
    x, alpha, total = (np.asarray(v, dtype=np.float64) for v in (x, alpha, total))
    beta = total - alpha
    boundary = total * x * (1.0 - x)
    small_a = (x <= 0.5) & (boundary < 2.5)
    small_b = (x >= 0.5) & (boundary < 0.75) & ~small_a
    big = ~small_a & ~small_b & (alpha > 6.0) & (beta > 6.0)
    with np.errstate(all="ignore"):
        tot = alpha + beta
        mean = alpha / tot
        sd = np.sqrt(alpha * beta / (tot + 1.0)) / tot
    window = (mean - 0.1 * sd <= x) & (x <= mean + 0.1 * sd)
    return np.where(small_a, SMALL_ALPHA, np.where(small_b, SMALL_BETA,
                    np.where(big & window, NEAR_MEAN, np.where(big, SADDLE, RATIONAL))))


def _plain(name, value):
    return value


def _digamma64(n, label, z):
    """scipy's digamma; under ``budget64`` the two intermediates of ``_digamma`` (asymptotic part, shift sum)."""
    if n is _plain:
        return sp.digamma(z)
    m = np.maximum(0.0, np.ceil(10.0 - z))
    shift = np.zeros_like(z)
    for i in range(10):
        shift = shift + np.where(i < m, 1.0 / (z + i), 0.0)
    return n(label + ": asymptotic part", sp.digamma(z + m)) - n(label + ": shift sum", shift)


def _small_alpha64(n, x, alpha, beta, n_terms):
    factor = _digamma64(n, "digamma(alpha)", alpha) - _digamma64(n, "digamma(alpha + beta)", alpha + beta) \
        - n("log x", np.log(x))
    ra = n("1 / alpha", 1.0 / alpha)
    numer = np.ones_like(x)
    series = numer * ra * (factor + ra)
    for i in range(1, n_terms + 1):
        ci = float(i)
        numer = n(f"numer_{i}", numer * ((ci - beta) * x / ci))
        rd = n(f"1 / (alpha + {i})", 1.0 / (alpha + ci))
        series = series + numer * rd * (factor + rd)
    return x * n("(1 - x)^(-beta)", np.exp(-beta * np.log(n("1 - x", 1.0 - x)))) * series


def _small_beta64(n, x, alpha, beta):
    factor = _digamma64(n, "digamma(alpha + beta)", alpha + beta) - _digamma64(n, "digamma(beta)", beta)
    numer, betas, dbetas = np.ones_like(x), np.ones_like(x), np.zeros_like(x)
    series = factor * n("1 / alpha", 1.0 / alpha)
    for i in range(1, N_SMALL_BETA + 1):
        ci = float(i)
        numer = n(f"numer_{i}", numer * (-x / ci))
        dbetas = n(f"dbetas_{i}", dbetas * (beta - ci) + betas)
        betas = n(f"betas_{i}", betas * (beta - ci))
        series = series + numer * n(f"1 / (alpha + {i})", 1.0 / (alpha + ci)) * (dbetas + factor * betas)
    return -n("(1 - x)^(1 - beta)", np.exp((1.0 - beta) * np.log(1.0 - x))) * series


def _near_mean64(n, x, alpha, beta):
    total = alpha + beta
    b2 = beta * beta
    poly = 47.0 * x * b2 * b2 + alpha * ((43.0 + 20.0 * (16.0 + 27.0 * beta) * x) * b2 * beta + alpha * (
        3.0 * (59.0 + 180.0 * beta - 90.0 * x) * b2 + alpha * (
            (453.0 + 1620.0 * beta * (1.0 - x) - 455.0 * x) * beta + alpha * (8.0 * (1.0 - x) * (135.0 * beta - 11.0)))))
    pre_num = n("pre_num", (1.0 + 12.0 * alpha) * (1.0 + 12.0 * beta) / total / total)
    pre_den = n("pre_den", 12960.0 * alpha * alpha * alpha * beta * beta * (1.0 + 12.0 * total))
    return pre_num * n("poly", poly) / ((1.0 - x) * pre_den)


def _saddle64(n, x, alpha, beta, c288):
    total = alpha + beta
    mean = alpha / total
    ra, rb, rtot = 1.0 / alpha, 1.0 / beta, 1.0 / total
    prefactor = -x / np.sqrt(2.0 * alpha * beta / total)
    stirling = ((1.0 + ra / 12.0 + ra * ra / c288) * (1.0 + rb / 12.0 + rb * rb / c288)
                / (1.0 + rtot / 12.0 + rtot * rtot / c288))
    term1_num = 2.0 * (alpha * alpha) * (x - 1.0) + alpha * beta * (x - 1.0) - x * (beta * beta)
    axbx = n("axbx: alpha (x - 1)", alpha * (x - 1.0)) + n("axbx: beta x", beta * x)
    term1_den = np.sqrt(2.0 * alpha / beta) * (total * np.sqrt(total)) * axbx * axbx
    term1 = n("term1", term1_num / term1_den)
    la = n("la", np.log(n("la: alpha / (total x)", alpha / (total * x))))
    lb = n("lb", np.log(n("lb: beta / (total (1 - x))", beta / (total * (1.0 - x)))))
    term2 = 0.5 * la
    term3 = np.sqrt(8.0 * alpha * beta / total) / axbx
    term4_base = n("term4_base: beta lb", beta * lb) + n("term4_base: alpha la", alpha * la)
    term4 = 1.0 / (term4_base * np.sqrt(term4_base))
    t23, t24 = n("term2 term3", term2 * term3), n("term2 term4", term2 * term4)
    return stirling * prefactor * (term1 + (t23 + np.where(x < mean, t24, -t24)))


def _rational64(n, x, alpha, total, beta, coef):
    u = n("log x", np.log(x))
    a = n("log alpha", np.log(alpha)) - u
    b = n("log total", np.log(total)) - a
    pow_u, pow_a = (1.0, u, u * u), (1.0, a, a * a)
    p, q = np.zeros_like(x), np.zeros_like(x)
    c = coef
    for i in range(3):
        for j in range(3):
            ua = pow_u[i] * pow_a[j]
            p = p + ua * (c[0][i][j][0] + b * (c[0][i][j][1] + b * (c[0][i][j][2] + b * c[0][i][j][3])))
            q = q + ua * (c[1][i][j][0] + b * (c[1][i][j][1] + b * (c[1][i][j][2] + b * c[1][i][j][3])))
    approx = x * (_digamma64(n, "digamma(total)", total) - _digamma64(n, "digamma(alpha)", alpha)) / beta
    return n("p", p) * approx / n("q", q)


def _branch64_value(n, b, xs, al, be, to, c288=288.0, coef=DIR_GRAD_C, n_terms=N_SMALL_ALPHA):
    be = n("beta", be)
    if b == SMALL_ALPHA:
        v = _small_alpha64(n, xs, al, be, n_terms)
        return np.where(np.isnan(v), 0.0, v)
    if b == SMALL_BETA:
        v = _small_beta64(n, 1.0 - xs, be, al)
        return -np.where(np.isnan(v), 0.0, v)
    if b == NEAR_MEAN:
        return _near_mean64(n, xs, al, be)
    if b == SADDLE:
        return _saddle64(n, xs, al, be, c288)
    return _rational64(n, xs, al, to, be, coef)


def port64(x, alpha, total, branch=None, c288=288.0, coef=DIR_GRAD_C, n_terms=N_SMALL_ALPHA, with_branch=False):
    """The formula in numpy float64 (true division, libm ``log``, scipy's ``digamma``), any shape; the branch is
    ``branch64``'s unless given.  ``c288``, ``coef`` and ``n_terms`` plant the errors of
    tests/test_dirichlet_grad_reference.py.  As in the header a NaN of either series becomes 0."""
    x, alpha, total = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (x, alpha, total)))
    br = branch64(x, alpha, total) if branch is None else np.broadcast_to(np.asarray(branch), x.shape)
    beta = total - alpha
    out = np.empty(x.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for b in range(5):
            m = br == b
            if not m.any():
                continue
            out[m] = _branch64_value(_plain, b, x[m], alpha[m], beta[m], total[m], c288, coef, n_terms)
    return (out, br) if with_branch else out


FD_STEP = 2.0 ** -26  # budget64's perturbation: first order to 1e-8, far above the float64 noise of the difference


def budget64(x, alpha, total):
    """``(value, budget / |value|, branch)`` in float64, vectorised: ``port64`` and the budget of ``budget`` by finite
    differences - each named intermediate scaled by ``1 + FD_STEP`` in the float64 formulas, the moves added and scaled
    back to one ulp.  For the hundreds of evaluations of a screen, where ``budget`` itself would take seconds;
    test_budget64_is_the_budget holds it to the fixture's 60-digit budgets."""
    x, alpha, total = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (x, alpha, total)))
    br = branch64(x, alpha, total)
    beta = total - alpha
    value, rel = np.empty(x.shape), np.empty(x.shape)
    with np.errstate(all="ignore"):
        for b in range(5):
            m = br == b
            if not m.any():
                continue
            args = (b, x[m], alpha[m], beta[m], total[m])
            seen = []
            base = _branch64_value(lambda name, v: (seen.append(name), v)[1], *args)
            moved = np.zeros_like(base)
            for k in seen:
                moved += np.abs(_branch64_value(lambda name, v, k=k: v * (1.0 + FD_STEP) if name == k else v, *args) - base)
            value[m], rel[m] = _branch64_value(_plain, *args), moved * (ULP / FD_STEP) / np.abs(base)
    return value, rel, br


def port64_torch(x, concentration, total):
    """``port64`` with the signature of ``torch._dirichlet_grad``: the oracle's alternative implicit gradient."""
    import torch

    out = port64(x.detach().cpu().numpy(), concentration.detach().cpu().numpy(), total.detach().cpu().numpy())
    return torch.as_tensor(out, dtype=x.dtype)


def header_coefficients(path):
    """The 72 doubles of ``kDirGradC`` as csrc/bean_special.hpp holds them."""
    import re

    text = open(path).read()
    body = text[text.index("kDirGradC[2][3][3][4] = {"):]
    body = body[body.index("{") + 1:body.index("};")]
    vals = [float(v) for v in re.findall(r"-?\d+\.?\d*(?:[eE][-+]?\d+)?", body)]
    assert len(vals) == 72, len(vals)
    return np.array(vals).reshape(2, 3, 3, 4)


# ---------------------------------------------------------------------------------------------------------------------
# the fixture and the rule
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dirichlet_grad_cases.npz")
K_MAX = 64.0      # no float64 evaluation on the host may need more in any branch (the condition on the list of names)
DEVICE_FACTOR = 4.0  # the device's reciprocal and log against true division and libm log: K_dev = 4 K_torch


def load_fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def fixture_ratio(value, f, exact_edges=True):
    """Per fixture point, the K that ``value`` needs: ``rule_ratio`` against the point's branch, or - near an edge, unless
    the point is planted exactly on it - against whichever of its two branches is nearer.  Also the branch matched."""
    r1 = rule_ratio(value, f["ref"], f["budget_rel"])
    two = ~np.isnan(f["branch2"])
    if exact_edges:
        two &= f["exact_edge"] == 0
    r2 = np.where(two, rule_ratio(value, np.where(two, f["ref2"], 1.0), np.where(two, f["budget2_rel"], 0.0)), np.inf)
    r1 = np.where(np.isfinite(np.asarray(value, dtype=np.float64)), r1, np.inf)
    second = r2 < r1
    return np.where(second, r2, r1), np.where(second, f["branch2"], f["branch"]).astype(int)


def needed_k(value, f):
    """The smallest K per branch (of the branch matched) with which ``value`` meets the rule on the whole fixture, and
    the index of the point that needs it."""
    ratio, br = fixture_ratio(value, f)
    ks, at = np.zeros(5), np.zeros(5, dtype=int)
    for b in range(5):
        idx = np.nonzero(br == b)[0]
        j = idx[int(np.argmax(ratio[idx]))]
        ks[b], at[b] = ratio[j], j
    return ks, at


def torch_values(f):
    import torch

    return torch._dirichlet_grad(torch.tensor(f["x"]), torch.tensor(f["alpha"]), torch.tensor(f["total"])).numpy()


def device_k(f=None):
    """``K_dev`` per branch: ``DEVICE_FACTOR`` times the K torch's float64 evaluation needs on the fixture."""
    f = load_fixture() if f is None else f
    return DEVICE_FACTOR * needed_k(torch_values(f), f)[0]


def path_allowance(k_dev, record=None):
    """For ``grad_bounds.elementwise_bounds``: per evaluation ``K_dev[branch] (2^-52 |g| + budget)`` with ``budget64``
    at the evaluation's own inputs.  ``record`` (a list) receives ``(x, alpha, total, branch)`` arrays."""
    import torch

    def allowance(x, conc, total, dgrad):
        xs, al, to = (t.detach().cpu().double().numpy() for t in (x, conc, total))
        value, rel, br = budget64(xs, al, to)
        assert np.array_equal(value, dgrad.detach().cpu().double().numpy())  # the oracle's gradient is port64
        if record is not None:
            record.append((xs.reshape(-1), al.reshape(-1), to.reshape(-1), br.reshape(-1)))
        return torch.as_tensor(np.asarray(k_dev)[br] * (ULP + rel) * np.abs(value), dtype=dgrad.dtype)

    return allowance
