"""Float64 restatement of the Gauss-Jacobi rule for the pairs section 21's predicate leaves out (DESIGN.md section 23;
csrc/bean_jacobi.hpp): the nodes and log weights from numpy's symmetric eigensolver on the Jacobi matrix, the rule on
marginal_reference.PairIntegrand, the combined rule (Gauss-Hermite where the pair is resolved, Gauss-Jacobi where it is
not), and the marginal log joint / exact moments built on the combined rule.  A plain module imported by bare name."""
import math

import numpy as np
import torch

import marginal_reference as mr
from oracle import elbo

TAIL_NODES = 64        # kTailNodes: the value
TAIL_CHECK_NODES = 48  # kTailCheckNodes: a second, independent value; tail_err = |J64 - J48|
TAIL_BOUND = 1e-3      # section 21's BOUND, nat per pair
_cache = {}


def jacobi_matrix(a, b, Q):
    """Diagonal d (Q) and off-diagonal e (Q - 1; e[n - 1] = e_n) of the Jacobi matrix of the weight
    z^(b - 1) (1 - z)^(a - 1) on (0, 1), in forms without a 1 + t cancellation."""
    al, be = a - 1.0, b - 1.0
    c = al + be
    n = np.arange(1, Q, dtype=np.float64)
    s = 2.0 * n + c
    d = np.empty(Q)
    d[0] = (1.0 + be) / (c + 2.0)
    d[1:] = (2.0 * n * (n + c + 1.0) + c * (1.0 + be)) / (s * (s + 2.0))
    e = np.empty(Q - 1)
    e[0] = math.sqrt((1.0 + al) * (1.0 + be) / (3.0 + c)) / (2.0 + c)
    m, sm = n[1:], s[1:]
    e[1:] = np.sqrt(m * (m + al) * (m + be) * (m + c) / ((sm - 1.0) * (sm + 1.0))) / sm
    return d, e


def _recurrence(x, d, e, e_last):
    """p_k(x), k < Q, of the orthonormal recurrence with p_0 = 1, then p_Q and p_Q' (up to e_last's scale)."""
    Q = d.size
    pm, p = np.zeros_like(x), np.ones_like(x)
    dm, dp = np.zeros_like(x), np.zeros_like(x)
    total = np.ones_like(x)
    for k in range(Q):
        ek = e[k - 1] if k > 0 else 0.0
        en = e[k] if k + 1 < Q else e_last
        pn = ((x - d[k]) * p - ek * pm) / en
        dn = ((x - d[k]) * dp + p - ek * dm) / en
        pm, p, dm, dp = p, pn, dp, dn
        if k + 1 < Q:
            total = total + p * p
    return total, p, dp


def gauss_jacobi(a, b, Q, polish=2):
    """Nodes z_i (ascending) and log weights of the Q-node Gauss-Jacobi rule for z^(b - 1) (1 - z)^(a - 1) on (0, 1), the
    weights normalised to sum 1: eigenvalues of the Jacobi matrix (numpy), ``polish`` Newton steps on the orthonormal
    recurrence, Christoffel numbers 1 / sum_k p_k(z_i)^2."""
    key = (float(a), float(b), int(Q), int(polish))
    if key not in _cache:
        d, e = jacobi_matrix(float(a), float(b), Q)
        z = np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
        Qf = float(Q)
        al, be = a - 1.0, b - 1.0
        c = al + be
        sQ = 2.0 * Qf + c
        e_last = math.sqrt(Qf * (Qf + al) * (Qf + be) * (Qf + c) / ((sQ - 1.0) * (sQ + 1.0))) / sQ
        for _ in range(polish):
            _, p, dp = _recurrence(z, d, e, e_last)
            z = z - p / dp
        total, _, _ = _recurrence(z, d, e, e_last)
        _cache[key] = (z, -np.log(total))
    return _cache[key]


def side_of(a_prime):
    """(..., ) bool: the smaller exponent is pi_1's (ties: pi_1)."""
    return a_prime[..., 1] <= a_prime[..., 0]


def jacobi_rule(h, a_prime, Q, where=None):
    """log int exp(h(u)) du per pair (R, G) by the Q-node Gauss-Jacobi rule in z, the share of the smaller exponent's
    side: lbeta(a0', a1') + logsumexp_i(lw_i + lg(z_i)), lg(z) = h(u(z)) - a0' log pi_0 - a1' log pi_1.  ``where`` (R, G)
    bool: the pairs to form (the others get 0, evaluated at z = 1/2)."""
    a0, a1 = a_prime[..., 0], a_prime[..., 1]
    R, G = a0.shape
    one = side_of(a_prime)
    small, big = torch.where(one, a1, a0), torch.where(one, a0, a1)
    z = torch.full((Q, R * G), 0.5, dtype=torch.float64)
    lw = torch.zeros((Q, R * G), dtype=torch.float64)
    at = torch.nonzero((torch.ones_like(one) if where is None else where).reshape(-1)).reshape(-1)
    if at.numel():
        # one rule per distinct pair of exponents (tiled copies of a guide share theirs)
        ab, inverse = torch.unique(torch.stack([big.reshape(-1)[at], small.reshape(-1)[at]], -1), dim=0, return_inverse=True)
        rules = [gauss_jacobi(float(a), float(b), Q) for a, b in ab.tolist()]
        z[:, at] = torch.from_numpy(np.stack([r[0] for r in rules], -1))[:, inverse]
        lw[:, at] = torch.from_numpy(np.stack([r[1] for r in rules], -1))[:, inverse]
    z, lw = z.reshape(Q, R, G), lw.reshape(Q, R, G)
    lz, l1z = z.log(), torch.log1p(-z)
    u = torch.where(one[None], lz - l1z, l1z - lz)
    lg = h(u) - small[None] * lz - big[None] * l1z
    out = torch.lgamma(a0) + torch.lgamma(a1) - torch.lgamma(a0 + a1) + torch.logsumexp(lw + lg, 0)
    return out if where is None else torch.where(where, out, torch.zeros_like(out))


def combined_rule(h, a_prime, Q, tail_nodes=TAIL_NODES):
    """Section 21's rule at Q where the pair is resolved, the Gauss-Jacobi rule at ``tail_nodes`` where it is not."""
    ok = a_prime.min(-1).values >= mr.MARG_MIN_CONC
    gh = mr.mode_centred_rule(h, a_prime, Q)
    if bool(ok.all()):
        return gh
    return torch.where(ok, gh, jacobi_rule(h, a_prime, tail_nodes, where=~ok))


def grid_terms(data, params, mu_t, y_t, Q, use_bcmatch=True, prior_params=None, ctrl=None):
    """What bean_hip_marginal_grid_tail forms at ONE node (mu_t, y_t) per target: lj (T,), the pair terms (R, G), the
    pairs' tail_err |J64 - J48| (R, G; 0 at resolved pairs), tail_err per target (T,), and the summed magnitudes of the
    terms of lj (T,), of each pair (R, G) and of the two log integrals of tail_err (R, G)."""
    data64 = elbo.as_float64(data)
    T = data.n_targets
    c_p = mr.model_conc(data, params)
    a_prime = mr.beta_exponents(data64, c_p, ctrl)
    h = mr.PairIntegrand(data64, mu_t, y_t.exp(), c_p, use_bcmatch, ctrl=ctrl)
    rg = data.repguide_mask
    tail = (~(a_prime.min(-1).values >= mr.MARG_MIN_CONC)) & rg
    full = mr.mode_centred_rule(h, a_prime, Q)
    j64 = jacobi_rule(h, a_prime, TAIL_NODES, where=tail)
    j48 = jacobi_rule(h, a_prime, TAIL_CHECK_NODES, where=tail)
    full = torch.where(tail, j64, full)
    lognorm = torch.lgamma(c_p.sum(-1)) - torch.lgamma(c_p).sum(-1)
    zero = torch.zeros_like(full)
    pairs = torch.where(rg, full - lognorm[None], zero)
    norm = torch.where(rg, lognorm[None].expand_as(full), zero)
    pair_mag = pairs.abs() + norm.abs()
    err = torch.where(tail, (j64 - j48).abs(), zero)
    err_mag = torch.where(tail, (j64 - lognorm[None]).abs() + (j48 - lognorm[None]).abs() + 2.0 * norm.abs(), zero)
    g2t = torch.repeat_interleave(torch.arange(T), data.target_lengths)
    add = lambda v: torch.zeros(T, dtype=torch.float64).index_add_(0, g2t, v.sum(0))  # noqa: E731
    p_mu, p_sd = elbo._priors((T, 1), 0.01, prior_params)
    lp_mu = p_mu.log_prob(mu_t.reshape(T, 1)).reshape(T)
    lp_sd = p_sd.log_prob(y_t.exp().reshape(T, 1)).reshape(T)
    lj = add(pairs + norm) + lp_mu + lp_sd + y_t
    mag = add(pair_mag) + lp_mu.abs() + lp_sd.abs() + y_t.abs()
    return {"lj": lj, "pairs": pairs, "pair_err": err, "tail_err": add(err), "mag": mag, "pair_mag": pair_mag,
            "err_mag": err_mag, "tail": tail}


def marginal_log_joint(sub, c_p, mu, y, Q=32, use_bcmatch=True, sd_scale=0.01, tail_nodes=TAIL_NODES, with_err=False):
    """marginal_reference.marginal_log_joint with the combined rule inside; ``with_err``: also the summed |J64 - J48| of
    the target's tail pairs per point."""
    assert sub.n_targets == 1
    K, G = mu.numel(), sub.n_guides
    tiled = mr.tile_guides(sub, K)
    cp = c_p.repeat(K, 1)
    h = mr.PairIntegrand(tiled, mu.repeat_interleave(G), y.exp().repeat_interleave(G), cp, use_bcmatch, per_guide=True)
    a_prime = mr.beta_exponents(tiled, cp)
    tail = (~(a_prime.min(-1).values >= mr.MARG_MIN_CONC)) & tiled.repguide_mask
    pairs = mr.mode_centred_rule(h, a_prime, Q)
    zero = torch.zeros_like(pairs)
    err = zero
    if bool(tail.any()):
        value = jacobi_rule(h, a_prime, tail_nodes, where=tail)
        pairs = torch.where(tail, value, pairs)
        if with_err:
            j64 = value if tail_nodes == TAIL_NODES else jacobi_rule(h, a_prime, TAIL_NODES, where=tail)
            err = (j64 - jacobi_rule(h, a_prime, TAIL_CHECK_NODES, where=tail)).abs()
    pairs = torch.where(tiled.repguide_mask, pairs, zero)
    p_mu, p_sd = elbo._priors((K,), sd_scale, None)
    lj = pairs.reshape(sub.n_reps, K, G).sum((0, 2)) + p_mu.log_prob(mu) + p_sd.log_prob(y.exp()) + y
    if not with_err:
        return lj
    return lj, err.reshape(sub.n_reps, K, G).sum((0, 2))


def exact_marginal_moments(sub, c_p, tail_nodes=128, **kw):
    """marginal_reference.exact_marginal_moments with the ``tail_nodes``-node Jacobi rule inside for tail pairs (Q = 64
    Gauss-Hermite for the others, as there)."""
    inner = mr.marginal_log_joint
    mr.marginal_log_joint = lambda s, c, m, y, Q=64, use_bcmatch=True, sd_scale=0.01: marginal_log_joint(  # noqa: E731
        s, c, m, y, Q=Q, use_bcmatch=use_bcmatch, sd_scale=sd_scale, tail_nodes=tail_nodes)
    try:
        return mr.exact_marginal_moments(sub, c_p, **kw)
    finally:
        mr.marginal_log_joint = inner
