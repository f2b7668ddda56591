"""Float64 restatement of the importance weights with pi integrated out, from the oracle's own
functions: the log integrand of a (replicate, guide) pair in u = logit(pi_1), the Q-node mode-centred Gauss-Hermite rule,
a dense composite Simpson rule as the independent reference, and the per-target marginal log weights built from them.
A plain module imported by bare name (test_marginal_reference.py, test_importance_marginal_cpu.py,
test_gpu_importance_marginal.py)."""
import math

import numpy as np
import torch
import torch.distributions as tdist

from oracle import elbo

MARG_MIN_CONC = 2.0   # kMargMinConc: a pair is resolved where min(a0', a1') >= this
NEWTON_STEPS = 4      # kMargNewton: damped Newton steps towards the mode, the same count for every pair
FD_STEP = 0.1         # kMargFd: the difference step of gradient and curvature, in units of the Beta factor's scale
STEP_CAP = 2.0        # kMargStepCap: a Newton step is clamped to +- this many Beta scales
NODES = (16, 32, 64)


def gauss_hermite(Q):
    """Nodes x_i and log-weights log w_i + x_i^2 of the Q-node Gauss-Hermite rule (weight exp(-x^2)), so that
    int f(u) du ~ sqrt(2) sigma sum_i exp(lw_i) f(m + sqrt(2) sigma x_i)."""
    x, w = np.polynomial.hermite.hermgauss(Q)
    return torch.tensor(x, dtype=torch.float64), torch.tensor(np.log(w) + x * x, dtype=torch.float64)


def model_conc(data, params):
    """c_p (G, 2): the model-side Dirichlet concentrations of the pi site, alpha_pi / sum alpha_pi * pi_a0, the
    exponential taken in the parameter's own dtype."""
    al = params["alpha_pi"].detach().cpu().exp().double().reshape(data.n_guides, 2)
    return al / al.sum(-1, keepdim=True) * data.pi_a0.double()[:, None]


def beta_exponents(data, c_p, ctrl=None):
    """a' (R, G, 2) = c_p + control allele counts summed over the control conditions: the exponents of the Beta-shaped
    factor pi_0^a0' pi_1^a1' of the integrand in u."""
    ctrl = data.allele_counts_control.double() if ctrl is None else ctrl
    return c_p[None] + ctrl.sum(1)


def resolved(data, c_p, ctrl=None):
    """(R, G) bool: the validity predicate of the rule.  Draw-independent."""
    return beta_exponents(data, c_p, ctrl).min(-1).values >= MARG_MIN_CONC


class PairIntegrand:
    """h(u)[n, r, g]: the log of the pair's integrand in u = logit(pi_1) at (mu_t, sd_t) of its target (and, with
    accessibility, the guide's drawn noise), Jacobian pi_0 pi_1 and the Dirichlet normaliser of c_p included:

        [n > mask_thres] log DirMult(x | alpha(pi)) (and X_bcmatch) + log Multinomial(control counts | pi)
        + log Dirichlet(pi; c_p) + log pi_0 + log pi_1

    Every site under the repguide mask is part of f; where the mask is off the pair's weight is 0 and h is not used."""

    def __init__(self, data, mu_t, sd_t, c_p, use_bcmatch=True, scale_by_accessibility=False, lpn=None, ctrl=None,
                 mask_thres=10, per_guide=False):
        self.data = data = elbo.as_float64(data)
        self.R, self.B, self.G = data.n_reps, data.n_condits, data.n_guides
        T = self.G if per_guide else data.n_targets  # per_guide: (mu, sd) given guide by guide (tile_guides)
        mu_t = torch.as_tensor(mu_t, dtype=torch.float64).reshape(T, 1)
        sd_t = torch.as_tensor(sd_t, dtype=torch.float64).reshape(T, 1)
        mu = torch.cat([torch.zeros((T, 1), dtype=torch.float64), mu_t], -1)
        sd = torch.cat([torch.ones((T, 1), dtype=torch.float64), sd_t], -1)
        if not per_guide:
            mu = torch.repeat_interleave(mu, data.target_lengths, dim=0)
            sd = torch.repeat_interleave(sd, data.target_lengths, dim=0)
        uq = data.upper_bounds[:, None, None].expand(-1, self.G, 2)
        lq = data.lower_bounds[:, None, None].expand(-1, self.G, 2)
        self.p_bin = elbo.std_normal_bin_prob(uq, lq, mu[None].expand(self.B, -1, -1), sd[None].expand(self.B, -1, -1))
        self.c_p = c_p.double()
        self.ctrl = data.allele_counts_control.double() if ctrl is None else ctrl.double()
        self.use_bcmatch, self.acc, self.lpn, self.mask_thres = use_bcmatch, scale_by_accessibility, lpn, mask_thres

    def __call__(self, u):
        data, R, B, G = self.data, self.R, self.B, self.G
        N = u.shape[0]
        u = u.reshape(N * R, 1, G)
        pi = torch.stack([torch.sigmoid(-u), torch.sigmoid(u)], -1)                      # (N R, 1, G, 2)
        h = tdist.Dirichlet(self.c_p[None, None].expand(N * R, 1, -1, -1), validate_args=False).log_prob(pi)
        h = h + pi.log().sum(-1)                                                          # the Jacobian of u
        h = h.reshape(N * R, G)
        h = h + tdist.Multinomial(probs=pi, validate_args=False).log_prob(self.ctrl.repeat(N, 1, 1, 1)).sum(1)
        pi_eff = pi
        if self.acc:
            pi_eff = elbo.scale_pi_by_accessibility(pi, data.guide_accessibility, self.lpn.double())
        egp = (pi_eff.expand(N * R, B, -1, -1) * self.p_bin[None]).sum(-1)                # (N R, B, G)
        liks = [(data.X_masked, data.size_factor, data.a0)]
        if self.use_bcmatch:
            liks.append((data.X_bcmatch_masked, data.size_factor_bcmatch, data.a0_bcmatch))
        for x, sf, a0 in liks:
            a = elbo.dirmult_concentration(egp, sf.repeat(N, 1), data.sample_mask.repeat(N, 1), a0)
            obs = x.permute(0, 2, 1).repeat(N, 1, 1)
            ll = elbo.dirichlet_multinomial_log_prob(a, obs)
            h = h + torch.where(obs.sum(-1) > self.mask_thres, ll, ll.new_zeros(()))
        return h.reshape(N, R, G)


def mode_centred_rule(h, a_prime, Q, newton=True):
    """log int exp(h(u)) du per pair (R, G) by Q-node Gauss-Hermite centred at the mode of h and scaled by its curvature
    there: from the Beta factor's centre u0 = log(a1'/a0') and scale s = sqrt(1/a0' + 1/a1'), NEWTON_STEPS Newton steps
    with gradient and curvature from central differences at +- FD_STEP s (a gradient step of length g s^2 where the
    second difference is not negative), each clamped to +- STEP_CAP s; the curvature at the end point gives sigma, and
    where it is not negative the Beta centre and scale are kept.  ``newton=False``: the Beta centre and scale as they
    are."""
    x, lw = gauss_hermite(Q)
    a0, a1 = a_prime[..., 0], a_prime[..., 1]
    u0 = (a1 / a0).log()
    s = (1.0 / a0 + 1.0 / a1).sqrt()
    m, sig = u0, s
    if newton:
        d = FD_STEP * s

        def diffs(m):
            hm, h0, hp = h(torch.stack([m - d, m, m + d]))
            return (hp - hm) / (2.0 * d), (hp - 2.0 * h0 + hm) / (d * d)

        for _ in range(NEWTON_STEPS):
            g, H = diffs(m)
            step = torch.where(H < 0, -g / H, g * s * s)
            m = m + torch.minimum(torch.maximum(step, -STEP_CAP * s), STEP_CAP * s)
        _, H = diffs(m)
        ok = H < 0
        m = torch.where(ok, m, u0)
        sig = torch.where(ok, 1.0 / (-H).clamp(min=1e-300).sqrt(), s)
    scale = math.sqrt(2.0) * sig
    vals = h(m[None] + scale[None] * x[:, None, None]) + lw[:, None, None]
    return scale.log() + torch.logsumexp(vals, 0)


def dense_rule(h, a_prime, n_points=20001, half_width=40.0, chunk=2001):
    """The independent reference: composite Simpson on ``n_points`` points over u0 +- half_width s, combined in logs."""
    assert n_points % 2 == 1
    a0, a1 = a_prime[..., 0], a_prime[..., 1]
    u0 = (a1 / a0).log()
    s = (1.0 / a0 + 1.0 / a1).sqrt()
    step = 2.0 * half_width * s / (n_points - 1)
    parts = []
    for i0 in range(0, n_points, chunk):
        i = torch.arange(i0, min(i0 + chunk, n_points), dtype=torch.float64)
        w = torch.where(i.long() % 2 == 1, 4.0, 2.0)
        w = torch.where((i == 0) | (i == n_points - 1), torch.ones_like(w), w)
        u = u0[None] + (i[:, None, None] - (n_points - 1) / 2) * step[None]
        parts.append(torch.logsumexp(h(u) + w.log()[:, None, None], 0))
    return (step / 3.0).log() + torch.logsumexp(torch.stack(parts), 0)


def target_site_terms(params, mu_t, y_t, sd_scale=0.01, prior_params=None):
    """log p(mu_t) - log q(mu_t) + log p(sd_t) - log q(sd_t), (T,): the sites of the oracle's losses."""
    P = elbo.constrained({k: params[k].detach().cpu().double().reshape(-1, 1) for k in ("mu_loc", "mu_scale", "sd_loc",
                                                                                         "sd_scale")})
    T = P["mu_loc"].shape[0]
    mu_t, sd_t = mu_t.reshape(T, 1), y_t.reshape(T, 1).exp()
    p_mu, p_sd = elbo._priors((T, 1), sd_scale, prior_params)
    lp = p_mu.log_prob(mu_t) + p_sd.log_prob(sd_t)
    lq = tdist.Normal(P["mu_loc"], P["mu_scale"]).log_prob(mu_t) + tdist.LogNormal(P["sd_loc"], P["sd_scale"]).log_prob(sd_t)
    return (lp - lq).reshape(T)


def marginal_log_weights(data, params, mu_t, y_t, Q, use_bcmatch=True, scale_by_accessibility=False, fit_noise=True,
                         eps_noise=None, sd_scale=0.01, prior_params=None, with_target_sites=True):
    """logw_marg (T,) and its pair terms (R, G) of ONE draw (mu_t, y_t = log sd_t, eps_noise) by the Q-node rule, with
    the summed magnitudes of the terms (T,) and of each pair's (R, G) for the tolerance of a comparison.  The pair terms
    are the library's: the constants plus the log of the integral WITHOUT the normaliser of Dirichlet(c_p), which the
    target sum adds once per pair under the repguide mask."""
    data64 = elbo.as_float64(data)
    T, G = data.n_targets, data.n_guides
    c_p = model_conc(data, params)
    lpn = None
    per_guide = torch.zeros(G, dtype=torch.float64)
    if scale_by_accessibility:
        eps = torch.as_tensor(eps_noise, dtype=torch.float64).reshape(G)
        if fit_noise:
            loc = params["noise_loc"].detach().cpu().double().reshape(G)
            sc = params["noise_scale"].detach().cpu().double().reshape(G).exp()
        else:
            # (the oracle's q_noise: Normal(zeros, full(0.655)) in float32 tensors)
            loc, sc = torch.zeros(G, dtype=torch.float64), torch.full((G,), elbo.PI_NOISE_SD).double()
        lpn = loc + eps * sc
        per_guide = tdist.Normal(0.0, elbo.PI_NOISE_SD).log_prob(lpn).double() - tdist.Normal(loc, sc).log_prob(lpn)
    h = PairIntegrand(data64, mu_t, y_t.exp(), c_p, use_bcmatch, scale_by_accessibility, lpn)
    rg = data.repguide_mask
    full = mode_centred_rule(h, beta_exponents(data64, c_p), Q)
    lognorm = torch.lgamma(c_p.sum(-1)) - torch.lgamma(c_p).sum(-1)                      # (G,)
    zero = torch.zeros_like(full)
    pairs = torch.where(rg, full - lognorm[None], zero)
    norm = torch.where(rg, lognorm[None].expand_as(full), zero)
    pair_mag = pairs.abs() + norm.abs()
    g2t = torch.repeat_interleave(torch.arange(T), data.target_lengths)
    tot = torch.zeros(T, dtype=torch.float64).index_add_(0, g2t, (pairs + norm).sum(0) + per_guide)
    mag = torch.zeros(T, dtype=torch.float64).index_add_(0, g2t, pair_mag.sum(0) + per_guide.abs())
    if with_target_sites:
        site = target_site_terms(params, mu_t, y_t, sd_scale, prior_params)
        tot, mag = tot + site, mag + site.abs()
    return tot, pairs, mag, pair_mag


def n_unresolved(data, params):
    """(T,) int: the pairs of a target that are under the repguide mask and fail the predicate."""
    c_p = model_conc(data, params)
    bad = (~resolved(elbo.as_float64(data), c_p)) & data.repguide_mask
    g2t = torch.repeat_interleave(torch.arange(data.n_targets), data.target_lengths)
    return torch.zeros(data.n_targets, dtype=torch.int64).index_add_(0, g2t, bad.sum(0))


# ------------------------------------------------------------------ the exact posterior of one target, pi integrated out
def tile_guides(data, K):
    """The fields PairIntegrand reads, the guides of ``data`` laid out K times (copy k: guides k G .. (k + 1) G - 1)."""
    import types

    data = elbo.as_float64(data)
    out = types.SimpleNamespace(n_reps=data.n_reps, n_condits=data.n_condits, n_guides=K * data.n_guides,
                                upper_bounds=data.upper_bounds, lower_bounds=data.lower_bounds,
                                size_factor=data.size_factor, size_factor_bcmatch=data.size_factor_bcmatch,
                                sample_mask=data.sample_mask)
    out.X_masked = data.X_masked.repeat(1, 1, K)
    out.X_bcmatch_masked = data.X_bcmatch_masked.repeat(1, 1, K)
    out.a0, out.a0_bcmatch = data.a0.repeat(K), data.a0_bcmatch.repeat(K)
    out.allele_counts_control = data.allele_counts_control.repeat(1, 1, K, 1)
    out.repguide_mask = data.repguide_mask.repeat(1, K)
    return out


def marginal_log_joint(sub, c_p, mu, y, Q=64, use_bcmatch=True, sd_scale=0.01):
    """``log p(x, mu, sd)``, pi integrated out by the Q-node rule, of the ONE-target screen ``sub`` at K points
    (mu[k], sd = exp(y[k])), as a density in (mu, y = log sd): the Jacobian sd of y is included."""
    assert sub.n_targets == 1
    K, G = mu.numel(), sub.n_guides
    tiled = tile_guides(sub, K)
    cp = c_p.repeat(K, 1)
    h = PairIntegrand(tiled, mu.repeat_interleave(G), y.exp().repeat_interleave(G), cp, use_bcmatch, per_guide=True)
    pairs = mode_centred_rule(h, beta_exponents(tiled, cp), Q)
    pairs = torch.where(tiled.repguide_mask, pairs, torch.zeros_like(pairs))
    p_mu, p_sd = elbo._priors((K,), sd_scale, None)
    return pairs.reshape(sub.n_reps, K, G).sum((0, 2)) + p_mu.log_prob(mu) + p_sd.log_prob(y.exp()) + y


def exact_marginal_moments(sub, c_p, n_mu=61, n_y=31, width=6.5, use_bcmatch=True):
    """``E[mu | x]``, ``sd[mu | x]`` of the one-target screen by 2-D quadrature of ``marginal_log_joint`` over (mu, log sd)
    on an n_mu x n_y grid of +- ``width`` posterior sds, the same moments from every second grid line (the step
    doubled), and the largest density on the grid's border relative to the peak."""
    def moments(lj, x):
        w = torch.softmax(lj, 0)
        m = float((w * x).sum())
        return m, float((w * (x - m) ** 2).sum().sqrt())

    lj1 = lambda m, y: marginal_log_joint(sub, c_p, m, y, use_bcmatch=use_bcmatch)  # noqa: E731
    coarse = torch.linspace(-5.0, 5.0, 401, dtype=torch.float64)
    m0, _ = moments(lj1(coarse, torch.zeros_like(coarse)), coarse)
    yc = torch.linspace(-0.5, 0.5, 401, dtype=torch.float64)
    y0, sy = moments(lj1(torch.full_like(yc, m0), yc), yc)
    fine = torch.linspace(m0 - 1.0, m0 + 1.0, 401, dtype=torch.float64)
    m0, s0 = moments(lj1(fine, torch.full_like(fine, y0)), fine)
    s0, sy = max(s0, 1e-3), max(sy, 1e-3)
    mus = torch.linspace(m0 - width * s0, m0 + width * s0, n_mu, dtype=torch.float64)
    ys = torch.linspace(y0 - width * sy, y0 + width * sy, n_y, dtype=torch.float64)
    MU, Y = torch.meshgrid(mus, ys, indexing="ij")
    lj = lj1(MU.reshape(-1), Y.reshape(-1)).reshape(n_mu, n_y)
    dens = (lj - lj.max()).exp()
    border = torch.cat([dens[0], dens[-1], dens[:, 0], dens[:, -1]]).max()

    def grid_moments(d, M):
        w = d / d.sum()
        mean = float((w * M).sum())
        return mean, math.sqrt(float((w * (M - mean) ** 2).sum()))

    mean, sd = grid_moments(dens, MU)
    mean2, sd2 = grid_moments(dens[::2, ::2], MU[::2, ::2])
    return {"mean": mean, "sd": sd, "mean_coarse": mean2, "sd_coarse": sd2, "border": float(border), "y_mean": y0, "y_sd": sy}


# ------------------------------------------------------------------ the claim test: guide, exact moments, assertion
# q(mu_t) = N(0, 0.2), q(log sd_t) = N(0, 0.04) on importance_common.claim_screen(), MixtureNormal, alpha_pi at its initial
# value.  With pi integrated out the posterior of a null target there has sd[mu | x] 0.05 - 0.08 around means of -0.11 ...
# 0.14 (a tenth to a quarter of a guide's cells are edited: less is known about mu than in the Normal family) and
# log sd 0.03 +- 0.01: covered two and a half times and four times over
CLAIM_MU_SCALE, CLAIM_SD_SCALE = 0.2, 0.04
_exact = {}


def claim_params(data):
    T = data.n_targets
    return {"mu_loc": torch.zeros(T, 1), "mu_scale": torch.full((T, 1), math.log(CLAIM_MU_SCALE)),
            "sd_loc": torch.zeros(T, 1), "sd_scale": torch.full((T, 1), math.log(CLAIM_SD_SCALE))}


def claim_exact(data, t):
    """exact_marginal_moments of target t of the claim screen; computed once per process."""
    if t not in _exact:
        idx = list(range(int(data.target_offsets[t]), int(data.target_offsets[t + 1])))
        c_p = model_conc(data, elbo.init_params("MixtureNormal", data))
        _exact[t] = exact_marginal_moments(elbo.as_float64(data[idx]), c_p[idx])
    return _exact[t]


def assert_marginal_claim(summary, data, targets, what):
    """On ``targets``: wherever psis_k_marg < 0.7, |mu_is_marg - E[mu | x]| <= 4 sd[mu | x] / sqrt(is_ess_marg), on at
    least two (the form of importance_common.assert_claim).  The exact moments must come from a grid whose border
    density is below 1e-6 of the peak and whose mean moves by less than a tenth of the cap when the step is doubled."""
    ok = 0
    for t in targets:
        ex = claim_exact(data, t)
        assert ex["border"] < 1e-6, (t, ex["border"])
        k, ess = float(summary["psis_k_marg"][t]), float(summary["is_ess_marg"][t])
        got, got_sd = float(summary["mu_is_marg"][t]), float(summary["mu_sd_is_marg"][t])
        cap = 4.0 * ex["sd"] / math.sqrt(ess)
        print(f"{what} target {t}: psis_k_marg {k:.3f} is_ess_marg {ess:.1f} mu_is_marg {got:.5f} exact {ex['mean']:.5f} "
              f"|diff| {abs(got - ex['mean']):.5f} cap {cap:.5f}; mu_sd_is_marg {got_sd:.5f} exact sd {ex['sd']:.5f}; "
              f"border {ex['border']:.2e}; step doubled: mean moves {abs(ex['mean'] - ex['mean_coarse']):.2e}")
        assert abs(ex["mean"] - ex["mean_coarse"]) < 0.1 * cap, (t, ex, cap)
        if k < 0.7:
            ok += 1
            assert abs(got - ex["mean"]) <= cap, (t, got, ex["mean"], cap)
    assert ok >= 2, ok
