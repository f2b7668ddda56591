"""What the importance-sampling tests share (test_importance_cpu.py, test_gpu_importance.py): cutting a screen, its
parameters and its noise down to one target for the oracle, the one-target log joint of the Normal family built from the
oracle's own functions, its exact posterior moments by 2-D quadrature, and the hand-set guide of the claim test.  A plain
module imported by bare name."""
import math

import torch

from oracle import elbo

PER_TARGET = ("mu_loc", "mu_scale", "sd_loc", "sd_scale")
PER_GUIDE = ("alpha_pi", "noise_loc", "noise_scale")

# ---- the claim test (section "the check does what it claims"): screen, guide and draws
CLAIM_GUIDES, CLAIM_REPS, CLAIM_SEED = 40, 3, 3
# q(mu_t) = N(0, 0.06), q(log sd_t) = N(0, 0.04).  The posterior of a null target of this screen (15 pairs of ~2 500
# reads, two likelihoods) has sd[mu | x] ~ 0.015 and log sd ~ 0.04 +- 0.01: four times covered in both directions
CLAIM_MU_SCALE, CLAIM_SD_SCALE = 0.06, 0.04
CLAIM_TARGETS = (3, 5, 7)  # null targets (target 0 carries an effect: mu_loc = 0 does not cover it)
CLAIM_DRAWS = 4096


def target_guides(data, t):
    off = data.target_offsets
    return list(range(int(off[t]), int(off[t + 1])))


def cut_params(params, t, idx):
    """The (float64, CPU) parameters of target t and its guides, shaped as the oracle takes them for a one-target screen."""
    out = {}
    for k, v in params.items():
        v = v.detach().cpu().double()
        out[k] = v[t:t + 1] if k in PER_TARGET else v[idx]
    return out


def cut_noise(noise, t, idx):
    out = {}
    for k, v in noise.items():
        v = torch.as_tensor(v).detach().cpu().double()
        if k in ("eps_mu", "eps_sd"):
            out[k] = v.reshape(-1, 1)[t:t + 1]
        elif k == "pi":
            out[k] = v[:, :, idx, :]
        elif k == "eps_noise":
            out[k] = v.reshape(-1)[idx]
    return out


def cut_kw(kw, t):
    kw = dict(kw)
    if kw.get("prior_params") is not None:
        # (float64 mode: as_float64 promotes the screen, not the priors - left in float32, torch forms log(scale) and
        # scale**2 of the prior in float32, 2e-5 of a target's terms; the engine takes the same values as float64)
        kw["prior_params"] = {k: torch.as_tensor(v)[t:t + 1].double() for k, v in kw["prior_params"].items()}
    return kw


def oracle_logw(family, data, params, noise, t, kw):
    """``log p - log q`` of target t alone by the oracle, float64 mode, and the sum of its site terms' magnitudes."""
    idx = target_guides(data, t)
    rec = {}
    loss = elbo.LOSSES[family](elbo.as_float64(data[idx]), cut_params(params, t, idx), noise=cut_noise(noise, t, idx),
                               record=rec, **cut_kw(kw, t))
    mag = sum(abs(v) for v in rec["model"].values()) + sum(abs(v) for v in rec["guide"].values())
    return -float(loss), mag


# ------------------------------------------------------------------ the Normal family's one-target log joint
def normal_log_joint(sub, mu, y, sd_scale=0.01, use_bcmatch=True):
    """``log p(x, mu, sd)`` of the ONE-target Normal-family screen ``sub`` (float64) at N points (mu[n], sd = exp(y[n])):
    the sites of ``oracle.elbo.normal_loss`` evaluated with the oracle's own functions, the N points laid out as N
    copies of the target's guides."""
    assert sub.n_targets == 1
    N = mu.numel()
    R, B, G = sub.n_reps, sub.n_condits, sub.n_guides
    sd = y.exp()
    p_mu, p_sd = elbo._priors((N,), sd_scale, None)
    lp = p_mu.log_prob(mu) + p_sd.log_prob(sd)
    uq = sub.upper_bounds.reshape(1, B)
    lq = sub.lower_bounds.reshape(1, B)
    p = elbo.std_normal_bin_prob(uq.expand(N, B), lq.expand(N, B), mu.reshape(N, 1).expand(N, B),
                                 sd.sqrt().reshape(N, 1).expand(N, B))                      # (N, B)
    egp = p.t().reshape(1, B, N, 1).expand(R, B, N, G).reshape(R, B, N * G)
    liks = [(sub.X_masked, sub.size_factor, sub.a0)]
    if use_bcmatch:
        liks.append((sub.X_bcmatch_masked, sub.size_factor_bcmatch, sub.a0_bcmatch))
    for x, sf, a0 in liks:
        a = elbo.dirmult_concentration(egp, sf, sub.sample_mask, a0.repeat(N))
        obs = x.permute(0, 2, 1).repeat(1, N, 1)
        m = torch.logical_and(obs.sum(-1) > 10, sub.repguide_mask.repeat(1, N))
        ll = elbo.dirichlet_multinomial_log_prob(a, obs)
        lp = lp + torch.where(m, ll, ll.new_zeros(())).reshape(R, N, G).sum((0, 2))
    return lp


def exact_moments(sub, n_mu=241, n_y=121, use_bcmatch=True):
    """``E[mu | x]``, ``sd[mu | x]`` of the one-target screen by 2-D quadrature of ``normal_log_joint`` over (mu, log sd),
    and the largest density on the grid's border relative to the peak."""
    def moments(lj, x):
        w = torch.softmax(lj, 0)
        m = float((w * x).sum())
        return m, float((w * (x - m) ** 2).sum().sqrt())

    # where the mass is: mu along log sd = 0, log sd along that mu, mu again along that log sd - then +-8 sd around it
    coarse = torch.linspace(-5.0, 5.0, 2001, dtype=torch.float64)
    m0, _ = moments(normal_log_joint(sub, coarse, torch.zeros_like(coarse), use_bcmatch=use_bcmatch), coarse)
    yc = torch.linspace(-0.5, 0.5, 2001, dtype=torch.float64)
    y0, sy = moments(normal_log_joint(sub, torch.full_like(yc, m0), yc, use_bcmatch=use_bcmatch), yc)
    fine = torch.linspace(m0 - 0.5, m0 + 0.5, 2001, dtype=torch.float64)
    m0, s0 = moments(normal_log_joint(sub, fine, torch.full_like(fine, y0), use_bcmatch=use_bcmatch), fine)
    s0, sy = max(s0, 1e-3), max(sy, 1e-3)
    mus = torch.linspace(m0 - 8 * s0, m0 + 8 * s0, n_mu, dtype=torch.float64)
    ys = torch.linspace(y0 - 8 * sy, y0 + 8 * sy, n_y, dtype=torch.float64)
    MU, Y = torch.meshgrid(mus, ys, indexing="ij")
    lj = normal_log_joint(sub, MU.reshape(-1), Y.reshape(-1), use_bcmatch=use_bcmatch).reshape(n_mu, n_y)
    lj = lj - lj.max()
    dens = lj.exp()
    border = torch.cat([dens[0], dens[-1], dens[:, 0], dens[:, -1]]).max()
    w = dens / dens.sum()
    mean = float((w * MU).sum())
    sd = math.sqrt(float((w * (MU - mean) ** 2).sum()))
    return mean, sd, float(border)


def claim_screen():
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    return make_sorting_variant_screen(CLAIM_GUIDES, CLAIM_REPS, seed=CLAIM_SEED)


def claim_params(data):
    """The hand-set guide: mu_loc = 0 and scales wide enough to cover the posterior (unconstrained, float32)."""
    T = data.n_targets
    return {"mu_loc": torch.zeros(T, 1), "mu_scale": torch.full((T, 1), math.log(CLAIM_MU_SCALE)),
            "sd_loc": torch.zeros(T, 1), "sd_scale": torch.full((T, 1), math.log(CLAIM_SD_SCALE))}


def assert_claim(summary, data, what):
    """The claim on the CLAIM_TARGETS: |mu_is - E| <= 4 sd / sqrt(is_ess) wherever psis_k < 0.7, on at least two."""
    ok = 0
    for t in CLAIM_TARGETS:
        sub = elbo.as_float64(data[target_guides(data, t)])
        mean, sd, border = exact_moments(sub)
        assert border < 1e-6, (t, border)
        k, ess = float(summary["psis_k"][t]), float(summary["is_ess"][t])
        got, got_sd = float(summary["mu_is"][t]), float(summary["mu_sd_is"][t])
        cap = 4.0 * sd / math.sqrt(ess)
        print(f"{what} target {t}: psis_k {k:.3f} is_ess {ess:.1f} mu_is {got:.5f} exact {mean:.5f} "
              f"|diff| {abs(got - mean):.5f} cap {cap:.5f}; mu_sd_is {got_sd:.5f} exact sd {sd:.5f}; border {border:.2e}")
        if k < 0.7:
            ok += 1
            assert abs(got - mean) <= cap, (t, got, mean, cap)
    assert ok >= 2, ok
