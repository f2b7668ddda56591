"""The Normal side of the oracle-parity tests moved off ``init + 0.3 randn``: strong effects, narrow and wide target
scales, variational scales a converged fit has, and count precisions small enough for a bin's concentration to sit on
its floor because of its PROBABILITY (test_effect_regimes.py on the host, test_gpu_effect_regimes.py on the device).  A
plain module imported by bare name; nothing here is code under test and nothing here looks at a device.

``with_small_a0(data)`` is a copy of a screen whose ``a0`` / ``a0_bcmatch`` follow ``A0_PATTERN`` guide by guide; every
other attribute is the object ``data`` holds.  ``get_alpha`` forms ``(p sf + eps / B) / (S + eps) a0`` and floors it at
``eps = 1e-5``: with ``p = 0`` that is ``a0 eps / (B (S + eps))``, and with the size factors and bin probabilities the
screens have (``S + eps`` near 1, B = 5) it is above the floor for every ``a0 >= 5.1``: the generated screens
(``a0 >= 11``) never reach a floor through a probability, only through ``sample_mask``.  The pattern holds guides on
both sides of 5, and 4.9 | 5.1 straddle that point.

``effect_point(kind, data, start, seed)`` replaces, in the float32 unconstrained parameters ``start``: ``mu_loc`` by
``MU`` cycled over the targets (edits), ``sd_loc`` by the log of ``SD`` cycled, both log-scales by draws from
``LOG_SCALES`` per target, ``alpha_pi`` by ``grad_bounds.fitted_like_alpha_pi``.  With the bin edges at the normal
quantiles of 0.2 ... 0.8 (|z| <= 0.85) the mixture families reach ``|u| = |z - mu| / sd`` of 97 at (mu, sd) = (4,
0.05), the Normal family (scale ``exp(y / 2)``) 22.

The survival kinds have no ``sd``; their ``mu_loc`` is ``MU`` times ``SURVIVAL_MU_MAX / 4``, that is the symmetric range
+-``SURVIVAL_MU_MAX`` = +-256.  The range was chosen on the host over the ladder 4, 8, 16, ... as the widest at which the
survival oracles' loss and every gradient are finite on the time points of ``survival_130x2`` (0, 0.2, ..., 1) and
``survival_tiling_70x2`` (0, 0.5, 1) of test_gpu_grad_elementwise.py and no ``tol_k`` is zero where the reference is
not; test_effect_regimes.py repeats the check at the chosen range and shows that the next rung, 512, fails it (the
tiling oracle's loss is NaN there: the growth term is ``exp(mu t)`` with ``t`` in [0, 1], a tiling allele adds up its
edits, and ``exp`` of three times 512 is not a float64).  Floors by probability begin at a range of 16 (variant) and 8
(tiling); at 256, 93 of 260 and 122 of 140 pairs hold one.

``near_one_pi(shape, seed)``: Dirichlet draws to hand in, a third of the (replicate, guide) pairs with ``pi_0`` in
[1e-12, 1e-6] (log-uniform) - the edited component alone decides the concentration, and bins floor as in the Normal
family - the rest with ``pi_0`` in [0.05, 0.95].

``floor_census`` counts, from the oracle's own ``std_normal_bin_prob`` and ``dirmult_concentration`` as the family's
loss calls them, what the point reaches; ``exact_alpha`` is the 50-digit evaluation of the concentrations together with
the error budget of a float64 evaluation (section 5 of DESIGN.md).

``CASES`` are the evaluations both test files make: name: (kind, generator arguments, model arguments, family,
whether ``near_one_pi`` is handed in, and whether the census must show the regime - the Normal family and the mixture
with ``near_one_pi``; elsewhere the wild-type component or the accessibility clamp of 1e-3 keeps every bin up).
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

import grad_bounds as gb
from oracle import elbo
from oracle import survival as osurv

A0_PATTERN = (0.5, 1.0, 2.0, 4.0, 4.9, 5.1, 20.0, 300.0)
MU = (-4.0, -3.0, -2.0, -1.0, -0.3, 0.0, 0.3, 1.0, 2.0, 3.0, 4.0)
SD = (0.05, 0.2, 0.5, 1.0, 2.0)
LOG_SCALES = (-3.0, -4.0, -5.0)
SURVIVAL_MU_MAX = 256.0
EPS = elbo.EPS
WAVE = 64
MASK_THRES = 10

VARIANT = dict(n_guides=130, n_reps=2, guides_per_target=3, seed=31)
CASES = {
    "variant_130x2": ("variant", dict(VARIANT), {}, "Normal", False, True),
    "variant_130x2_nobc": ("variant", dict(VARIANT), dict(use_bcmatch=False), "Normal", False, True),
    "variant_130x2_near_one_pi": ("variant", dict(VARIANT), {}, "MixtureNormal", True, True),
    "variant_130x2_acc": ("variant", dict(VARIANT, with_accessibility=True), dict(scale_by_accessibility=True),
                          "MixtureNormal", False, False),
    "variant_257x3_long_targets": ("variant", dict(n_guides=257, n_reps=3, guides_per_target=100, seed=33), {}, "Normal",
                                   False, True),
    "tiling_130x2_a5": ("tiling", dict(n_guides=130, n_reps=2, n_max_alleles=5, seed=4, depth_per_guide=30.0), {},
                        "MultiMixtureNormal", False, False),
    "tiling_70x2_a48": ("tiling", dict(n_guides=70, n_reps=2, n_max_alleles=48, seed=14), {}, "MultiMixtureNormal", False,
                        False),
    "survival_130x2": ("survival", dict(n_guides=130, n_reps=2, seed=4), {}, "MixtureNormal", False, False),
    "survival_tiling_70x2": ("survival_tiling", dict(n_guides=70, n_reps=2, n_max_alleles=5, seed=5, depth_per_guide=30.0),
                             {}, "MultiMixtureNormal", False, False),
}
PI_SEED = 7
# the steppers' screen: 65 targets of two guides (the fused steppers need 64 targets or more; fewer: k_param's
# one-block-per-target mode)
STEPPER_SCREEN = dict(n_guides=130, n_reps=2, guides_per_target=2, seed=31)


def with_small_a0(data):
    out = copy.copy(data)
    G = data.n_guides
    pat = torch.tensor(A0_PATTERN, dtype=torch.float64)[torch.arange(G) % len(A0_PATTERN)]
    out.a0 = pat.to(device=data.a0.device, dtype=data.a0.dtype)
    out.a0_bcmatch = pat.to(device=data.a0_bcmatch.device, dtype=data.a0_bcmatch.dtype)
    return out


def _cycled(values, shape, scale=1.0):
    n = int(np.prod(shape)) if len(shape) else 1
    v = torch.tensor(values, dtype=torch.float64)[torch.arange(n) % len(values)] * scale
    return v.reshape(shape).float()


def effect_point(kind, data, start, seed=7, mu_max=None):
    """``start``: the unconstrained parameters of any point (the engine's or ``init_params``' start values, perturbed or
    not); returns float32 tensors, the ones named in the module docstring replaced and the others as handed in.
    ``mu_max`` overrides the largest ``|mu_loc|`` (the survival range is found with it)."""
    rng = np.random.default_rng(seed)
    out = {k: v.detach().cpu().float().clone() for k, v in start.items()}
    shape = tuple(out["mu_loc"].shape)
    if mu_max is None:
        mu_max = SURVIVAL_MU_MAX if kind.startswith("survival") else max(MU)
    out["mu_loc"] = _cycled(MU, shape, mu_max / max(MU))
    if "sd_loc" in out:
        out["sd_loc"] = _cycled(SD, shape).log()
    for k in ("mu_scale", "sd_scale"):
        if k in out:
            pick = rng.integers(0, len(LOG_SCALES), size=max(1, int(np.prod(shape))))
            out[k] = torch.tensor(np.asarray(LOG_SCALES)[pick]).reshape(shape).float()
    if "alpha_pi" in out:
        out["alpha_pi"] = gb.fitted_like_alpha_pi(data, out["alpha_pi"], seed=seed)
    assert all(v.dtype == torch.float32 for v in out.values())
    return out


def near_one_pi(shape, seed=0):
    """(R, 1, G, A) float64 draws, rows summing to 1: pair ``i`` (replicates major) has ``pi_0`` log-uniform in [1e-12,
    1e-6] where ``i mod 3 == 0`` and uniform in [0.05, 0.95] elsewhere; the other alleles share the rest by uniform
    weights (with two alleles ``pi_1 = 1 - pi_0``)."""
    R, one, G, A = shape
    assert one == 1 and A >= 2
    rng = np.random.default_rng(seed)
    small = np.exp(rng.uniform(np.log(1e-12), np.log(1e-6), R * G))
    usual = rng.uniform(0.05, 0.95, R * G)
    pi0 = np.where(np.arange(R * G) % 3 == 0, small, usual).reshape(R, 1, G)
    w = rng.uniform(0.5, 1.5, (R, 1, G, A - 1))
    rest = (1.0 - pi0)[..., None] * w / w.sum(-1, keepdims=True)
    return torch.tensor(np.concatenate([pi0[..., None], rest], -1))


def loss_of(family, data):
    """The oracle loss of a family name on this kind of screen (a callable is returned as it is)."""
    if callable(family):
        return family
    mod = osurv if getattr(data, "timepoints", None) is not None else elbo
    return mod.LOSSES[family]


def _spied(data, params, noise, kw, family):
    """One evaluation of the family's oracle loss (float64) with its calls of ``std_normal_bin_prob`` and
    ``dirmult_concentration`` recorded: ([(probabilities, allele mask or None)], [(egp, size factors, mask, a0)])."""
    probs, concs = [], []

    def spy_p(orig):
        def f(uq, lq, mu, sd, mask=None):
            res = orig(uq, lq, mu, sd, mask=mask)
            probs.append((res.detach(), mask))
            return res
        return f

    def spy_c(orig):
        def f(egp, size_factor, sample_mask, a0, eps=EPS):
            concs.append((egp.detach(), size_factor, sample_mask, a0))
            return orig(egp, size_factor, sample_mask, a0, eps)
        return f

    p = {k: v.detach().double() for k, v in params.items()}
    with gb._Patched("std_normal_bin_prob", spy_p), gb._Patched("dirmult_concentration", spy_c), torch.no_grad():
        loss_of(family, data)(elbo.as_float64(data), p, noise=noise, **dict(kw or {}))
    return probs, concs


def raw_concentration(egp, size_factor, sample_mask, a0, eps=EPS):
    """``dirmult_concentration`` before its mask and floor: (R, G, B)."""
    p = egp.permute(0, 2, 1) * size_factor[:, None, :]
    return (p + eps / p.shape[-1]) / (p.sum(-1)[:, :, None] + eps) * a0[None, :, None]


def floor_census(data, params, noise, kw=None, family="Normal"):
    """What one evaluation at ``params`` / ``noise`` reaches, per count likelihood the family evaluates (X first).  A bin
    is floored by its probability where ``sample_mask == 1`` and the raw concentration is below 1e-5; a pair is a
    (replicate, guide) the likelihood's mask keeps (total above 10 and ``repguide_mask``); a lane holds a pair, a wave
    the 64 consecutive guides of one replicate, and a lane is floored where one of its bins is.

    Returns a dict: ``floored_bins``, ``kept_pairs``, ``floored_pairs`` (kept pairs with a floored bin), ``mixed_pairs``
    (kept pairs with floored AND unfloored bins), ``waves``, ``full_waves`` (64 guides), ``mixed_waves`` and
    ``mixed_full_waves`` (floored and unfloored kept lanes side by side), ``floored_lanes_per_wave`` (first likelihood,
    replicate 0) - each a list over the likelihoods but the last -, ``p_zero`` / ``p_one`` (bin probabilities of unmasked
    alleles that are exactly 0 / 1) and ``nearest``, the smallest ``|raw / 1e-5 - 1|`` over the unmasked bins of both
    likelihoods."""
    probs, concs = _spied(data, params, noise, kw, family)
    out = {k: [] for k in ("floored_bins", "kept_pairs", "floored_pairs", "mixed_pairs", "waves", "full_waves",
                           "mixed_waves", "mixed_full_waves")}
    p_zero = p_one = 0
    for res, mask in probs:
        live = torch.ones_like(res, dtype=torch.bool) if mask is None else mask.expand_as(res)
        p_zero += int(((res == 0.0) & live).sum())
        p_one += int(((res == 1.0) & live).sum())
    nearest = math.inf
    planes = (data.X_masked, data.X_bcmatch_masked)
    G = data.n_guides
    for i, (egp, sf, sm, a0) in enumerate(concs):
        raw = raw_concentration(egp, sf, sm, a0)                       # (R, G, B)
        on = (sm[:, None, :] == 1).expand_as(raw)
        floored = on & (raw < EPS)
        nearest = min(nearest, float((raw / EPS - 1.0).abs()[on].min()))
        kept = torch.logical_and(planes[i].permute(0, 2, 1).double().sum(-1) > MASK_THRES, data.repguide_mask)  # (R, G)
        lane = floored.any(-1) & kept
        clean = (on & ~floored).any(-1)
        out["floored_bins"].append(int((floored & kept[..., None]).sum()))
        out["kept_pairs"].append(int(kept.sum()))
        out["floored_pairs"].append(int(lane.sum()))
        out["mixed_pairs"].append(int((lane & clean).sum()))
        n_w = (G + WAVE - 1) // WAVE
        waves = full = mixed = mixed_full = 0
        per_wave = []
        for r in range(raw.shape[0]):
            for w in range(n_w):
                sl = slice(w * WAVE, min(G, (w + 1) * WAVE))
                k, f = kept[r, sl], lane[r, sl]
                is_full = sl.stop - sl.start == WAVE
                is_mixed = bool(f.any()) and bool((k & ~f).any())
                waves, full = waves + 1, full + int(is_full)
                mixed, mixed_full = mixed + int(is_mixed), mixed_full + int(is_mixed and is_full)
                if r == 0:
                    per_wave.append(int(f.sum()))
        for k, v in (("waves", waves), ("full_waves", full), ("mixed_waves", mixed), ("mixed_full_waves", mixed_full)):
            out[k].append(v)
        if i == 0:
            out["floored_lanes_per_wave"] = per_wave
    out.update(p_zero=p_zero, p_one=p_one, nearest=nearest)
    return out


def census_line(c):
    return (f"floored bins {c['floored_bins']}, pairs with one {c['floored_pairs']} of {c['kept_pairs']} kept "
            f"({c['mixed_pairs']} hold unfloored bins too), waves mixing floored and unfloored lanes {c['mixed_waves']} of "
            f"{c['waves']} (full: {c['mixed_full_waves']} of {c['full_waves']}), floored lanes per wave of replicate 0 "
            f"{c['floored_lanes_per_wave']}, P == 0: {c['p_zero']}, P == 1: {c['p_one']}, nearest |raw / 1e-5 - 1| "
            f"{c['nearest']:.3e}")


def assert_reaches_the_regime(c, what):
    """The conditions of the regime on a census: a tenth of the kept pairs hold a floored bin, every full wave mixes
    floored and unfloored lanes, some probability is exactly 0, and no raw concentration is within 1e-6 (relative) of
    the floor - the device and the oracle then take the same side at every bin."""
    for i in range(len(c["kept_pairs"])):
        assert c["floored_pairs"][i] >= 0.1 * c["kept_pairs"][i], (what, i, c["floored_pairs"], c["kept_pairs"])
        assert c["full_waves"][i] > 0 and c["mixed_full_waves"][i] == c["full_waves"][i], (what, i, c)
    assert c["p_zero"] > 0, (what, c["p_zero"])
    assert c["nearest"] >= 1e-6, (what, c["nearest"])


# ---------------------------------------------------------------- the concentrations in exact arithmetic
# The error budget of a float64 evaluation of alpha, in units of 2^-53:
U53 = 2.0 ** -53
C_PHI = 4.0      # absolute, per edge: 0.5 (1 + erf(u / sqrt 2)) or 0.5 erfc(-u / sqrt 2) - a few roundings of a value <= 1
C_U = 4.0        # relative rounding of u = (z - mu) / sd: exp for sd, the difference, the quotient, the 1 / sqrt 2
C_W_ACC = 16.0   # absolute, per component weight formed by scale_pi_by_accessibility (pow, logit, exp, quotient, 1 - p)
C_FORM = 8.0     # relative, on alpha itself: the products, the sum over B bins, the quotient
# The multiple of that budget torch's float64 evaluation - the reference's own arithmetic, and the oracle's - needs against
# the 50-digit values over the cases of test_effect_regimes.py (measured there and asserted: 0.177, 0.183 and 0.047, rounded
# up); the device, which differs from torch in its erf and in the order of a few additions, is held to DEVICE_MARGIN times
# that, the margin the implicit-gradient fixture gave the device over torch (tests/dirichlet_grad_reference.py)
K_HOST = 0.2
DEVICE_MARGIN = 4.0


def site_values(family, data, params, acc_noise=None):
    """The float64 values the concentrations are a function of when every site sits at its location (eps = 0): per guide
    and component the mean and scale, (G, C) arrays; ``z_hi`` / ``z_lo`` (B,) with +-inf at the outer edges; and for
    the +Acc model ``kacc`` (G,) and the logit noise (G,)."""
    T = data.n_targets
    tl = data.target_lengths.cpu()
    mu_t = params["mu_loc"].detach().cpu().double().reshape(T)
    y_t = params["sd_loc"].detach().cpu().double().reshape(T)
    mu_g = torch.repeat_interleave(mu_t, tl).numpy()
    y_g = torch.repeat_interleave(y_t, tl).numpy()
    std = torch.distributions.Normal(0.0, 1.0)
    uq, lq = data.upper_bounds.cpu().double(), data.lower_bounds.cpu().double()
    half = torch.full_like(uq, 0.5)
    z_hi = torch.where(uq == 1.0, torch.full_like(uq, math.inf), std.icdf(torch.where(uq == 1.0, half, uq))).numpy()
    z_lo = torch.where(lq == 0.0, torch.full_like(lq, -math.inf), std.icdf(torch.where(lq == 0.0, half, lq))).numpy()
    out = dict(mu_g=mu_g, y_g=y_g, z_hi=z_hi, z_lo=z_lo, mixture=family != "Normal")
    if acc_noise is not None:
        kacc = torch.exp(torch.tensor(elbo.ACC_B)) * torch.pow(data.guide_accessibility.cpu(), elbo.ACC_A)
        out["kacc"] = kacc.double().numpy()
        out["lpn"] = acc_noise.detach().cpu().double().numpy()
    return out


def exact_alpha(family, data, params, pi=None, acc_noise=None, use_bcmatch=True, digits=50):
    """``get_alpha`` composed with ``std_normal_bin_prob`` in ``digits``-digit arithmetic (mpmath) from the float64 inputs
    ``site_values`` names and, for the mixture family, the draws ``pi`` (R, 1, G, 2).  Returns ``(alpha, budget,
    floored)``: (L, R, B, G) float64 arrays shaped like the device's ``alpha`` plane - the floored concentration
    rounded to float64, the error budget of a float64 evaluation of it (``U53`` times the constants above, carried
    through the formula) and whether the element sits on the floor."""
    import mpmath as mp

    s = site_values(family, data, params, acc_noise)
    R, B, G = data.n_reps, data.n_condits, data.n_guides
    sm = data.sample_mask.cpu().numpy()
    liks = [(data.size_factor, data.a0)] + ([(data.size_factor_bcmatch, data.a0_bcmatch)] if use_bcmatch else [])
    alpha = np.zeros((len(liks), R, B, G))
    budget = np.zeros_like(alpha)
    floored = np.zeros(alpha.shape, dtype=bool)
    with mp.workdps(digits):
        half, rt2, eps = mp.mpf(0.5), mp.sqrt(2), mp.mpf(EPS)

        def phi(u):
            return half * mp.erfc(-u / rt2)

        def pdf(u):
            return mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi)

        def bin_probs(mu, sd):
            P, dP = [], []
            for b in range(B):
                val, err = mp.mpf(0), mp.mpf(0)
                for z, sign in ((s["z_hi"][b], 1), (s["z_lo"][b], -1)):
                    if math.isinf(z):
                        val += sign * (1 if z > 0 else 0)
                        continue
                    u = (mp.mpf(float(z)) - mu) / sd
                    val += sign * phi(u)
                    err += (C_PHI + C_U * abs(u) * pdf(u)) * U53
                P.append(val)
                dP.append(err)
            return P, dP

        for g in range(G):
            mu1, y1 = mp.mpf(float(s["mu_g"][g])), mp.mpf(float(s["y_g"][g]))
            if s["mixture"]:
                comp = [bin_probs(mp.mpf(0), mp.mpf(1)), bin_probs(mu1, mp.exp(y1))]
            else:
                comp = [bin_probs(mu1, mp.exp(y1 / 2))]                    # NormalModel: scale sqrt(sd_t)
            for r in range(R):
                dw = mp.mpf(0)
                if not s["mixture"]:
                    w = [mp.mpf(1)]
                else:
                    w = [mp.mpf(float(pi[r, 0, g, a])) for a in range(2)]
                    if acc_noise is not None:
                        # scale_pi_by_accessibility with two alleles, every clamp as the oracle places it
                        s1 = w[1] * mp.mpf(float(s["kacc"][g]))
                        ctrl = 1 - s1
                        tot = max(ctrl + s1, mp.mpf(1))
                        p1 = min(max(s1 / tot, mp.mpf("1e-3")), 1 - mp.mpf("1e-3"))
                        e = mp.exp(mp.log(p1 / (1 - p1)) + mp.mpf(float(s["lpn"][g])))
                        pn = min(max(e / (1 + e), mp.mpf("1e-3")), 1 - mp.mpf("1e-3"))
                        w, dw = [1 - pn, pn], C_W_ACC * U53
                e_b = [sum(w[a] * comp[a][0][b] for a in range(len(w))) for b in range(B)]
                de_b = [sum(w[a] * comp[a][1][b] + dw * comp[a][0][b] for a in range(len(w))) for b in range(B)]
                for l, (sf, a0) in enumerate(liks):
                    sfr = [mp.mpf(float(sf[r, b])) for b in range(B)]
                    S = sum(e_b[b] * sfr[b] for b in range(B)) + eps
                    dS = sum(de_b[b] * sfr[b] for b in range(B))
                    a0g = mp.mpf(float(a0[g]))
                    for b in range(B):
                        raw = (e_b[b] * sfr[b] + eps / B) / S * a0g * int(sm[r, b])
                        if raw < eps:
                            alpha[l, r, b, g], floored[l, r, b, g] = EPS, True
                            continue
                        alpha[l, r, b, g] = float(raw)
                        budget[l, r, b, g] = float(a0g / S * sfr[b] * de_b[b] + raw / S * dS + C_FORM * U53 * raw)
    return alpha, budget, floored


def oracle_alpha(family, data, params, pi=None, acc_noise=None, kw=None):
    """The same planes by the oracle's float64 arithmetic (torch): every eps at 0."""
    T, G = data.n_targets, data.n_guides
    noise = {"eps_mu": torch.zeros(T, 1, dtype=torch.float64), "eps_sd": torch.zeros(T, 1, dtype=torch.float64)}
    if pi is not None:
        noise["pi"] = pi
    kw = dict(kw or {})
    if acc_noise is not None:
        noise["eps_noise"] = torch.zeros(G, dtype=torch.float64)
    _, concs = _spied(data, params, noise, kw, family)
    return np.stack([elbo.dirmult_concentration(*c).permute(0, 2, 1).numpy() for c in concs])


def alpha_ratio(got, alpha, budget, floored):
    """The worst ``|got - alpha| / budget`` over the unfloored elements and whether every floored element of ``alpha`` is
    exactly 1e-5 in ``got``."""
    got = np.asarray(got, dtype=np.float64)
    free = ~floored
    assert (budget[free] > 0).all()
    ratio = np.abs(got - alpha)[free] / budget[free]
    return float(ratio.max()), bool((got[floored] == EPS).all())
