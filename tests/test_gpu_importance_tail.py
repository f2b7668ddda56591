"""The Gauss-Jacobi rule for the pairs the marginal importance weights' quadrature leaves out, on the GPU
(bean_hip_log_weights_marginal_tail, csrc/bean_importance_tail.hpp): pairs / logw / tail_err against
the CPU rule with and without accessibility, more tail pairs than a wave has lanes, bit identity with the plain call
wherever no tail pair is involved, chunking and splits of the draws, the grid posterior's kernel at a draw's (mu, y),
refusals, the claim of the check on a screen with unedited guides against an exact posterior, and the CLI end to end.
-m gpu."""
import ctypes
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.grid_posterior import grid_posterior
from bean_amd.model.importance import MARGINAL_KEYS, TAIL_KEYS, marginal_summary
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

import importance_common as ic
import marginal_reference as mr
import tail_common as tc
import tail_reference as tr
from members_common import DEV, VAR, _h5ad_reader_present, _run, _without_columns  # noqa: F401
from oracle import elbo

pytestmark = pytest.mark.gpu
SEED = 101
LOG2 = math.log(2.0)
S, FIRST, Q = 3, 5, 32
# tests/test_gpu_grid_tail.py's cases - (guide, alpha_pi in units of log 2, control reads zeroed): the small exponent on
# pi_1, the mirrored case on pi_0, and a guide with no control reads at all
CASES = {"40": ((1, (5, -5), 1), (4, (3, -3), 1), (8, (-5, 5), 0), (12, (5, -5), None), (13, (5, -5), 1)),
         "130": ((3, (5, -5), 1), (70, (-5, 5), 0), (100, (4, -4), 1), (129, (5, -5), None)),
         # 40 guides unedited in both replicates: more tail pairs than a wave has lanes, the last wave ragged
         "130many": tuple((g, (5, -5), 1) for g in range(1, 121, 3))}
CONFIGS = [dict(), dict(use_bcmatch=False), dict(scale_by_accessibility=True, fit_noise=True),
           dict(use_bcmatch=False, scale_by_accessibility=True, fit_noise=True)]


def _id(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items()) or "plain"


def _screen(which, acc):
    data = (make_sorting_variant_screen(40, 3, seed=3, with_accessibility=acc) if which == "40"
            else make_sorting_variant_screen(130, 2, seed=11, mask_fraction=0.05, with_accessibility=acc))
    for g, _, allele in CASES[which]:
        tc.zero_control_counts(data, [g], allele)
    return data


@pytest.fixture(scope="module")
def screens():
    cache = {}

    def get(which, acc=False):
        if (which, acc) not in cache:
            cache[(which, acc)] = _screen(which, acc)
        return cache[(which, acc)]

    return get


@pytest.fixture(scope="module")
def engines(screens):
    from bean_amd import engine

    cache = {}

    def get(which, kw=None, family="MixtureNormal"):
        kw = kw or {}
        key = (which, family, _id(kw))
        if key not in cache:
            data = screens(which, bool(kw.get("scale_by_accessibility")))
            cache[key] = engine.HipSVI(family, data.to(DEV), num_steps=50, **kw)
            assert cache[key].guide_order is None
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def _set(eng, name, value):
    p = eng.unconstrained[name]
    p.copy_(torch.as_tensor(value, dtype=p.dtype).reshape(p.shape).to(p.device))


def _hand_set(eng, data, which, mu_loc=0.5, sd=1.0, tail=True, seed=3):
    """Parameters a fit could reach (tests/test_gpu_importance_marginal.py), alpha_pi at logs of powers of two - the
    float32 exp of which is the same on both sides - and with ``tail`` the CASES' values on their guides."""
    g = torch.Generator().manual_seed(seed)
    T, G = data.n_targets, data.n_guides
    _set(eng, "mu_loc", torch.full((T,), float(mu_loc)))
    _set(eng, "mu_scale", torch.full((T,), math.log(0.1)))
    _set(eng, "sd_loc", torch.full((T,), math.log(sd)))
    _set(eng, "sd_scale", torch.full((T,), math.log(0.05)))
    if "alpha_pi" in eng.unconstrained:
        alpha = torch.randint(-1, 3, (G, 2), generator=g).float()
        if tail:
            for guide, powers, _ in CASES[which]:
                alpha[guide] = torch.tensor(powers).float()
        _set(eng, "alpha_pi", alpha * LOG2)
    if "noise_loc" in eng.unconstrained:
        _set(eng, "noise_loc", 0.3 * torch.randn(G, generator=g))
        _set(eng, "noise_scale", math.log(0.655) + 0.1 * torch.randn(G, generator=g))


def _params(eng):
    return {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}


def _eps_noise(data, seed=9):
    return torch.randn(data.n_guides, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _reference(data, params, mu, y, kw, eps_noise=None):
    """What bean_hip_log_weights_marginal_tail forms at ONE draw (mu, y per target; with accessibility the injected noise):
    marginal_reference.marginal_log_weights with jacobi_rule at 64 nodes on the tail pairs, tail_err from the 48-node
    rule, and the summed magnitudes of their terms (tail_reference.grid_terms' forms)."""
    use_bc, acc = kw.get("use_bcmatch", True), bool(kw.get("scale_by_accessibility"))
    data64 = elbo.as_float64(data)
    T = data.n_targets
    tot, pairs, mag, pair_mag = mr.marginal_log_weights(data, params, mu, y, Q, use_bcmatch=use_bc,
                                                        scale_by_accessibility=acc, fit_noise=True, eps_noise=eps_noise)
    c_p = mr.model_conc(data, params)
    a_prime = mr.beta_exponents(data64, c_p)
    lpn = None
    if acc:
        loc = params["noise_loc"].double().reshape(-1)
        lpn = loc + eps_noise * params["noise_scale"].double().reshape(-1).exp()
    h = mr.PairIntegrand(data64, mu, y.exp(), c_p, use_bc, acc, lpn)
    rg = data.repguide_mask
    tail = (~(a_prime.min(-1).values >= mr.MARG_MIN_CONC)) & rg
    lognorm = (torch.lgamma(c_p.sum(-1)) - torch.lgamma(c_p).sum(-1))[None].expand_as(pairs)
    j64 = tr.jacobi_rule(h, a_prime, tr.TAIL_NODES, where=tail)
    j48 = tr.jacobi_rule(h, a_prime, tr.TAIL_CHECK_NODES, where=tail)
    zero = torch.zeros_like(pairs)
    g2t = torch.repeat_interleave(torch.arange(T), data.target_lengths)
    add = lambda v: torch.zeros(T, dtype=torch.float64).index_add_(0, g2t, v.sum(0))  # noqa: E731
    want_pairs = torch.where(tail, j64 - lognorm, pairs)
    want_mag = torch.where(tail, want_pairs.abs() + lognorm.abs(), pair_mag)
    err = torch.where(tail, (j64 - j48).abs(), zero)
    err_mag = torch.where(tail, (j64 - lognorm).abs() + (j48 - lognorm).abs() + 2.0 * lognorm.abs(), zero)
    return {"logw": tot + add(want_pairs - pairs), "mag": mag + add(want_mag - pair_mag), "pairs": want_pairs,
            "pair_mag": want_mag, "tail_err": add(err), "err_mag": add(err_mag), "tail": tail, "a_prime": a_prime}


def _check_against_reference(eng, data, kw, what):
    """S draws from FIRST on: pairs, logw and tail_err within 1e-9 of the summed magnitudes of their terms; returns the
    output, the references per draw and the largest deviations relative to the terms."""
    acc = bool(kw.get("scale_by_accessibility"))
    params = _params(eng)
    eps = _eps_noise(data) if acc else None
    if acc:
        eng.set_noise({"eps_noise": eps})
    try:
        out = eng.log_weights(FIRST, S, seed=SEED, pairs=True, integrate_pi=Q, tail_rule=True)
        torch.cuda.synchronize()
    finally:
        eng.set_noise(None)
    T = data.n_targets
    assert out["tail_err"].shape == (S, T) and out["tail_err"].dtype == torch.float64
    got = {k: v.cpu() for k, v in out.items()}
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("logw", "pairs", "tail_err")) and bool((got["tail_err"] >= 0).all())
    assert not torch.equal(got["mu"][0], got["mu"][1])
    worst = {"pair": 0.0, "logw": 0.0, "err": 0.0, "tail_err": 0.0}
    refs = []
    for j in range(S):
        want = _reference(data, params, got["mu"][j], got["y"][j], kw, eps)
        refs.append(want)
        n_un = mr.n_unresolved(data, params)
        assert got["n_unresolved"].tolist() == n_un.tolist() and int(want["tail"].sum()) == int(n_un.sum())
        assert bool((got["tail_err"][j][n_un == 0] == 0).all())
        dp = (got["pairs"][j] - want["pairs"]).abs()
        dl = (got["logw"][j] - want["logw"]).abs()
        de = (got["tail_err"][j] - want["tail_err"]).abs()
        worst["pair"] = max(worst["pair"], float((dp / want["pair_mag"].clamp(min=1.0)).max()))
        worst["logw"] = max(worst["logw"], float((dl / want["mag"]).max()))
        worst["err"] = max(worst["err"], float((de / want["err_mag"].clamp(min=1.0)).max()))
        worst["tail_err"] = max(worst["tail_err"], float(got["tail_err"][j].max()))
        print(f"{what} draw {FIRST + j}: pairs |diff| {float(dp.max()):.2e}, logw |diff| {float(dl.max()):.2e}, tail_err "
              f"|diff| {float(de.max()):.2e}; largest tail_err {float(got['tail_err'][j].max()):.2e}")
        assert bool((dp <= 1e-9 * want["pair_mag"]).all()), (what, j, float(dp.max()))
        assert bool((dl <= 1e-9 * want["mag"]).all()), (what, j, float(dl.max()))
        assert bool((de <= 1e-9 * want["err_mag"]).all()), (what, j, float(de.max()))
    print(f"{what}: {int(refs[0]['tail'].sum())} tail pairs; largest deviation, relative to the terms: pairs "
          f"{worst['pair']:.2e}, logw {worst['logw']:.2e}, tail_err {worst['err']:.2e}; largest tail_err {worst['tail_err']:.2e}")
    return out, refs


# ------------------------------------------------------------------ 1. against the CPU rule
@pytest.mark.parametrize("size", ["40", "130"])
@pytest.mark.parametrize("kw", CONFIGS, ids=_id)
def test_pairs_logw_and_tail_err_are_the_cpu_rules(engines, screens, kw, size):
    """pairs[d, r, g], logw[d, t] and tail_err[d, t] of draws 5 .. 7 against jacobi_rule at 64 and 48 nodes on
    PairIntegrand at the device's own mu and y (with accessibility: the injected noise), within 1e-9 of the summed
    magnitudes of their terms - the bound of tests/test_gpu_grid_tail.py.  The tail pairs cover the small exponent on
    pi_1, on pi_0, and a guide with no control reads at all."""
    acc = bool(kw.get("scale_by_accessibility"))
    data, eng = screens(size, acc), engines(size, kw)
    _hand_set(eng, data, size)
    _, refs = _check_against_reference(eng, data, kw, f"{size} {_id(kw)}")
    tail, a_prime = refs[0]["tail"], refs[0]["a_prime"]
    assert int(tail.sum()) >= len(CASES[size])
    sides = {int(v) for v in tr.side_of(a_prime)[tail].tolist()}
    assert sides == {0, 1}
    no_reads = [g for g, _, allele in CASES[size] if allele is None]
    assert no_reads and all(bool(tail[:, g].any()) and float(data.allele_counts_control[:, :, g].sum()) == 0 for g in no_reads)


# ------------------------------------------------------------------ 2. more tail pairs than a wave has lanes
@pytest.mark.parametrize("kw", [dict(), dict(scale_by_accessibility=True, fit_noise=True)], ids=_id)
def test_more_than_64_tail_pairs(engines, screens, kw):
    acc = bool(kw.get("scale_by_accessibility"))
    data, eng = screens("130many", acc), engines("130many", kw)
    _hand_set(eng, data, "130many")
    out, refs = _check_against_reference(eng, data, kw, f"130many {_id(kw)}")
    n_tail = int(refs[0]["tail"].sum())
    assert n_tail > 64 and (n_tail * S) % 64 != 0 and int(out["n_unresolved"].sum()) == n_tail


# ------------------------------------------------------------------ 3. bit identity
@pytest.mark.parametrize("kw", [dict(), dict(scale_by_accessibility=True, fit_noise=True)], ids=_id)
def test_what_the_rule_does_not_touch_keeps_its_bits(engines, screens, kw):
    acc = bool(kw.get("scale_by_accessibility"))
    data, eng = screens("130", acc), engines("130", kw)
    _hand_set(eng, data, "130")
    plain = eng.log_weights(FIRST, S, seed=SEED, pairs=True, integrate_pi=Q)
    out = eng.log_weights(FIRST, S, seed=SEED, pairs=True, integrate_pi=Q, tail_rule=True)
    torch.cuda.synchronize()
    assert "tail_err" not in plain
    for k in ("mu", "y", "n_unresolved"):
        assert torch.equal(out[k], plain[k]), k
    c_p = mr.model_conc(data, _params(eng))
    tail = ((~mr.resolved(elbo.as_float64(data), c_p)) & data.repguide_mask).to(DEV)
    assert int(tail.sum()) == int(out["n_unresolved"].sum()) > 0
    assert torch.equal(out["pairs"][:, ~tail], plain["pairs"][:, ~tail])
    assert not bool((out["pairs"][:, tail] == plain["pairs"][:, tail]).any())
    without = out["n_unresolved"] == 0
    assert bool(without.any()) and torch.equal(out["logw"][:, without], plain["logw"][:, without])
    assert not bool((out["logw"][:, ~without] == plain["logw"][:, ~without]).any())
    assert bool((out["tail_err"][:, without] == 0).all()) and bool((out["tail_err"][:, ~without] > 0).all())


@pytest.mark.parametrize("family", ["MixtureNormal", "Normal"])
def test_without_tail_pairs_it_is_the_plain_call(engines, screens, family):
    data, eng = screens("130"), engines("130", family=family)
    _hand_set(eng, data, "130", tail=False)
    plain = eng.log_weights(FIRST, S, seed=SEED, pairs=True, integrate_pi=Q)
    out = eng.log_weights(FIRST, S, seed=SEED, pairs=True, integrate_pi=Q, tail_rule=True)
    torch.cuda.synchronize()
    assert int(out["n_unresolved"].abs().sum()) == 0
    for k in ("logw", "mu", "y", "pairs", "n_unresolved"):
        assert torch.equal(out[k], plain[k]), k
    assert out["tail_err"].shape == (S, data.n_targets) and bool((out["tail_err"] == 0).all())


@pytest.mark.parametrize("kw", [dict(), dict(scale_by_accessibility=True, fit_noise=True)], ids=_id)
def test_chunks_and_splits_give_the_same_bits(engines, screens, kw):
    """LOGW_PAIR_BYTES patched down so that a chunk holds 1 or 2 draws: the bits of one call.  Draw d is the same
    whichever first_draw / n_draws split reaches it."""
    acc = bool(kw.get("scale_by_accessibility"))
    data, eng = screens("40", acc), engines("40", kw)
    _hand_set(eng, data, "40")
    R, G = data.n_reps, data.n_guides
    call = lambda first, n: eng.log_weights(first, n, seed=SEED, pairs=True, integrate_pi=Q, tail_rule=True)  # noqa: E731
    whole = call(FIRST, S)
    keys = ("logw", "mu", "y", "pairs", "tail_err")
    assert float(whole["tail_err"].max()) > 0
    for per_chunk in (1, 2):
        eng.LOGW_PAIR_BYTES = per_chunk * 8 * R * G
        try:
            chunked = call(FIRST, S)
        finally:
            del eng.LOGW_PAIR_BYTES
        torch.cuda.synchronize()
        for k in keys + ("n_unresolved",):
            assert torch.equal(whole[k], chunked[k]), (per_chunk, k)
    a, b = call(FIRST, 1), call(FIRST + 1, S - 1)
    wide = call(FIRST - 2, S + 4)
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(whole[k], torch.cat([a[k], b[k]])), k
        assert torch.equal(whole[k], wide[k][2:2 + S]), k
    with pytest.raises(ValueError, match="needs integrate_pi"):
        eng.log_weights(FIRST, S, tail_rule=True)


# ------------------------------------------------------------------ 4. the grid posterior's kernel at a draw's (mu, y)
@pytest.mark.parametrize("size", ["40", "130"])
def test_a_draw_is_the_grid_kernels_node(engines, screens, size):
    """marginal_grid(tail_rule=True, pairs=True) on a one-node grid centred at a draw's (mu, y) gives that draw's tail-pair
    slots and tail_err within the 1e-9 bound (two kernels may contract differently: not equal bits)."""
    data, eng = screens(size), engines(size)
    _hand_set(eng, data, size)
    out, refs = _check_against_reference(eng, data, {}, f"{size} plain")
    step = torch.full((data.n_targets,), 0.1, dtype=torch.float64)
    for j in range(S):
        node = eng.marginal_grid(out["mu"][j], out["y"][j], step, step, 1, 1, nodes=Q, pairs=True, tail_rule=True)
        torch.cuda.synchronize()
        tail = refs[j]["tail"]
        dp = (node["pairs"][0, 0].cpu() - out["pairs"][j].cpu()).abs()
        de = (node["tail_err"][0, 0].cpu() - out["tail_err"][j].cpu()).abs()
        print(f"{size} draw {FIRST + j}: against k_grid_pairs_tail: tail slots |diff| {float(dp[tail].max()):.2e}, tail_err "
              f"|diff| {float(de.max()):.2e}")
        assert bool((dp[tail] <= 1e-9 * refs[j]["pair_mag"][tail]).all())
        assert bool((de <= 1e-9 * refs[j]["err_mag"]).all())
        assert float(node["tail_err"].max()) > 0


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens("130")
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, G, T = data.n_reps, data.n_guides, data.n_targets
    lw, mu, y = (torch.zeros(S * T, dtype=torch.float64, device=DEV) for _ in range(3))
    te = torch.full((S * T,), -1.0, dtype=torch.float64, device=DEV)
    pl = torch.zeros(S * R * G, dtype=torch.float64, device=DEV)
    un = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    nt, npair, nu = 8 * S * T, 8 * S * R * G, 4 * T
    name = "bean_hip_log_weights_marginal_tail"
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
    _hand_set(eng, data, "130")
    call = lambda *a, n=S, q=Q: lib.bean_hip_log_weights_marginal_tail(eng._h, SEED, FIRST, n, q, *a, eng._sptr())  # noqa: E731
    good = (p(lw), nt, p(mu), nt, p(y), nt, p(pl), npair, p(un), nu, p(te), nt)
    assert call(*good, q=20) < 0 and "n_nodes" in err() and "16, 32 or 64" in err() and err().startswith(name + ":")
    assert call(*good[:10], p(te), nt + 8) < 0 and "tail_err_out" in err() and str(nt) in err()
    assert call(*good[:10], p(te), nt - 8) < 0 and "tail_err_out" in err()
    assert call(*good[:10], None, nt) < 0 and "tail_err_out" in err()
    assert call(p(lw), nt - 8, *good[2:]) < 0 and "logw_out" in err()
    assert call(*good[:8], p(un), nu + 4, *good[10:]) < 0 and "unresolved_out" in err()
    for n in (0, _lib.MAX_LOGW_DRAWS + 1):
        assert call(*good, n=n) < 0 and "n_draws" in err()
    assert lib.bean_hip_log_weights_marginal_tail(None, SEED, FIRST, S, Q, *good, None) < 0 and "null handle" in err()
    # an unprepared handle of the same shape
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(eng._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_log_weights_marginal_tail(h, SEED, FIRST, S, Q, *good, None) < 0
    assert err() == name + ": call bean_hip_prepare first"
    assert lib.bean_hip_destroy(h) == 0
    torch.cuda.synchronize()
    assert float(lw.abs().sum()) == 0 and float(pl.abs().sum()) == 0 and bool((un == -1).all()) and bool((te == -1).all())
    assert call(*good) == 0
    torch.cuda.synchronize()
    want = eng.log_weights(FIRST, S, seed=SEED, integrate_pi=Q, tail_rule=True)
    assert torch.equal(lw.reshape(S, T), want["logw"]) and torch.equal(te.reshape(S, T), want["tail_err"])
    assert torch.equal(un, want["n_unresolved"]) and int(un.sum()) > 0
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()
    for other in (engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10)):
        assert lib.bean_hip_log_weights_marginal_tail(other._h, SEED, FIRST, S, Q, *good, other._sptr()) < 0
        assert "bean_hip_predictive_supported" in err() and err().startswith(name)
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.log_weights(FIRST, S, integrate_pi=Q, tail_rule=True)
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()


# ------------------------------------------------------------------ 6. the check does what it claims
@pytest.fixture(scope="module")
def claim():
    """tail_common.claim_screen_with_unedited_guides(): the first guide of every target unedited, three tail pairs per
    target.  q(mu, log sd) is set around the posterior as section 21 sets it - its scales, marginal_reference.CLAIM_*,
    centred per target at the grid posterior's mean of mu and log of its mean sd (the planted effects of targets 0, 2
    and 5 lie far outside N(0, 0.2)) - S = 4096 draws, Q = 32; the summaries with and without the rule."""
    from bean_amd import engine

    data, alpha = tc.claim_screen_with_unedited_guides()
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=10)
    for k, v in mr.claim_params(data).items():
        eng.unconstrained[k].copy_(v.reshape(eng.unconstrained[k].shape).to(DEV))
    _set(eng, "alpha_pi", alpha)
    grid = grid_posterior(eng, tail_rule=True)
    assert bool(grid["grid_ok"].all())
    _set(eng, "mu_loc", grid["mu_grid"].float())
    _set(eng, "sd_loc", grid["sd_grid"].log().float())
    res = {}
    for rule in (False, True):
        kw = {"tail_rule": True} if rule else {}
        m = eng.log_weights(0, ic.CLAIM_DRAWS, seed=SEED, integrate_pi=Q, **kw)
        torch.cuda.synchronize()
        res[rule] = {k: v.cpu() for k, v in marginal_summary(m["logw"], m["mu"], m["n_unresolved"],
                                                             **({"tail_err": m["tail_err"]} if rule else {})).items()}
    eng.close()
    c_p = mr.model_conc(data, {"alpha_pi": alpha})
    return data, c_p, res


def test_without_the_rule_every_claim_target_is_left_out(claim):
    data, _, res = claim
    assert data.n_targets == 8 and res[False]["n_pairs_unresolved"].tolist() == [3.0] * 8
    assert set(res[False]) == set(MARGINAL_KEYS) and set(res[True]) == set(MARGINAL_KEYS) | set(TAIL_KEYS)
    for k in MARGINAL_KEYS[:4]:
        assert bool(torch.isnan(res[False][k]).all()), k
        assert bool(torch.isfinite(res[True][k]).all()), k
    assert res[True]["n_pairs_tail"].tolist() == [3.0] * 8
    assert bool((res[True]["is_tail_err"] <= 1e-3 * res[True]["n_pairs_tail"]).all())
    assert bool((res[True]["psis_k_marg"] < 0.7).all()), res[True]["psis_k_marg"]
    print(f"is_tail_err {[f'{v:.1e}' for v in res[True]['is_tail_err'].tolist()]} against 1e-3 per tail pair")


@pytest.mark.parametrize("t", range(8))
def test_marginal_check_with_the_rule_recovers_the_exact_posterior(claim, t):
    """Per target: it passes the bar, psis_k_marg < 0.7, and |mu_is_marg - E[mu | x]| <= 4 sd[mu | x] / sqrt(is_ess_marg)
    against tail_reference.exact_marginal_moments (the 128-node Jacobi rule inside for the tail pairs), whose grid must
    have a border density below 1e-6 of the peak and a mean that moves by less than a tenth of the cap when the step is
    doubled - marginal_reference.assert_marginal_claim's criterion, on every target.  Measured: DESIGN.md section 25."""
    data, c_p, res = claim
    s = res[True]
    idx = ic.target_guides(data, t)
    ex = tr.exact_marginal_moments(elbo.as_float64(data[idx]), c_p[idx])
    k, ess = float(s["psis_k_marg"][t]), float(s["is_ess_marg"][t])
    got, got_sd = float(s["mu_is_marg"][t]), float(s["mu_sd_is_marg"][t])
    cap = 4.0 * ex["sd"] / math.sqrt(ess)
    print(f"| {t} | {k:.2f} | {ess:.0f} | {got:.5f} | {ex['mean']:.5f} | {abs(got - ex['mean']):.5f} | {cap:.5f} | {got_sd:.5f} | "
          f"{ex['sd']:.5f} | {float(s['is_tail_err'][t]):.1e} | {ex['border']:.1e} | {abs(ex['mean'] - ex['mean_coarse']):.1e} |")
    assert float(s["is_tail_err"][t]) <= 1e-3 * float(s["n_pairs_tail"][t])
    assert ex["border"] < 1e-6 and abs(ex["mean"] - ex["mean_coarse"]) < 0.1 * cap, (t, ex, cap)
    assert k < 0.7, (t, k)
    assert abs(got - ex["mean"]) <= cap, (t, got, ex["mean"], cap)


# ------------------------------------------------------------------ 7. CLI
def test_cli_importance_tail_rule(tmp_path, caplog):
    """`bean run` on the fixture, 300 steps, --importance-check 200 --importance-integrate-pi.  With
    --importance-tail-rule every target with tail pairs has a finite is_tail_err and marginal numbers exactly where the bar
    passes; every other file, and every other column of the element table, is that of the run without the flag."""
    import logging

    caplog.set_level(logging.INFO, logger="bean_run")
    base = ["sorting", "variant", VAR, "--n-iter", "300", "--importance-check", "200", "--importance-integrate-pi"]
    d1 = _run(str(tmp_path / "tail"), *base, "--importance-tail-rule")
    d0 = _run(str(tmp_path / "plain"), *base)
    name = "bean_element_result.MixtureNormal.csv"
    marg = list(MARGINAL_KEYS[:4])
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0))
    for f in os.listdir(d0):
        if f != name and not f.endswith(".log"):
            assert open(f"{d1}/{f}", "rb").read() == open(f"{d0}/{f}", "rb").read(), f
    assert _without_columns(f"{d1}/{name}", marg + list(TAIL_KEYS)) == _without_columns(f"{d0}/{name}", marg)
    el = pd.read_csv(f"{d1}/{name}", index_col=0)
    plain = pd.read_csv(f"{d0}/{name}", index_col=0)
    assert [c for c in el.columns if c not in plain.columns] == list(TAIL_KEYS)
    cols = list(el.columns)
    assert cols[cols.index("n_pairs_unresolved") + 1:][:2] == list(TAIL_KEYS)  # behind the marginal columns
    assert el["n_pairs_tail"].dtype == np.int64 and el["n_pairs_tail"].tolist() == el["n_pairs_unresolved"].tolist()
    had = el["n_pairs_tail"] > 0
    assert int(had.sum()) == 5 and len(el) == 6
    assert bool(np.isfinite(el["is_tail_err"]).all()) and bool((el["is_tail_err"][~had] == 0).all())
    passes = el["is_tail_err"] <= 1e-3 * el["n_pairs_tail"]
    for c in marg:
        assert bool(np.isfinite(el[c][passes]).all()) and bool(el[c][~passes].isna().all()), c
        assert bool(plain[c][had].isna().all()) and plain[c][~had].equals(el[c][~had]), c
    print(f"CLI: {int(had.sum())} of {len(el)} targets had tail pairs; {int((had & passes).sum())} of those have numbers; "
          f"{int((had & ~passes).sum())} refused by the tail bar; is_tail_err {el['is_tail_err'].tolist()}; psis_k_marg "
          f"{el['psis_k_marg'].tolist()}")
    lines = [r.getMessage() for r in caplog.records if "tail rule:" in r.getMessage()]
    assert len(lines) == 1 and f"{int(had.sum())} of {len(el)} targets" in lines[0] and "refused by the tail bar" in lines[0]
    assert f"{int((had & passes).sum())} of those" in lines[0]
