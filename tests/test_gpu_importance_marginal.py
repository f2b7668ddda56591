"""Importance weights with pi integrated out on the GPU (bean_hip_log_weights_marginal, csrc/bean_importance_marg.hpp):
per pair against the CPU rule, the identity of the draws, the Normal family, unresolved pairs, the claim of the check
against an exact posterior, its refusals, and the CLI end to end.  -m gpu."""
import copy
import ctypes
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.importance import MARGINAL_KEYS, importance_summary, marginal_summary
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

import importance_common as ic
import marginal_reference as mr
from members_common import CONFIGS, DEV, VAR, _h5ad_reader_present, _kw_of, _run, _without_columns  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = 101
MIXTURE = [kw for family, kw in CONFIGS if family == "MixtureNormal"]
EFFECTS = ((0.0, 1.0), (0.5, 1.0), (2.0, 1.3))  # (mu_loc, exp(sd_loc)): null, moderate, strong


# ------------------------------------------------------------------ screens and engines, built once per module
@pytest.fixture(scope="module")
def screens():
    big = dict(seed=11, mask_fraction=0.05)
    return {
        "40": make_sorting_variant_screen(40, 3, seed=3),
        "40acc": make_sorting_variant_screen(40, 3, seed=3, with_accessibility=True),
        # two tiles, the second ragged; masked pairs
        "130": make_sorting_variant_screen(130, 2, **big),
        "130acc": make_sorting_variant_screen(130, 2, with_accessibility=True, **big),
    }


@pytest.fixture(scope="module")
def engines(screens):
    from bean_amd import engine

    cache = {}

    def get(which, family, kw):
        key = (which, family, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in cache:
            data = screens[which]
            cache[key] = engine.HipSVI(family, data.to(DEV), num_steps=50, **_kw_of(kw, data))
            assert cache[key].guide_order is None  # parameters and pairs are in screen order
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def _which(size, kw):
    return size + ("acc" if kw.get("scale_by_accessibility") else "")


def _set(eng, name, value):
    p = eng.unconstrained[name]
    p.copy_(torch.as_tensor(value, dtype=p.dtype).reshape(p.shape).to(p.device))


def _hand_set(eng, data, mu_loc, sd, seed=3):
    """Parameters a fit could reach: the effect at ``mu_loc``, sd around ``sd``, every guide's alpha_pi a power of two (0.5
    ... 4: float32 exp of its log rounds to it in any implementation within half an ulp, so the device and the reference
    form the same c_p - they differ by a factor of up to 8 between the alleles), noise sites away from their priors."""
    g = torch.Generator().manual_seed(seed)
    T, G = data.n_targets, data.n_guides
    _set(eng, "mu_loc", torch.full((T,), float(mu_loc)))
    _set(eng, "mu_scale", torch.full((T,), math.log(0.1)))
    _set(eng, "sd_loc", torch.full((T,), math.log(sd)))
    _set(eng, "sd_scale", torch.full((T,), math.log(0.05)))
    _set(eng, "alpha_pi", torch.randint(-1, 3, (G, 2), generator=g).float() * math.log(2.0))
    if "noise_loc" in eng.unconstrained:
        _set(eng, "noise_loc", 0.3 * torch.randn(G, generator=g))
        _set(eng, "noise_scale", math.log(0.655) + 0.1 * torch.randn(G, generator=g))


def _given(data, acc, seed=9):
    g = torch.Generator().manual_seed(seed)
    T, G, R = data.n_targets, data.n_guides, data.n_reps
    given = {"eps_mu": torch.randn(T, 1, generator=g, dtype=torch.float64),
             "eps_sd": torch.randn(T, 1, generator=g, dtype=torch.float64)}
    p1 = 0.05 + 0.9 * torch.rand(R, 1, G, generator=g, dtype=torch.float64)
    given["pi"] = torch.stack([1 - p1, p1], -1)  # injected and ignored
    if acc:
        given["eps_noise"] = torch.randn(G, generator=g, dtype=torch.float64)
    return given


def _id(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items()) or "plain"


# ------------------------------------------------------------------ 1. per pair against the CPU rule
@pytest.mark.parametrize("size", ["40", "130"])
@pytest.mark.parametrize("kw", MIXTURE, ids=_id)
def test_pairs_and_weights_are_the_cpu_rules(engines, screens, kw, size):
    """pairs[d, r, g] and logw[d, t] against tests/marginal_reference.py at the same Q (32; 16 and 64 at the moderate
    effect), (mu, sd) injected through set_noise at null, moderate and strong effect: within 1e-9 of the summed
    magnitudes of the pair's, the target's terms.  Largest deviations measured: see DESIGN.md section 21."""
    which = _which(size, kw)
    data, eng = screens[which], engines(which, "MixtureNormal", kw)
    okw = _kw_of(kw, data)
    acc = bool(okw.get("scale_by_accessibility"))
    prior = okw.get("prior_params")
    if prior is not None:
        prior = {k: torch.as_tensor(v).double() for k, v in prior.items()}
    given = _given(data, acc)
    worst_pair = worst_logw = 0.0
    for mu_loc, sd in EFFECTS:
        _hand_set(eng, data, mu_loc, sd)
        params = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
        # loc + eps * scale, formed on the device as tests/test_gpu_importance.py forms it (the last bit of exp is the
        # device's)
        p64 = {k: v.detach().double().reshape(-1) for k, v in eng.unconstrained.items() if k in ic.PER_TARGET}
        mu = (p64["mu_loc"] + given["eps_mu"].to(DEV).reshape(-1) * p64["mu_scale"].exp()).cpu()
        y = (p64["sd_loc"] + given["eps_sd"].to(DEV).reshape(-1) * p64["sd_scale"].exp()).cpu()
        eng.set_noise(given)
        try:
            for Q in ((16, 32, 64) if mu_loc == 0.5 else (32,)):
                out = eng.log_weights(3, 2, seed=SEED, pairs=True, integrate_pi=Q)
                torch.cuda.synchronize()
                assert torch.equal(out["mu"][0].cpu(), mu) and torch.equal(out["y"][0].cpu(), y)
                assert torch.equal(out["logw"][0], out["logw"][1]) and torch.equal(out["pairs"][0], out["pairs"][1])
                want, want_pairs, mag, pair_mag = mr.marginal_log_weights(
                    data, params, mu, y, Q, use_bcmatch=okw.get("use_bcmatch", True), scale_by_accessibility=acc,
                    fit_noise=okw.get("fit_noise", True), eps_noise=given.get("eps_noise"), prior_params=prior)
                got, got_pairs = out["logw"][0].cpu(), out["pairs"][0].cpu()
                assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_pairs).all())
                assert bool((got_pairs[~data.repguide_mask] == 0).all())
                dp = ((got_pairs - want_pairs).abs() / pair_mag.clamp(min=1.0)).max()
                dl = ((got - want).abs() / mag).max()
                worst_pair, worst_logw = max(worst_pair, float(dp)), max(worst_logw, float(dl))
                print(f"{which} {_id(kw)} mu_loc {mu_loc} Q {Q}: pairs |diff| {float((got_pairs - want_pairs).abs().max()):.2e} "
                      f"({float(dp):.2e} of the terms), logw |diff| {float((got - want).abs().max()):.2e} ({float(dl):.2e})")
                assert bool(((got_pairs - want_pairs).abs() <= 1e-9 * pair_mag).all())
                assert bool(((got - want).abs() <= 1e-9 * mag).all())
                assert out["n_unresolved"].cpu().tolist() == mr.n_unresolved(data, params).tolist()
        finally:
            eng.set_noise(None)
    print(f"{which} {_id(kw)}: largest deviation, relative to the terms: pairs {worst_pair:.2e}, logw {worst_logw:.2e}")


# ------------------------------------------------------------------ 2. the draws are log_weights' draws
def test_draws_are_those_of_log_weights_and_chunks_give_the_same_bits(engines, screens):
    eng = engines("130", "MixtureNormal", {})
    _hand_set(eng, screens["130"], 0.5, 1.0)
    joint = eng.log_weights(2, 7, seed=SEED)
    whole = eng.log_weights(2, 7, seed=SEED, pairs=True, integrate_pi=32)
    a = eng.log_weights(2, 3, seed=SEED, pairs=True, integrate_pi=32)
    b = eng.log_weights(5, 4, seed=SEED, pairs=True, integrate_pi=32)
    R, G = eng.data.n_reps, eng.data.n_guides
    eng.LOGW_PAIR_BYTES = 2 * 8 * R * G
    try:
        chunked = eng.log_weights(2, 7, seed=SEED, pairs=True, integrate_pi=32)
    finally:
        del eng.LOGW_PAIR_BYTES
    torch.cuda.synchronize()
    assert torch.equal(whole["mu"], joint["mu"]) and torch.equal(whole["y"], joint["y"])
    assert not torch.equal(whole["logw"], joint["logw"])
    for k in ("logw", "mu", "y", "pairs"):
        assert torch.equal(whole[k], torch.cat([a[k], b[k]])), k
        assert torch.equal(whole[k], chunked[k]), k
    assert torch.equal(whole["n_unresolved"], chunked["n_unresolved"]) and whole["n_unresolved"].dtype == torch.int32
    assert not bool((whole["logw"][0] == whole["logw"][1]).all())
    with pytest.raises(ValueError, match="16, 32, 64"):
        eng.log_weights(0, 2, integrate_pi=20)


# ------------------------------------------------------------------ 3. the Normal family has no pi
@pytest.mark.parametrize("kw", [dict(), dict(use_bcmatch=False)], ids=_id)
def test_normal_family_weights_are_the_joint_ones(engines, kw):
    eng = engines("130", "Normal", kw)
    joint = eng.log_weights(1, 5, seed=SEED, pairs=True)
    marg = eng.log_weights(1, 5, seed=SEED, pairs=True, integrate_pi=64)
    torch.cuda.synchronize()
    for k in ("logw", "mu", "y", "pairs"):
        assert torch.equal(joint[k], marg[k]), k
    assert marg["n_unresolved"].shape == (eng.T,) and int(marg["n_unresolved"].abs().sum()) == 0


# ------------------------------------------------------------------ 4. unresolved pairs
def test_an_unedited_guide_leaves_its_target_out_and_no_other(screens):
    """One guide gets c_p1 < 0.1 and no edited control reads: its target counts as many unresolved pairs as the guide has
    unmasked replicates and has NaN marginal columns; every other target's weights keep their bits."""
    from bean_amd import engine

    data = screens["130"]
    nrg = data.repguide_mask.sum(0)
    off = data.target_offsets.tolist()
    # a guide with a masked and an unmasked replicate where the screen has one, in a target that is not the first
    cand = [g for g in range(off[1], data.n_guides) if 0 < int(nrg[g]) < data.n_reps] or [off[1] + 2]
    gi = cand[0]
    t0 = int(torch.repeat_interleave(torch.arange(data.n_targets), data.target_lengths)[gi])
    planted = copy.copy(data)
    planted.allele_counts_control = data.allele_counts_control.clone()
    planted.allele_counts_control[:, :, gi, 1] = 0
    S = 64
    outs = []
    for d, plant in ((data, False), (planted, True)):
        eng = engine.HipSVI("MixtureNormal", d.to(DEV), num_steps=10)
        assert eng.guide_order is None
        if plant:
            eng.unconstrained["alpha_pi"][gi, 1] = math.log(1e-4)
            c_p1 = float(mr.model_conc(d, {"alpha_pi": eng.unconstrained["alpha_pi"]})[gi, 1])
            assert 0 < c_p1 < 0.1, c_p1
        outs.append(eng.log_weights(0, S, seed=SEED, integrate_pi=32))
        torch.cuda.synchronize()
        eng.close()
    plain, got = outs
    assert int(plain["n_unresolved"].abs().sum()) == 0
    want = torch.zeros(data.n_targets, dtype=torch.int32)
    want[t0] = int(nrg[gi])
    assert int(nrg[gi]) >= 1 and got["n_unresolved"].cpu().tolist() == want.tolist()
    others = torch.arange(data.n_targets) != t0
    assert torch.equal(got["logw"][:, others.to(DEV)], plain["logw"][:, others.to(DEV)])
    assert not torch.equal(got["logw"][:, t0], plain["logw"][:, t0])
    summary = marginal_summary(got["logw"], got["mu"], got["n_unresolved"])
    for k in MARGINAL_KEYS[:4]:
        assert bool(torch.isnan(summary[k][t0])) and bool(torch.isfinite(summary[k][others.to(DEV)]).all()), k
    assert float(summary["n_pairs_unresolved"][t0]) == float(nrg[gi])


# ------------------------------------------------------------------ 5. the check does what it claims
def test_marginal_check_recovers_the_exact_posterior():
    """MixtureNormal on importance_common.claim_screen(), alpha_pi at its initial value, q(mu, log sd) set by hand
    (marginal_reference.CLAIM_*), S = 4096 draws, Q = 32.  The exact E[mu | x] and sd[mu | x] of the CLAIM_TARGETS come
    from 2-D quadrature of the marginal log joint (the Q = 64 rule inside): |mu_is_marg - E| <= 4 sd / sqrt(is_ess_marg)
    wherever psis_k_marg < 0.7, on at least two.  tests/test_importance_marginal_cpu.py makes the same claim with the CPU
    rule and torch's generator alone."""
    from bean_amd import engine

    data = ic.claim_screen()
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=10)
    for k, v in mr.claim_params(data).items():
        eng.unconstrained[k].copy_(v.reshape(eng.unconstrained[k].shape).to(DEV))
    joint = eng.log_weights(0, ic.CLAIM_DRAWS, seed=SEED)
    marg = eng.log_weights(0, ic.CLAIM_DRAWS, seed=SEED, integrate_pi=32)
    torch.cuda.synchronize()
    eng.close()
    js = {k: v.cpu() for k, v in importance_summary(joint["logw"], joint["mu"]).items()}
    summary = {k: v.cpu() for k, v in marginal_summary(marg["logw"], marg["mu"], marg["n_unresolved"]).items()}
    assert int(summary["n_pairs_unresolved"].sum()) == 0
    for t in ic.CLAIM_TARGETS:
        print(f"target {t}: joint psis_k {float(js['psis_k'][t]):.3f} (is_ess {float(js['is_ess'][t]):.1f}), "
              f"psis_k_marg {float(summary['psis_k_marg'][t]):.3f} (is_ess_marg {float(summary['is_ess_marg'][t]):.1f})")
    mr.assert_marginal_claim(summary, data, ic.CLAIM_TARGETS, "device")


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["130"].to(DEV)
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, G, T = data.n_reps, data.n_guides, data.n_targets
    S = 3
    lw, mu, y = (torch.zeros(S * T, dtype=torch.float64, device=DEV) for _ in range(3))
    pl = torch.zeros(S * R * G, dtype=torch.float64, device=DEV)
    un = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    nt, npair, nu = 8 * S * T, 8 * S * R * G, 4 * T
    name = "bean_hip_log_weights_marginal"

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    call = lambda *a, n=S, q=32: lib.bean_hip_log_weights_marginal(eng._h, SEED, 0, n, q, *a, eng._sptr())  # noqa: E731
    good = (p(lw), nt, p(mu), nt, p(y), nt, p(pl), npair, p(un), nu)
    for q in (20, 0, 128):
        assert call(*good, q=q) < 0 and "n_nodes" in err() and "16, 32 or 64" in err() and err().startswith(name)
    assert call(p(lw), nt - 8, *good[2:]) < 0 and "logw_out" in err()
    assert call(*good[:2], p(mu), nt + 8, *good[4:]) < 0 and "mu_out" in err()
    assert call(*good[:4], p(y), nt - 8, *good[6:]) < 0 and "y_out" in err()
    assert call(*good[:6], p(pl), npair - 8, *good[8:]) < 0 and "pair_out" in err()
    assert call(*good[:8], p(un), nu + 4) < 0 and "unresolved_out" in err()
    assert call(*good[:8], None, 0) < 0 and "unresolved_out" in err()
    for n in (0, _lib.MAX_LOGW_DRAWS + 1):
        assert call(*good, n=n) < 0 and "n_draws" in err()
    assert lib.bean_hip_log_weights_marginal(None, SEED, 0, S, 32, *good, None) < 0 and "null handle" in err()
    torch.cuda.synchronize()
    assert float(lw.abs().sum()) == 0 and float(pl.abs().sum()) == 0 and bool((un == -1).all())  # nothing was launched
    assert call(*good) == 0
    assert call(*good[:4], None, 0, *good[6:]) == 0  # y_out is optional
    torch.cuda.synchronize()
    want = eng.log_weights(0, S, seed=SEED, integrate_pi=32)
    assert torch.equal(lw.reshape(S, T), want["logw"]) and torch.equal(un, want["n_unresolved"])
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()

    neg = make_sorting_variant_screen(900, 3, seed=32)
    neg = neg[neg.negctrl_guide_idx]
    for other in (engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("ControlNormal", neg.to(DEV), num_steps=10)):
        assert lib.bean_hip_log_weights_marginal(other._h, SEED, 0, S, 32, *good, other._sptr()) < 0
        assert "bean_hip_predictive_supported" in err() and err().startswith(name)
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.log_weights(0, 2, integrate_pi=32)
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()


# ------------------------------------------------------------------ 7. CLI
def test_cli_importance_integrate_pi(tmp_path, caplog):
    import logging

    caplog.set_level(logging.INFO, logger="bean_run")
    base = ["sorting", "variant", VAR, "--n-iter", "200", "--importance-check", "100"]
    d1 = _run(str(tmp_path / "marg"), *base, "--importance-integrate-pi", "--importance-nodes", "16")
    d0 = _run(str(tmp_path / "joint"), *base)
    own = list(MARGINAL_KEYS)
    name = "bean_element_result.MixtureNormal.csv"
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0))
    for f in os.listdir(d0):
        if f != name and not f.endswith(".log"):  # (the run's log names its output directory)
            assert open(f"{d1}/{f}", "rb").read() == open(f"{d0}/{f}", "rb").read(), f
    assert _without_columns(f"{d1}/{name}", own) == open(f"{d0}/{name}", "rb").read()
    el = pd.read_csv(f"{d1}/{name}", index_col=0)
    joint = pd.read_csv(f"{d0}/{name}", index_col=0)
    assert [c for c in el.columns if c not in joint.columns] == own
    cols = list(el.columns)
    assert cols[cols.index("n_is") + 1:cols.index("n_is") + 6] == own
    resolved = el["n_pairs_unresolved"] == 0
    assert el["n_pairs_unresolved"].dtype == np.int64 and bool((el["n_pairs_unresolved"] >= 0).all())
    for c in own[:4]:
        assert bool(np.isfinite(el[c][resolved]).all()) and bool(el[c][~resolved].isna().all()), c
    assert bool((el["is_ess_marg"][resolved] >= 1.0).all()) and bool((el["is_ess_marg"][resolved] <= 100 + 1e-9).all())
    lines = [r.getMessage() for r in caplog.records if "psis_k_marg > 0.7 on" in r.getMessage()]
    assert len(lines) == 1 and f"of {len(el)} targets" in lines[0] and "left out as unresolved" in lines[0], lines
    assert f"{int((~resolved).sum())} of {len(el)} targets" in lines[0]
