"""The log joint on a grid of given (mu, log sd) per target on the GPU (bean_hip_marginal_grid, csrc/bean_grid.hpp): per
node and pair against the CPU rule, the Normal family, the tie to the shipped marginal weights, chunking, state, refusals,
grid_posterior against an exact posterior, and the CLI end to end.  -m gpu."""
import ctypes
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.grid_posterior import GRID_KEYS, grid_posterior
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

import grid_common as gc
import importance_common as ic
import marginal_reference as mr
from members_common import CONFIGS, DEV, VAR, _assert_same, _h5ad_reader_present, _kw_of, _run, _state, _without_columns  # noqa: F401
from oracle import elbo

pytestmark = pytest.mark.gpu
SEED = 101
MIXTURE = [kw for family, kw in CONFIGS if family == "MixtureNormal" and not kw.get("scale_by_accessibility")]
EFFECTS = ((0.0, 1.0), (0.5, 1.0), (2.0, 1.3))  # (mu_loc, exp(sd_loc)): null, moderate, strong
N_MU, N_Y = 5, 3


@pytest.fixture(scope="module")
def screens():
    return {"40": make_sorting_variant_screen(40, 3, seed=3),
            # two tiles, the second ragged; masked pairs and samples
            "130": make_sorting_variant_screen(130, 2, seed=11, mask_fraction=0.05)}


@pytest.fixture(scope="module")
def engines(screens):
    from bean_amd import engine

    cache = {}

    def get(which, family, kw):
        key = (which, family, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in cache:
            data = screens[which]
            cache[key] = engine.HipSVI(family, data.to(DEV), num_steps=50, **_kw_of(kw, data))
            assert cache[key].guide_order is None
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def _set(eng, name, value):
    p = eng.unconstrained[name]
    p.copy_(torch.as_tensor(value, dtype=p.dtype).reshape(p.shape).to(p.device))


def _hand_set(eng, data, mu_loc, sd, seed=3):
    """alpha_pi at logs of powers of two (0.5 ... 4: the float32 exp of its log rounds to it in any implementation within
    half an ulp, so the device and the reference form the same c_p); the target parameters only place the grid."""
    g = torch.Generator().manual_seed(seed)
    T, G = data.n_targets, data.n_guides
    _set(eng, "mu_loc", torch.full((T,), float(mu_loc)))
    _set(eng, "sd_loc", torch.full((T,), math.log(sd)))
    if "alpha_pi" in eng.unconstrained:
        _set(eng, "alpha_pi", torch.randint(-1, 3, (G, 2), generator=g).float() * math.log(2.0))


def _grid_of(data, mu_loc, sd, seed=5):
    """Centres near (mu_loc, log sd) and steps, different for every target."""
    g = torch.Generator().manual_seed(seed)
    T = data.n_targets
    r = lambda: torch.rand(T, generator=g, dtype=torch.float64)  # noqa: E731
    return (mu_loc + 0.2 * (r() - 0.5), math.log(sd) + 0.1 * (r() - 0.5), 0.02 + 0.1 * r(), 0.01 + 0.04 * r())


def _id(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items()) or "plain"


def _prior_terms(T, mu, y, prior):
    p_mu, p_sd = elbo._priors((T, 1), 0.01, prior)
    return p_mu.log_prob(mu.reshape(T, 1)).reshape(T), p_sd.log_prob(y.exp().reshape(T, 1)).reshape(T)


# ------------------------------------------------------------------ 1. per node and pair against the CPU rule
@pytest.mark.parametrize("size", ["40", "130"])
@pytest.mark.parametrize("kw", MIXTURE, ids=_id)
def test_lj_and_pairs_are_the_cpu_rules(engines, screens, kw, size):
    """lj[i, k, t] and pairs[i, k, r, g] on a 5 x 3 grid whose centres and steps differ per target, around null, moderate
    and strong effect, against tests/marginal_reference.py at the same Q (32; 16 and 64 at the moderate effect): within
    1e-9 of the summed magnitudes of the target's, the pair's terms.  Largest ratios measured: DESIGN.md section 22."""
    data, eng = screens[size], engines(size, "MixtureNormal", kw)
    okw = _kw_of(kw, data)
    prior = okw.get("prior_params")
    if prior is not None:
        prior = {k: torch.as_tensor(v).double() for k, v in prior.items()}
    T = data.n_targets
    worst_pair = worst_lj = 0.0
    for mu_loc, sd in EFFECTS:
        _hand_set(eng, data, mu_loc, sd)
        params = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
        c_mu, c_y, s_mu, s_y = _grid_of(data, mu_loc, sd)
        for Q in ((16, 32, 64) if mu_loc == 0.5 else (32,)):
            out = eng.marginal_grid(c_mu, c_y, s_mu, s_y, N_MU, N_Y, nodes=Q, pairs=True)
            torch.cuda.synchronize()
            got, got_pairs = out["lj"].cpu(), out["pairs"].cpu()
            assert got.shape == (N_MU, N_Y, T) and got_pairs.shape == (N_MU, N_Y, data.n_reps, data.n_guides)
            assert got.dtype == torch.float64 and bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_pairs).all())
            assert out["n_unresolved"].cpu().tolist() == mr.n_unresolved(data, params).tolist()
            for i in range(N_MU):
                for k in range(N_Y):
                    mu = c_mu + (i - (N_MU - 1) / 2.0) * s_mu
                    y = c_y + (k - (N_Y - 1) / 2.0) * s_y
                    want, want_pairs, mag, pair_mag = mr.marginal_log_weights(
                        data, params, mu, y, Q, use_bcmatch=okw.get("use_bcmatch", True), prior_params=prior,
                        with_target_sites=False)
                    lp_mu, lp_sd = _prior_terms(T, mu, y, prior)
                    want = want + lp_mu + lp_sd + y
                    mag = mag + lp_mu.abs() + lp_sd.abs() + y.abs()
                    assert bool((got_pairs[i, k][~data.repguide_mask] == 0).all())
                    dp = (got_pairs[i, k] - want_pairs).abs()
                    dl = (got[i, k] - want).abs()
                    worst_pair = max(worst_pair, float((dp / pair_mag.clamp(min=1.0)).max()))
                    worst_lj = max(worst_lj, float((dl / mag).max()))
                    assert bool((dp <= 1e-9 * pair_mag).all()), (mu_loc, Q, i, k, float(dp.max()))
                    assert bool((dl <= 1e-9 * mag).all()), (mu_loc, Q, i, k, float(dl.max()))
    print(f"{size} {_id(kw)}: largest deviation, relative to the terms: pairs {worst_pair:.2e}, lj {worst_lj:.2e}")


# ------------------------------------------------------------------ 2. the Normal family has no pi
@pytest.mark.parametrize("size", ["40", "130"])
@pytest.mark.parametrize("kw", [dict(), dict(use_bcmatch=False)], ids=_id)
def test_normal_family_is_the_normal_log_joint_plus_y(engines, screens, kw, size):
    """importance_common.normal_log_joint + y, target by target.  Its likelihood terms are log-probabilities, all of one
    sign, so the summed magnitudes of the terms are |log p(mu)| + |log p(sd)| + |y| + |the rest|."""
    data, eng = screens[size], engines(size, "Normal", kw)
    T = data.n_targets
    worst = 0.0
    for mu_loc, sd in EFFECTS:
        c_mu, c_y, s_mu, s_y = _grid_of(data, mu_loc, sd)
        out = eng.marginal_grid(c_mu, c_y, s_mu, s_y, N_MU, N_Y, nodes=16)
        torch.cuda.synchronize()
        got = out["lj"].cpu()
        assert out["n_unresolved"].shape == (T,) and int(out["n_unresolved"].abs().sum()) == 0
        for t in range(T):
            sub = elbo.as_float64(data[ic.target_guides(data, t)])
            MU, Y = torch.meshgrid(gc.node_coords(c_mu[t], s_mu[t], N_MU), gc.node_coords(c_y[t], s_y[t], N_Y), indexing="ij")
            mu, y = MU.reshape(-1), Y.reshape(-1)
            want = ic.normal_log_joint(sub, mu, y, use_bcmatch=kw.get("use_bcmatch", True)) + y
            p_mu, p_sd = elbo._priors((mu.numel(),), 0.01, None)
            lp_mu, lp_sd = p_mu.log_prob(mu), p_sd.log_prob(y.exp())
            mag = lp_mu.abs() + lp_sd.abs() + y.abs() + (want - lp_mu - lp_sd - y).abs()
            d = (got[:, :, t].reshape(-1) - want).abs()
            worst = max(worst, float((d / mag).max()))
            assert bool((d <= 1e-9 * mag).all()), (mu_loc, t, float(d.max()))
    with pytest.raises(ValueError, match="16, 32, 64"):
        eng.marginal_grid(c_mu, c_y, s_mu, s_y, N_MU, N_Y, nodes=20)  # n_nodes is validated all the same
    print(f"Normal {size} {_id(kw)}: largest deviation, relative to the terms: {worst:.2e}")


# ------------------------------------------------------------------ 3. the tie to the shipped marginal weights
@pytest.mark.parametrize("size", ["40", "130"])
def test_centre_node_is_the_marginal_weight_of_the_zero_draw(engines, screens, size):
    """eps_mu = eps_sd = 0 injected: the draw of bean_hip_log_weights_marginal is (mu_loc, sd_loc), and its weight less
    - log q = mu_scale_raw + sd_scale_raw + log(2 pi) + ... is the log joint; q is a density in (mu, sd), the grid's in
    (mu, y): logw_marg = lj + mu_scale_raw + sd_scale_raw + log(2 pi)."""
    data, eng = screens[size], engines(size, "MixtureNormal", {})
    _hand_set(eng, data, 0.5, 1.1)
    T = data.n_targets
    P = {k: eng.unconstrained[k].detach().double().reshape(-1) for k in ic.PER_TARGET}
    zeros = torch.zeros(T, 1, dtype=torch.float64)
    eng.set_noise({"eps_mu": zeros, "eps_sd": zeros})
    try:
        marg = eng.log_weights(0, 1, seed=SEED, pairs=True, integrate_pi=32)
    finally:
        eng.set_noise(None)
    _, _, s_mu, s_y = _grid_of(data, 0.5, 1.1)
    out = eng.marginal_grid(P["mu_loc"], P["sd_loc"], s_mu, s_y, 3, 3, nodes=32, pairs=True)
    torch.cuda.synchronize()
    assert torch.equal(marg["mu"][0], P["mu_loc"]) and torch.equal(marg["y"][0], P["sd_loc"])
    want = marg["logw"][0] - P["mu_scale"] - P["sd_scale"] - math.log(2.0 * math.pi)
    got = out["lj"][1, 1]
    # (|lj| and |pair| are no larger than the summed magnitudes of their terms: the project's bound at the least)
    d, dp = (got - want).abs(), (out["pairs"][1, 1] - marg["pairs"][0]).abs()
    print(f"{size}: centre node against logw_marg: largest |diff| {float(d.max()):.2e} of |lj| {float(got.abs().min()):.1f}; "
          f"pairs {float(dp.max()):.2e}")
    assert bool((d <= 1e-9 * got.abs()).all())
    assert bool((dp <= 1e-9 * marg["pairs"][0].abs()).all())
    assert not torch.equal(out["lj"][0, 1], got) and not torch.equal(out["lj"][1, 0], got)


# ------------------------------------------------------------------ 4. chunking
def test_chunks_give_the_same_bits(engines, screens):
    data, eng = screens["40"], engines("40", "MixtureNormal", {})
    _hand_set(eng, data, 0.5, 1.0)
    R, G = data.n_reps, data.n_guides
    c_mu, c_y, s_mu, s_y = _grid_of(data, 0.5, 1.0)
    s_mu, s_y = s_mu / 16, s_y / 16
    # (n_mu, n_y, forced LOGW_PAIR_BYTES): one node; the limit, a line of mu per call; a node per call
    for n_mu, n_y, limit in ((1, 1, 8 * R * G), (64, 64, 64 * 8 * R * G), (5, 3, 8 * R * G), (4, 6, 8 * R * G * 7)):
        whole = eng.marginal_grid(c_mu, c_y, s_mu, s_y, n_mu, n_y, pairs=True)
        eng.LOGW_PAIR_BYTES = limit
        try:
            chunked = eng.marginal_grid(c_mu, c_y, s_mu, s_y, n_mu, n_y, pairs=True)
            plain = eng.marginal_grid(c_mu, c_y, s_mu, s_y, n_mu, n_y)
        finally:
            del eng.LOGW_PAIR_BYTES
        torch.cuda.synchronize()
        assert whole["lj"].shape == (n_mu, n_y, data.n_targets) and bool(torch.isfinite(whole["lj"]).all())
        for k in ("lj", "pairs", "n_unresolved"):
            assert torch.equal(whole[k], chunked[k]), (n_mu, n_y, k)
        assert torch.equal(whole["lj"], plain["lj"]) and "pairs" not in plain
    # the chunked path's own torch work - centres converted from float32 device tensors, the line coordinates - is
    # ordered before the library's launches on the engine's stream even with the caller's stream busy
    whole = eng.marginal_grid(c_mu.float().double(), c_y.float().double(), s_mu, s_y, 6, 5)
    busy = torch.randn(4096, 4096, device=DEV)
    eng.LOGW_PAIR_BYTES = 8 * R * G * 5
    try:
        for _ in range(8):
            busy = busy @ busy * 1e-3
        chunked = eng.marginal_grid(c_mu.float().to(DEV), c_y.float().to(DEV), s_mu.to(DEV), s_y.to(DEV), 6, 5)
    finally:
        del eng.LOGW_PAIR_BYTES
    torch.cuda.synchronize()
    assert torch.equal(whole["lj"], chunked["lj"])
    one = eng.marginal_grid(c_mu, c_y, s_mu, s_y, 1, 1)["lj"]
    mid = eng.marginal_grid(c_mu, c_y, s_mu, s_y, 5, 3)["lj"]
    torch.cuda.synchronize()
    assert torch.equal(one[0, 0], mid[2, 1])  # the centre is a node of every odd grid
    with pytest.raises(ValueError, match="n_mu \\* n_y <= 4096"):
        eng.marginal_grid(c_mu, c_y, s_mu, s_y, 65, 64)
    with pytest.raises(ValueError, match="one value per target"):
        eng.marginal_grid(c_mu[:-1], c_y, s_mu, s_y, 3, 3)


# ------------------------------------------------------------------ 5. state
def test_the_fit_is_left_alone(screens):
    from bean_amd import engine

    data = screens["130"].to(DEV)
    c_mu, c_y, s_mu, s_y = _grid_of(screens["130"], 0.0, 1.0)
    states = []
    for with_grid in (True, False):
        eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
        eng.run(10, seed=SEED)
        torch.cuda.synchronize()
        if with_grid:
            before = _state(eng)
            hist = eng.loss_hist.clone()
            buffers = {k: v.clone() for k, v in eng.grads.items()}
            out = eng.marginal_grid(c_mu, c_y, s_mu, s_y, 4, 3)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["lj"]).all())
            _assert_same(_state(eng), before, "after marginal_grid")
            assert torch.equal(eng.loss_hist, hist) and eng.steps_done == 10  # (the whole buffer, beyond steps_done)
            for k, v in buffers.items():
                assert torch.equal(eng.grads[k], v), k
        eng.run(10, seed=SEED, resume=True)
        torch.cuda.synchronize()
        states.append(_state(eng))
        eng.close()
    _assert_same(states[0], states[1], "a run after marginal_grid against a run without it")


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["130"].to(DEV)
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, G, T = data.n_reps, data.n_guides, data.n_targets
    n_mu, n_y = 3, 2
    N = n_mu * n_y
    arrs = [torch.zeros(T, dtype=torch.float64, device=DEV) for _ in range(2)] + \
           [torch.full((T,), 0.1, dtype=torch.float64, device=DEV) for _ in range(2)]
    lj = torch.zeros(N * T, dtype=torch.float64, device=DEV)
    pl = torch.zeros(N * R * G, dtype=torch.float64, device=DEV)
    un = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    nl, npair, nu = 8 * N * T, 8 * N * R * G, 4 * T
    name = "bean_hip_marginal_grid"

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    call = lambda *a, q=32, nm=n_mu, ny=n_y, cs=None: lib.bean_hip_marginal_grid(  # noqa: E731
        eng._h, q, nm, ny, *(cs or [p(t) for t in arrs]), *a, eng._sptr())
    good = (p(lj), nl, p(pl), npair, p(un), nu)
    for q in (20, 0, 128):
        assert call(*good, q=q) < 0 and "n_nodes" in err() and "16, 32 or 64" in err() and err().startswith(name)
    for nm, ny in ((0, 2), (3, 0), (-1, 2), (65, 64), (4097, 1)):
        assert call(*good, nm=nm, ny=ny) < 0 and "n_mu" in err() and "n_y" in err() and "4096" in err(), (nm, ny, err())
        assert f"{nm} x {ny}" in err()
    for i in range(4):
        cs = [p(t) for t in arrs]
        cs[i] = None
        assert call(*good, cs=cs) < 0 and "null" in err() and "centre_mu" in err()
    assert call(p(lj), nl - 8, *good[2:]) < 0 and "lj_out" in err() and f"N = n_mu * n_y = {N}" in err() and str(nl) in err()
    assert call(None, nl, *good[2:]) < 0 and "lj_out" in err()
    assert call(*good[:2], p(pl), npair + 8, *good[4:]) < 0 and "pair_out" in err() and str(npair) in err()
    assert call(*good[:2], None, npair, *good[4:]) < 0 and "pair_out" in err()
    assert call(*good[:4], p(un), nu + 4) < 0 and "unresolved_out" in err() and str(nu) in err() and f"N = {N}" in err()
    assert call(*good[:4], None, 0) < 0 and "unresolved_out" in err()
    assert lib.bean_hip_marginal_grid(None, 32, n_mu, n_y, *[p(t) for t in arrs], *good, None) < 0 and "null handle" in err()
    torch.cuda.synchronize()
    assert float(lj.abs().sum()) == 0 and float(pl.abs().sum()) == 0 and bool((un == -1).all())  # nothing was launched
    assert call(*good) == 0
    torch.cuda.synchronize()
    want = eng.marginal_grid(*arrs, n_mu, n_y)
    assert torch.equal(lj.reshape(n_mu, n_y, T), want["lj"]) and torch.equal(un, want["n_unresolved"])
    # an unprepared handle of the same shape
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(eng._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_predictive_supported(h) == 1
    assert lib.bean_hip_marginal_grid(h, 32, n_mu, n_y, *[p(t) for t in arrs], *good, None) < 0
    assert err() == name + ": call bean_hip_prepare first"
    assert lib.bean_hip_destroy(h) == 0
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()

    acc = make_sorting_variant_screen(130, 2, seed=11, mask_fraction=0.05, with_accessibility=True)
    neg = make_sorting_variant_screen(900, 3, seed=32)
    neg = neg[neg.negctrl_guide_idx]
    others = (
        (engine.HipSVI("MixtureNormal", acc.to(DEV), num_steps=10, scale_by_accessibility=True, fit_noise=True),
         ("accessibility", "not 2-D"), "no accessibility"),
        (engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10),
         ("bean_hip_predictive_supported",), "MultiMixtureNormal"),
        (engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10),
         ("bean_hip_predictive_supported",), "survival"),
        (engine.HipSVI("ControlNormal", neg.to(DEV), num_steps=10), ("bean_hip_predictive_supported",), "ControlNormal"),
    )
    for other, words, match in others:
        assert lib.bean_hip_marginal_grid(other._h, 32, n_mu, n_y, *[p(t) for t in arrs], *good, other._sptr()) < 0
        assert err().startswith(name) and all(w in err() for w in words), err()
        with pytest.raises(PredictiveUnsupported, match=match):
            other.marginal_grid(*arrs, n_mu, n_y)
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()
    torch.cuda.synchronize()
    assert float(pl.abs().sum()) != 0  # (the good call above wrote it; the refused ones wrote nothing more)


# ------------------------------------------------------------------ 7. grid_posterior against the exact posterior
def test_grid_posterior_reaches_the_exact_posterior():
    """MixtureNormal on importance_common.claim_screen() with marginal_reference.claim_params (mu_loc = sd_loc = 0) and
    alpha_pi at its initial value; grid_posterior's defaults.  Targets 3, 5, 7 against claim_exact, the bound of
    tests/test_grid_posterior_cpu.py (grid_common.assert_meets_exact)."""
    from bean_amd import engine

    data = ic.claim_screen()
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=10)
    for k, v in mr.claim_params(data).items():
        eng.unconstrained[k].copy_(v.reshape(eng.unconstrained[k].shape).to(DEV))
    res = {k: v.cpu() for k, v in grid_posterior(eng).items()}
    torch.cuda.synchronize()
    eng.close()
    assert int(res["n_pairs_unresolved"].sum()) == 0
    for t in ic.CLAIM_TARGETS:
        gc.assert_meets_exact(res, t, mr.claim_exact(data, t), f"device, target {t}")
        assert math.isfinite(float(res["log_bf10_grid"][t])) and bool(res["grid_null_ok"][t])
        print(f"device, target {t}: sd_grid {float(res['sd_grid'][t]):.5f} p_mu_pos_grid {float(res['p_mu_pos_grid'][t]):.4f} "
              f"log_evidence_grid {float(res['log_evidence_grid'][t]):.4f} log_bf10_grid {float(res['log_bf10_grid'][t]):.4f}")
    print(f"grid_ok on {int(res['grid_ok'].sum())} of {data.n_targets} targets")


# ------------------------------------------------------------------ 8. CLI
def test_cli_grid_posterior(tmp_path, caplog):
    import logging

    caplog.set_level(logging.INFO, logger="bean_run")
    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    d1 = _run(str(tmp_path / "grid"), *base, "--grid-posterior", "--grid-nodes", "16")
    d0 = _run(str(tmp_path / "plain"), *base)
    own = list(GRID_KEYS) + ["n_pairs_unresolved"]
    name = "bean_element_result.MixtureNormal.csv"
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0))
    for f in os.listdir(d0):
        if f != name and not f.endswith(".log"):  # (the run's log names its output directory)
            assert open(f"{d1}/{f}", "rb").read() == open(f"{d0}/{f}", "rb").read(), f
    assert _without_columns(f"{d1}/{name}", own) == open(f"{d0}/{name}", "rb").read()
    el = pd.read_csv(f"{d1}/{name}", index_col=0)
    plain = pd.read_csv(f"{d0}/{name}", index_col=0)
    assert [c for c in el.columns if c not in plain.columns] == own
    assert el["grid_ok"].dtype == np.int64 and set(el["grid_ok"]) <= {0, 1} and el["n_pairs_unresolved"].dtype == np.int64
    out = (el["grid_ok"] == 0) | (el["n_pairs_unresolved"] > 0)
    for c in GRID_KEYS[:-1]:
        assert bool(np.isfinite(el[c][~out]).all()) and bool(el[c][out].isna().all()), c
    assert bool((el["mu_sd_grid"][~out] > 0).all()) and bool(el["p_mu_pos_grid"][~out].between(0, 1).all())
    print(f"CLI: {int(out.sum())} of {len(el)} targets not grid_ok or unresolved")
    lines = [r.getMessage() for r in caplog.records if "not grid_ok or unresolved" in r.getMessage()]
    assert len(lines) == 1 and f"{int(out.sum())} of {len(el)} targets" in lines[0] and "mu_sd / mu_sd_grid" in lines[0], lines
