"""Per-target log importance weights on the GPU (bean_hip_log_weights, csrc/bean_importance.hpp): against elbo_grad's
loss and draw, against the oracle target by target, chunking and reproducibility, the state it must leave alone, its
refusals, the claim of the check against an exact posterior, and the CLI end to end.  -m gpu."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.importance import importance_summary
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                               make_survival_variant_screen)

import importance_common as ic
from members_common import CONFIGS, DEV, VAR, _h5ad_reader_present, _kw_of, _mini, _run, _state, _without_columns  # noqa: F401

pytestmark = pytest.mark.gpu
SEED = 101


# ------------------------------------------------------------------ screens and engines, built once per module
@pytest.fixture(scope="module")
def screens(tmp_path_factory):
    kw = dict(seed=11, mask_fraction=0.05, depth_per_guide=100.0)
    return {
        # masks, a partial fourth tile, targets that cross a tile boundary (five guides per target, 64 per tile)
        "203": make_sorting_variant_screen(203, 3, **kw),
        "203acc": make_sorting_variant_screen(203, 3, with_accessibility=True, **kw),
        "mini": _mini(tmp_path_factory.mktemp("mini")),
    }


@pytest.fixture(scope="module")
def engines(screens):
    from bean_amd import engine

    cache = {}

    def get(which, family, kw):
        key = (which, family, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in cache:
            data = screens[which]
            eng = engine.HipSVI(family, data.to(DEV), num_steps=50, dump_noise=True, **_kw_of(kw, data))
            torch.manual_seed(3)
            for v in eng.unconstrained.values():  # away from the initial values, as a fit would be
                v.add_(0.3 * torch.randn_like(v))
            cache[key] = eng
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def _which(kw, mini=False):
    return "mini" if mini else ("203acc" if kw.get("scale_by_accessibility") else "203")


def _cases():
    out = [(family, kw, False) for family, kw in CONFIGS]
    out += [(family, kw, True) for family, kw in (CONFIGS[0], CONFIGS[2], CONFIGS[3])]
    return out


def _id(case):
    family, kw, mini = case
    return family + ("-" + "-".join(f"{k}={v}" for k, v in kw.items()) if kw else "") + ("-mini" if mini else "")


CASES = _cases()


# ------------------------------------------------------------------ (a) against elbo_grad
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_weights_sum_to_the_elbo_and_the_draw_is_the_elbos(engines, case):
    """For d in {0, 5}: - sum_t logw[d, t] is the loss of elbo_grad(step=d) to 1e-9 relative (the project's loss
    tolerance), and mu, y are loc + eps * scale of the noise that evaluation drew, bit for bit."""
    family, kw, mini = case
    eng = engines(_which(kw, mini), family, kw)
    assert eng.predictive_supported
    p = {k: v.detach().double() for k, v in eng.unconstrained.items()}
    for d in (0, 5):
        loss, _ = eng.elbo_grad(step=d, seed=SEED)
        noise = eng.drawn_noise()
        out = eng.log_weights(d, 1, seed=SEED, pairs=True)
        torch.cuda.synchronize()
        assert out["logw"].shape == (1, eng.T) and out["pairs"].shape == (1, eng.data.n_reps, eng.data.n_guides)
        assert out["logw"].dtype == torch.float64 and bool(torch.isfinite(out["logw"]).all())
        got = -float(out["logw"].sum())
        print(f"{_id(case)} d={d}: loss {loss:.9f}, - sum logw {got:.9f}, relative {abs(got - loss) / abs(loss):.2e}")
        assert abs(got - loss) <= 1e-9 * abs(loss)
        mu = p["mu_loc"].reshape(-1) + noise["eps_mu"].to(DEV).reshape(-1) * p["mu_scale"].reshape(-1).exp()
        y = p["sd_loc"].reshape(-1) + noise["eps_sd"].to(DEV).reshape(-1) * p["sd_scale"].reshape(-1).exp()
        assert torch.equal(out["mu"][0], mu) and torch.equal(out["y"][0], y)


# ------------------------------------------------------------------ (b) against the oracle, per target
def _targets_of(data):
    """First, last, one crossing a tile boundary (where the screen has one), one with a masked pair."""
    off = data.target_offsets.tolist()
    T = data.n_targets
    picked = [0, T - 1]
    crossing = [t for t in range(T) if off[t] // 64 != (off[t + 1] - 1) // 64]
    if data.n_guides > 64:
        assert crossing
        picked.append(crossing[0])
    masked = [t for t in range(T) if not bool(data.repguide_mask[:, off[t]:off[t + 1]].all())]
    if masked:
        picked.append(masked[len(masked) // 2])
    return picked, bool(masked)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_weights_are_the_oracles_per_target(engines, screens, case):
    """logw[d, t] against - LOSSES[family] of the screen, parameters and noise cut to target t (float64 oracle), within
    1e-9 x the sum of the magnitudes of that evaluation's site terms - once with the drawn noise, once with injected."""
    family, kw, mini = case
    which = _which(kw, mini)
    data = screens[which]
    eng = engines(which, family, kw)
    okw = _kw_of(kw, data)
    targets, has_masked = _targets_of(data)
    assert has_masked or mini
    params = {k: v.detach().cpu() for k, v in eng.unconstrained.items()}

    def check(logw, noise, what):
        for t in targets:
            want, mag = ic.oracle_logw(family, data, params, noise, t, okw)
            got = float(logw[t])
            print(f"{_id(case)} {what} target {t}: logw {got:.9f}, oracle {want:.9f}, |diff| {abs(got - want):.2e}, "
                  f"bound {1e-9 * mag:.2e}")
            assert abs(got - want) <= 1e-9 * mag, (what, t)

    d = 5
    eng.elbo_grad(step=d, seed=SEED)
    noise = {k: v.cpu() for k, v in eng.drawn_noise().items()}
    out = eng.log_weights(d, 1, seed=SEED)
    check(out["logw"][0].cpu(), noise, "drawn")
    g = torch.Generator().manual_seed(9)
    given = {k: (torch.randn(v.shape, generator=g, dtype=torch.float64) if k != "pi" else None) for k, v in noise.items()}
    if "pi" in noise:
        p1 = 0.05 + 0.9 * torch.rand(noise["pi"].shape[:-1], generator=g, dtype=torch.float64)
        given["pi"] = torch.stack([1 - p1, p1], -1)
    eng.set_noise(given)
    try:
        out = eng.log_weights(d + 1, 3, seed=SEED)
        torch.cuda.synchronize()
    finally:
        eng.set_noise(None)
    check(out["logw"][0].cpu(), given, "injected")
    # injected noise: every draw of the call is the same draw
    assert torch.equal(out["logw"][0], out["logw"][1]) and torch.equal(out["logw"][0], out["logw"][2])
    assert torch.equal(out["mu"][0], out["mu"][2])


# ------------------------------------------------------------------ (c) chunking and reproducibility
@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[9]], ids=_id)
def test_chunking_and_reproducibility(engines, case):
    family, kw, mini = case
    eng = engines(_which(kw, mini), family, kw)
    whole = eng.log_weights(2, 7, seed=SEED, pairs=True)
    a, b = eng.log_weights(2, 3, seed=SEED, pairs=True), eng.log_weights(5, 4, seed=SEED, pairs=True)
    again = eng.log_weights(2, 7, seed=SEED, pairs=True)
    other_seed = eng.log_weights(2, 7, seed=SEED + 1)
    other_draw = eng.log_weights(3, 7, seed=SEED)
    # the engine's own chunks (here: two draws per library call)
    R, G = eng.data.n_reps, eng.data.n_guides
    eng.LOGW_PAIR_BYTES = 2 * 8 * R * G
    try:
        chunked = eng.log_weights(2, 7, seed=SEED, pairs=True)
    finally:
        del eng.LOGW_PAIR_BYTES
    torch.cuda.synchronize()
    for k in ("logw", "mu", "y", "pairs"):
        assert torch.equal(whole[k], torch.cat([a[k], b[k]])), k
        assert torch.equal(whole[k], again[k]) and torch.equal(whole[k], chunked[k]), k
    for k in ("logw", "mu", "y"):
        assert not torch.equal(whole[k], other_seed[k]) and not torch.equal(whole[k], other_draw[k]), k
        assert torch.equal(whole[k][1:], other_draw[k][:-1]), k  # draw d is draw d
    assert not bool((whole["logw"][0] == whole["logw"][1]).all())
    with pytest.raises(ValueError, match="at least 1"):
        eng.log_weights(0, 0)


# ------------------------------------------------------------------ (d) state untouched, refusals
def test_log_weights_leave_the_fit_alone(screens):
    from bean_amd import engine

    data = screens["203"].to(DEV)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(20, seed=SEED)
    torch.cuda.synchronize()
    before = _state(eng)
    grads = {k: v.clone() for k, v in eng.grads.items()}
    hist = eng.loss_hist.clone()
    eng.log_weights(2, 5, seed=7)
    torch.cuda.synchronize()
    after = _state(eng)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    for k in grads:
        assert torch.equal(grads[k], eng.grads[k]), k
    assert torch.equal(hist, eng.loss_hist)
    eng.close()

    def fit(weights_first, resume):
        e = engine.HipSVI("MixtureNormal", data, num_steps=300)
        if resume:
            e.run(10, seed=SEED, resume=True)
        if weights_first == "raw":
            # the library call alone, behind the engine's back: the handle itself must not continue the window
            T, R, G = e.T, data.n_reps, data.n_guides
            lw, mu = (torch.empty(T, dtype=torch.float64, device=DEV) for _ in range(2))
            pl = torch.empty(R * G, dtype=torch.float64, device=DEV)
            p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            assert e.lib.bean_hip_log_weights(e._h, SEED + 5, 1, 1, p(lw), 8 * T, p(mu), 8 * T, None, 0, p(pl), 8 * R * G,
                                              e._sptr()) == 0
        elif weights_first:
            e.log_weights(1, 2, seed=SEED + 5)
        e.run(40, seed=SEED, resume=resume)
        torch.cuda.synchronize()
        st = _state(e)
        e.close()
        return st

    plain, weighted = fit(False, False), fit(True, False)
    for k in plain:
        assert torch.equal(plain[k], weighted[k]), k
    plain = fit(False, True)
    for how in (True, "raw"):
        weighted = fit(how, True)
        for k in plain:
            assert torch.equal(plain[k], weighted[k]), (how, k)


def test_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["203"].to(DEV)
    lib = _lib.load()
    err = lambda: lib.bean_hip_last_error().decode()  # noqa: E731
    R, G, T = data.n_reps, data.n_guides, data.n_targets
    S = 3
    lw, mu, y = (torch.zeros(S * T, dtype=torch.float64, device=DEV) for _ in range(3))
    pl = torch.zeros(S * R * G, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    nt, npair = 8 * S * T, 8 * S * R * G

    eng = engine.HipSVI("MixtureNormal", data, num_steps=50)
    call = lambda *a, n=S: lib.bean_hip_log_weights(eng._h, SEED, 0, n, *a, eng._sptr())  # noqa: E731
    assert call(p(lw), nt - 8, p(mu), nt, p(y), nt, p(pl), npair) < 0 and "logw_out" in err()
    assert call(None, 0, p(mu), nt, p(y), nt, p(pl), npair) < 0 and "logw_out" in err()
    assert call(p(lw), nt, p(mu), nt + 8, p(y), nt, p(pl), npair) < 0 and "mu_out" in err()
    assert call(p(lw), nt, None, 0, p(y), nt, p(pl), npair) < 0 and "mu_out" in err()
    assert call(p(lw), nt, p(mu), nt, p(y), nt - 8, p(pl), npair) < 0 and "y_out" in err()
    assert call(p(lw), nt, p(mu), nt, None, 8, p(pl), npair) < 0 and "y_out" in err()
    assert call(p(lw), nt, p(mu), nt, p(y), nt, p(pl), npair - 8) < 0 and "pair_out" in err()
    assert call(p(lw), nt, p(mu), nt, p(y), nt, None, 0) < 0 and "pair_out" in err() and "scratch" in err()
    for n in (0, -1, _lib.MAX_LOGW_DRAWS + 1):
        assert call(p(lw), nt, p(mu), nt, p(y), nt, p(pl), npair, n=n) < 0 and "n_draws" in err() and "4096" in err()
    assert lib.bean_hip_log_weights(None, SEED, 0, S, p(lw), nt, p(mu), nt, None, 0, p(pl), npair, None) < 0
    assert "null handle" in err()
    assert float(lw.abs().sum()) == 0 and float(pl.abs().sum()) == 0  # nothing was launched
    assert call(p(lw), nt, p(mu), nt, None, 0, p(pl), npair) == 0      # y_out is optional
    assert call(p(lw), nt, p(mu), nt, p(y), nt, p(pl), npair) == 0
    torch.cuda.synchronize()
    want = eng.log_weights(0, S, seed=SEED)
    assert torch.equal(lw.reshape(S, T), want["logw"]) and torch.equal(y.reshape(S, T), want["y"])
    # an unprepared handle of the same shape
    h = ctypes.c_void_p()
    assert lib.bean_hip_create(ctypes.byref(eng._shape), ctypes.byref(h)) == 0
    assert lib.bean_hip_predictive_supported(h) == 1
    assert lib.bean_hip_log_weights(h, SEED, 0, S, p(lw), nt, p(mu), nt, None, 0, p(pl), npair, None) < 0
    assert "bean_hip_prepare" in err()
    assert lib.bean_hip_destroy(h) == 0
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()

    for extra in (dict(n_members=2), dict(n_particles=2)):
        many = engine.HipSVI("MixtureNormal", data, num_steps=50, **extra)
        assert lib.bean_hip_log_weights(many._h, SEED, 0, S, p(lw), nt, p(mu), nt, None, 0, p(pl), npair, many._sptr()) < 0
        assert "bean_hip_predictive_supported" in err()
        with pytest.raises(PredictiveUnsupported):
            many.log_weights(0, 2)
        if "n_members" in extra:
            many.run_ensemble(5, [1, 2])
        else:
            many.run_particles(5, SEED)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(many.loss_hist[..., :5]).all())
        many.close()

    for other in (engine.HipSVI("MultiMixtureNormal", make_sorting_tiling_screen(200, 2, seed=2).to(DEV), num_steps=10),
                  engine.HipSVI("MixtureNormal", make_survival_variant_screen(200, 2, seed=2).to(DEV), num_steps=10)):
        with pytest.raises(PredictiveUnsupported, match=other.family):
            other.log_weights(0, 2)
        other.run(5, seed=SEED)
        torch.cuda.synchronize()
        assert np.isfinite(other.losses()).all()
        other.close()


# ------------------------------------------------------------------ (e) the check does what it claims
def test_check_recovers_the_exact_posterior():
    """Normal family, 40 guides x 3 replicates (8 targets), parameters set by hand: mu_loc = 0, mu_scale 0.06, sd_loc = 0,
    sd_scale 0.04 (importance_common.CLAIM_*), S = 4096.  On the three null targets 3, 5, 7 the exact E[mu | x] and
    sd[mu | x] come from 2-D quadrature of the oracle's one-target log joint over (mu, log sd) (grid border < 1e-6 of
    the peak); |mu_is - E| <= 4 sd / sqrt(is_ess) is asserted on every one with psis_k < 0.7, and at least two must
    qualify.  Screen seed and scales were chosen so that the oracle alone, drawing from the same q on the CPU, meets the
    cap - checked by tests/test_importance_cpu.py::test_the_claim_holds_for_the_oracle_alone (there: psis_k -0.64, -0.05,
    -0.47; is_ess 258, 140, 184; |mu_is - E| 0.0004, 0.0004, 0.00003 against caps of 0.0037, 0.0050, 0.0041)."""
    from bean_amd import engine

    data = ic.claim_screen()
    eng = engine.HipSVI("Normal", data.to(DEV), num_steps=10)
    for k, v in ic.claim_params(data).items():
        eng.unconstrained[k].copy_(v.reshape(eng.unconstrained[k].shape).to(DEV))
    out = eng.log_weights(0, ic.CLAIM_DRAWS, seed=SEED)
    summary = {k: v.cpu() for k, v in importance_summary(out["logw"], out["mu"]).items()}
    eng.close()
    assert summary["n_is"].tolist() == [float(ic.CLAIM_DRAWS)] * data.n_targets
    ic.assert_claim(summary, data, "device")


# ------------------------------------------------------------------ (f) CLI
def test_cli_importance_check(tmp_path, capsys, caplog):
    import logging

    from bean_amd.cli.execute import main as bean_main

    caplog.set_level(logging.INFO, logger="bean_run")

    base = ["sorting", "variant", VAR, "--n-iter", "200"]
    S = 100
    d1 = _run(str(tmp_path / "is"), *base, "--importance-check", str(S))
    d0 = _run(str(tmp_path / "plain"), *base)
    own = ["psis_k", "mu_is", "mu_sd_is", "is_ess", "n_is"]
    name = "bean_element_result.MixtureNormal.csv"
    sg = "bean_sgRNA_result.MixtureNormal.csv"
    assert open(f"{d1}/{sg}", "rb").read() == open(f"{d0}/{sg}", "rb").read()
    assert _without_columns(f"{d1}/{name}", own) == open(f"{d0}/{name}", "rb").read()
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0))  # no further file
    el = pd.read_csv(f"{d1}/{name}", index_col=0)
    plain = pd.read_csv(f"{d0}/{name}", index_col=0)
    assert [c for c in el.columns if c not in plain.columns] == own
    assert bool((el["n_is"] == S).all())
    for c in ("mu_is", "mu_sd_is", "is_ess"):
        assert bool(np.isfinite(el[c]).all()), c
    assert bool(np.isfinite(el["psis_k"]).all())
    assert bool((el["is_ess"] >= 1.0).all()) and bool((el["is_ess"] <= S + 1e-9).all()) and bool((el["mu_sd_is"] >= 0).all())
    lines = [r.getMessage() for r in caplog.records if "psis_k > 0.7 on" in r.getMessage()]
    assert len(lines) == 1 and f"of {len(el)} targets" in lines[0], lines
    til = os.path.join(os.path.dirname(VAR), "tiling_mini_screen.h5ad")
    with pytest.raises(SystemExit) as exc:
        bean_main(["run", "sorting", "tiling", til, "--importance-check", "50", "-o", str(tmp_path / "til")])
    assert exc.value.code == 2
    msg = capsys.readouterr().err
    assert "--importance-check" in msg and "tiling" in msg and "MultiMixtureNormal" in msg
