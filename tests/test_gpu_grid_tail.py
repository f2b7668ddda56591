"""The Gauss-Jacobi rule for the pairs the grid posterior's quadrature leaves out, on the GPU (bean_hip_marginal_grid_tail,
csrc/bean_jacobi.hpp): the device nodes against numpy's, pairs / lj / tail_err against the CPU rule,
bit identity with the plain call wherever no tail pair is involved, chunking, state, refusals, grid_posterior on a screen
with unedited guides against an exact posterior, and the CLI end to end.  -m gpu."""
import ctypes
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.model.grid_posterior import GRID_KEYS, TAIL_KEYS, grid_posterior
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

import grid_common as gc
import marginal_reference as mr
import tail_common as tc
import tail_reference as tr
from members_common import DEV, VAR, _assert_same, _run, _state
from oracle import elbo

pytestmark = pytest.mark.gpu
SEED = 101
LOG2 = math.log(2.0)
EFFECTS = ((0.0, 1.0), (2.0, 1.3))  # (mu_loc, exp(sd_loc)): null, strong
N_MU, N_Y = 5, 3
# (guide, alpha_pi in units of log 2, control reads zeroed): with pi_a0 of about 80 these give a' of about
# (hundreds, 0.08), (hundreds, 1.2), the mirrored case with the small exponent on pi_0, and a guide with no control
# reads at all, a' = c_p = (80, 0.08); two of them share a target
CASES = {"40": ((1, (5, -5), 1), (4, (3, -3), 1), (8, (-5, 5), 0), (12, (5, -5), None), (13, (5, -5), 1)),
         # two tiles, the second ragged: a tail pair in each, the last guide among them
         "130": ((3, (5, -5), 1), (70, (-5, 5), 0), (100, (4, -4), 1), (129, (5, -5), None))}


def _screen(which):
    data = (make_sorting_variant_screen(40, 3, seed=3) if which == "40"
            else make_sorting_variant_screen(130, 2, seed=11, mask_fraction=0.05))
    for g, _, allele in CASES[which]:
        tc.zero_control_counts(data, [g], allele)
    return data


@pytest.fixture(scope="module")
def screens():
    return {k: _screen(k) for k in CASES}


@pytest.fixture(scope="module")
def engines(screens):
    from bean_amd import engine

    cache = {}

    def get(which, family="MixtureNormal"):
        if (which, family) not in cache:
            eng = engine.HipSVI(family, screens[which].to(DEV), num_steps=50)
            assert eng.guide_order is None
            cache[(which, family)] = eng
        return cache[(which, family)]

    yield get
    for eng in cache.values():
        eng.close()


def _set(eng, name, value):
    p = eng.unconstrained[name]
    p.copy_(torch.as_tensor(value, dtype=p.dtype).reshape(p.shape).to(p.device))


def _hand_set(eng, data, which, mu_loc, sd, tail=True, seed=3):
    """alpha_pi at logs of powers of two (the float32 exp of which is the same on both sides): 0.5 ... 4 at random, and
    with ``tail`` the CASES' values on their guides."""
    g = torch.Generator().manual_seed(seed)
    T, G = data.n_targets, data.n_guides
    _set(eng, "mu_loc", torch.full((T,), float(mu_loc)))
    _set(eng, "sd_loc", torch.full((T,), math.log(sd)))
    if "alpha_pi" in eng.unconstrained:
        alpha = torch.randint(-1, 3, (G, 2), generator=g).float()
        if tail:
            for guide, powers, _ in CASES[which]:
                alpha[guide] = torch.tensor(powers).float()
        _set(eng, "alpha_pi", alpha * LOG2)


def _grid_of(data, mu_loc, sd, seed=5):
    g = torch.Generator().manual_seed(seed)
    T = data.n_targets
    r = lambda: torch.rand(T, generator=g, dtype=torch.float64)  # noqa: E731
    return (mu_loc + 0.2 * (r() - 0.5), math.log(sd) + 0.1 * (r() - 0.5), 0.02 + 0.1 * r(), 0.01 + 0.04 * r())


def _params(eng):
    return {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}


# ------------------------------------------------------------------ 1. the device nodes
@pytest.mark.parametrize("size", ["40", "130"])
def test_device_nodes_are_numpys(engines, screens, size):
    """The compact list is the reference's tail pairs in the order target, guide, replicate, with their sides; z and lw
    of the 64 + 48 nodes against numpy's eigenvalues of the Jacobi matrix, polished and weighted by the same recurrence
    (tail_reference.gauss_jacobi).  The bound on the nodes: numpy's eigenvalues carry an absolute error of a few
    Q eps ||J|| = 1e-14, two Newton steps take both sides to the root of the same recurrence up to its rounding; 1e-12
    absolute plus 1e-10 relative leaves two digits for that, and the weights - 2 Q terms in the nodes - 1e-8.  What
    binds is the comparison of the integrals (the next test).  Measured: DESIGN.md section 23."""
    data, eng = screens[size], engines(size)
    _hand_set(eng, data, size, 0.0, 1.0)
    params = _params(eng)
    got = {k: v.cpu() for k, v in eng.marginal_tail_nodes().items()}
    torch.cuda.synchronize()
    c_p = mr.model_conc(data, params)
    a_prime = mr.beta_exponents(elbo.as_float64(data), c_p)
    tail = (~mr.resolved(elbo.as_float64(data), c_p)) & data.repguide_mask
    want = [(r, g) for g in range(data.n_guides) for r in range(data.n_reps) if bool(tail[r, g])]
    assert len(want) >= len(CASES[size]) and list(zip(got["replicate"].tolist(), got["guide"].tolist())) == want
    assert got["z"].shape == (len(want), _lib.TAIL_NODES) and got["lw"].shape == got["z"].shape
    assert int(sum(mr.n_unresolved(data, params))) == len(want)
    worst = {"z_abs": 0.0, "z_rel": 0.0, "lw": 0.0}
    sides = set()
    for k, (r, g) in enumerate(want):
        a0, a1 = float(a_prime[r, g, 0]), float(a_prime[r, g, 1])
        assert int(got["side"][k]) == int(a1 <= a0)
        sides.add(int(got["side"][k]))
        for base, Q in ((0, tr.TAIL_NODES), (tr.TAIL_NODES, tr.TAIL_CHECK_NODES)):
            z, lw = tr.gauss_jacobi(max(a0, a1), min(a0, a1), Q)
            gz, glw = got["z"][k, base:base + Q].numpy(), got["lw"][k, base:base + Q].numpy()
            assert bool((np.diff(gz) > 0).all()) and gz[0] > 0 and gz[-1] < 1
            assert abs(float(np.exp(glw).sum()) - 1.0) < 1e-10
            worst["z_abs"] = max(worst["z_abs"], float(np.abs(gz - z).max()))
            worst["z_rel"] = max(worst["z_rel"], float((np.abs(gz - z) / z).max()))
            worst["lw"] = max(worst["lw"], float(np.abs(glw - lw).max()))
            assert bool((np.abs(gz - z) <= 1e-12 + 1e-10 * z).all()), (r, g, Q)
            assert bool((np.abs(glw - lw) <= 1e-8).all()), (r, g, Q)
    assert sides == {0, 1}
    print(f"{size}: {len(want)} tail pairs; device nodes against numpy: |dz| {worst['z_abs']:.2e}, |dz| / z "
          f"{worst['z_rel']:.2e}, |d lw| {worst['lw']:.2e}; smallest exponent {float(a_prime[tail].min()):.3f}, largest "
          f"{float(a_prime[tail].max()):.1f}")


# ------------------------------------------------------------------ 2. against the CPU rule
@pytest.mark.parametrize("size", ["40", "130"])
def test_pairs_lj_and_tail_err_are_the_cpu_rules(engines, screens, size):
    """pairs[i, k, r, g] and lj[i, k, t] on a 5 x 3 grid whose centres and steps differ per target against
    tail_reference.grid_terms: within 1e-9 of the summed magnitudes of their terms (the bound of
    tests/test_gpu_grid_posterior.py); tail_err[i, k, t] within the same bound on the two log integrals of each of the
    target's tail pairs.  The slots of resolved pairs are, bit for bit, those of tail_rule=False."""
    data, eng = screens[size], engines(size)
    T = data.n_targets
    worst = {"pair": 0.0, "lj": 0.0, "err": 0.0}
    for mu_loc, sd in EFFECTS:
        _hand_set(eng, data, size, mu_loc, sd)
        params = _params(eng)
        c_mu, c_y, s_mu, s_y = _grid_of(data, mu_loc, sd)
        out = eng.marginal_grid(c_mu, c_y, s_mu, s_y, N_MU, N_Y, nodes=32, pairs=True, tail_rule=True)
        plain = eng.marginal_grid(c_mu, c_y, s_mu, s_y, N_MU, N_Y, nodes=32, pairs=True)
        torch.cuda.synchronize()
        got, got_pairs, got_err = out["lj"].cpu(), out["pairs"].cpu(), out["tail_err"].cpu()
        assert got_err.shape == (N_MU, N_Y, T) and got_err.dtype == torch.float64
        assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_pairs).all()) and bool((got_err >= 0).all())
        n_un = mr.n_unresolved(data, params)
        assert out["n_unresolved"].cpu().tolist() == n_un.tolist() and torch.equal(out["n_unresolved"], plain["n_unresolved"])
        assert bool((got_err[:, :, n_un == 0] == 0).all())
        largest_err = 0.0
        for i in range(N_MU):
            for k in range(N_Y):
                mu = c_mu + (i - (N_MU - 1) / 2.0) * s_mu
                y = c_y + (k - (N_Y - 1) / 2.0) * s_y
                want = tr.grid_terms(data, params, mu, y, 32)
                tail = want["tail"]
                assert int(tail.sum()) == int(n_un.sum())
                assert torch.equal(got_pairs[i, k][~tail], plain["pairs"][i, k].cpu()[~tail])
                assert not bool((got_pairs[i, k][tail] == plain["pairs"][i, k].cpu()[tail]).any())
                dp = (got_pairs[i, k] - want["pairs"]).abs()
                dl = (got[i, k] - want["lj"]).abs()
                g2t = torch.repeat_interleave(torch.arange(T), data.target_lengths)
                err_mag = torch.zeros(T, dtype=torch.float64).index_add_(0, g2t, want["err_mag"].sum(0))
                de = (got_err[i, k] - want["tail_err"]).abs()
                worst["pair"] = max(worst["pair"], float((dp / want["pair_mag"].clamp(min=1.0)).max()))
                worst["lj"] = max(worst["lj"], float((dl / want["mag"]).max()))
                worst["err"] = max(worst["err"], float((de / err_mag.clamp(min=1.0)).max()))
                largest_err = max(largest_err, float(got_err[i, k].max()))
                assert bool((dp <= 1e-9 * want["pair_mag"]).all()), (mu_loc, i, k, float(dp.max()))
                assert bool((dl <= 1e-9 * want["mag"]).all()), (mu_loc, i, k, float(dl.max()))
                assert bool((de <= 1e-9 * err_mag).all()), (mu_loc, i, k, float(de.max()))
        print(f"{size} mu_loc {mu_loc}: largest tail_err on the grid {largest_err:.2e}")
    print(f"{size}: largest deviation, relative to the terms: pairs {worst['pair']:.2e}, lj {worst['lj']:.2e}, tail_err "
          f"{worst['err']:.2e}")


# ------------------------------------------------------------------ 3. no tail pair: the plain call, bit for bit
@pytest.mark.parametrize("family", ["MixtureNormal", "Normal"])
def test_without_tail_pairs_it_is_the_plain_call(engines, screens, family):
    data, eng = screens["130"], engines("130", family)
    _hand_set(eng, data, "130", 0.5, 1.0, tail=False)
    c_mu, c_y, s_mu, s_y = _grid_of(data, 0.5, 1.0)
    plain = eng.marginal_grid(c_mu, c_y, s_mu, s_y, N_MU, N_Y, pairs=True)
    out = eng.marginal_grid(c_mu, c_y, s_mu, s_y, N_MU, N_Y, pairs=True, tail_rule=True)
    torch.cuda.synchronize()
    assert int(out["n_unresolved"].abs().sum()) == 0
    for k in ("lj", "pairs", "n_unresolved"):
        assert torch.equal(out[k], plain[k]), k
    assert out["tail_err"].shape == (N_MU, N_Y, data.n_targets) and bool((out["tail_err"] == 0).all())
    nodes = eng.marginal_tail_nodes()
    assert nodes["z"].shape == (0, _lib.TAIL_NODES) and nodes["guide"].numel() == 0


# ------------------------------------------------------------------ 4. chunking
def test_chunks_give_the_same_bits(engines, screens):
    data, eng = screens["40"], engines("40")
    _hand_set(eng, data, "40", 0.5, 1.0)
    R, G = data.n_reps, data.n_guides
    c_mu, c_y, s_mu, s_y = _grid_of(data, 0.5, 1.0)
    for n_mu, n_y, limit in ((5, 3, 8 * R * G), (4, 6, 8 * R * G * 7), (1, 1, 8 * R * G)):
        whole = eng.marginal_grid(c_mu, c_y, s_mu, s_y, n_mu, n_y, pairs=True, tail_rule=True)
        eng.LOGW_PAIR_BYTES = limit
        try:
            chunked = eng.marginal_grid(c_mu, c_y, s_mu, s_y, n_mu, n_y, pairs=True, tail_rule=True)
        finally:
            del eng.LOGW_PAIR_BYTES
        torch.cuda.synchronize()
        assert float(whole["tail_err"].max()) > 0
        for k in ("lj", "pairs", "n_unresolved", "tail_err"):
            assert torch.equal(whole[k], chunked[k]), (n_mu, n_y, k)


# ------------------------------------------------------------------ 5. state
def test_the_fit_is_left_alone(screens):
    from bean_amd import engine

    data = screens["130"]
    c_mu, c_y, s_mu, s_y = _grid_of(data, 0.0, 1.0)
    states = []
    for with_grid in (True, False):
        eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
        _hand_set(eng, data, "130", 0.0, 1.0)
        eng.run(10, seed=SEED)
        torch.cuda.synchronize()
        if with_grid:
            before = _state(eng)
            hist = eng.loss_hist.clone()
            out = eng.marginal_grid(c_mu, c_y, s_mu, s_y, 4, 3, tail_rule=True)
            nodes = eng.marginal_tail_nodes()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(out["lj"]).all()) and int(out["n_unresolved"].sum()) > 0 and nodes["z"].shape[0] > 0
            _assert_same(_state(eng), before, "after marginal_grid(tail_rule=True)")
            assert torch.equal(eng.loss_hist, hist) and eng.steps_done == 10
        eng.run(10, seed=SEED, resume=True)
        torch.cuda.synchronize()
        states.append(_state(eng))
        eng.close()
    _assert_same(states[0], states[1], "a run after marginal_grid(tail_rule=True) against a run without it")


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_handle_usable(screens):
    from bean_amd import engine
    from bean_amd.engine import PredictiveUnsupported

    data = screens["130"]
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
    te = torch.full((N * T,), -1.0, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    nl, npair, nu = 8 * N * T, 8 * N * R * G, 4 * T
    name = "bean_hip_marginal_grid_tail"
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=50)
    _hand_set(eng, data, "130", 0.0, 1.0)
    call = lambda *a, q=32, nm=n_mu, ny=n_y: lib.bean_hip_marginal_grid_tail(  # noqa: E731
        eng._h, q, nm, ny, *[p(t) for t in arrs], *a, eng._sptr())
    good = (p(lj), nl, p(pl), npair, p(un), nu, p(te), nl)
    assert call(*good, q=20) < 0 and "16, 32 or 64" in err() and err().startswith(name + ":")
    assert call(*good, nm=65, ny=64) < 0 and "4096" in err() and "65 x 64" in err()
    assert call(p(lj), nl - 8, *good[2:]) < 0 and "lj_out" in err()
    assert call(*good[:4], p(un), nu + 4, *good[6:]) < 0 and "unresolved_out" in err()
    assert call(*good[:6], p(te), nl + 8) < 0 and "tail_err_out" in err() and str(nl) in err()
    assert call(*good[:6], None, nl) < 0 and "tail_err_out" in err()
    assert lib.bean_hip_marginal_grid_tail(None, 32, n_mu, n_y, *[p(t) for t in arrs], *good, None) < 0
    assert "null handle" in err()
    torch.cuda.synchronize()
    assert float(lj.abs().sum()) == 0 and float(pl.abs().sum()) == 0 and bool((un == -1).all()) and bool((te == -1).all())
    assert call(*good) == 0
    torch.cuda.synchronize()
    want = eng.marginal_grid(*arrs, n_mu, n_y, tail_rule=True)
    assert torch.equal(lj.reshape(n_mu, n_y, T), want["lj"]) and torch.equal(te.reshape(n_mu, n_y, T), want["tail_err"])
    count = ctypes.c_int32(-1)
    assert lib.bean_hip_marginal_tail_nodes(eng._h, 0, None, None, None, None, ctypes.byref(count), eng._sptr()) == 0
    assert count.value == int(want["n_unresolved"].sum()) > 1
    small = torch.zeros(1, dtype=torch.int32, device=DEV)
    zz = torch.zeros(_lib.TAIL_NODES, dtype=torch.float64, device=DEV)
    assert lib.bean_hip_marginal_tail_nodes(eng._h, 1, p(small), p(zz), p(zz), p(small), ctypes.byref(count),
                                            eng._sptr()) < 0
    assert "capacity 1" in err() and f"{count.value} tail pairs" in err()
    assert lib.bean_hip_marginal_tail_nodes(eng._h, 0, None, None, None, None, None, eng._sptr()) < 0 and "n_tail_out" in err()
    torch.cuda.synchronize()
    assert float(zz.abs().sum()) == 0
    eng.run(5, seed=SEED)
    torch.cuda.synchronize()
    assert np.isfinite(eng.losses()).all()
    eng.close()
    acc = make_sorting_variant_screen(130, 2, seed=11, mask_fraction=0.05, with_accessibility=True)
    other = engine.HipSVI("MixtureNormal", acc.to(DEV), num_steps=10, scale_by_accessibility=True, fit_noise=True)
    assert lib.bean_hip_marginal_grid_tail(other._h, 32, n_mu, n_y, *[p(t) for t in arrs], *good, other._sptr()) < 0
    assert err().startswith(name) and "accessibility" in err()
    with pytest.raises(PredictiveUnsupported, match="no accessibility"):
        other.marginal_grid(*arrs, n_mu, n_y, tail_rule=True)
    with pytest.raises(PredictiveUnsupported, match="no accessibility"):
        other.marginal_tail_nodes()
    other.close()


# ------------------------------------------------------------------ 7. grid_posterior on a screen with unedited guides
def test_grid_posterior_with_unedited_guides_reaches_the_exact_posterior():
    """tail_common.claim_screen_with_unedited_guides(): one guide of every target unedited.  grid_posterior's defaults
    with tail_rule=True: every target is grid_ok and passes the tail bar; without it every target is NaN.  Targets 3 and
    5 against exact_marginal_moments with the 128-node Jacobi rule inside for the tail pairs, under the bound of
    tests/test_grid_posterior_cpu.py (grid_common.assert_meets_exact) - the digits of tests/test_grid_tail_cpu.py."""
    from bean_amd import engine

    data, alpha = tc.claim_screen_with_unedited_guides()
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=10)
    for k, v in mr.claim_params(data).items():
        eng.unconstrained[k].copy_(v.reshape(eng.unconstrained[k].shape).to(DEV))
    _set(eng, "alpha_pi", alpha)
    res = {k: v.cpu() for k, v in grid_posterior(eng, tail_rule=True).items()}
    plain = {k: v.cpu() for k, v in grid_posterior(eng).items()}
    torch.cuda.synchronize()
    eng.close()
    assert bool((res["n_pairs_tail"] > 0).all()) and bool((res["n_pairs_tail"] <= data.n_reps).all())
    assert bool(res["grid_ok"].all()) and bool(res["grid_tail_ok"].all()) and bool(res["grid_null_ok"].all())
    assert not bool(plain["grid_ok"].any()) and bool(torch.isnan(plain["mu_grid"]).all())
    assert "grid_tail_err" not in plain and torch.equal(plain["n_pairs_unresolved"], res["n_pairs_tail"])
    print(f"grid_tail_err {[f'{v:.1e}' for v in res['grid_tail_err'].tolist()]} against 1e-3 per tail pair")
    c_p = mr.model_conc(data, {"alpha_pi": alpha})
    for t in (3, 5):
        idx = list(range(int(data.target_offsets[t]), int(data.target_offsets[t + 1])))
        ex = tr.exact_marginal_moments(elbo.as_float64(data[idx]), c_p[idx])
        gc.assert_meets_exact(res, t, ex, f"device, tail rule, target {t}")
        assert math.isfinite(float(res["log_bf10_grid"][t]))


# ------------------------------------------------------------------ 8. CLI
def test_cli_grid_tail_rule(tmp_path, caplog):
    """`bean run` on the fixture, 300 steps.  With --grid-tail-rule every target has finite grid columns or a reported
    reason (grid_ok 0: not settled, or the tail bar), and at least one target with unresolved pairs gets numbers;
    without it the files are those of --grid-posterior alone."""
    import logging

    caplog.set_level(logging.INFO, logger="bean_run")
    base = ["sorting", "variant", VAR, "--n-iter", "300", "--grid-posterior"]
    d1 = _run(str(tmp_path / "tail"), *base, "--grid-tail-rule")
    d0 = _run(str(tmp_path / "plain"), *base)
    name = "bean_element_result.MixtureNormal.csv"
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0))
    for f in os.listdir(d0):
        if f != name and not f.endswith(".log"):
            assert open(f"{d1}/{f}", "rb").read() == open(f"{d0}/{f}", "rb").read(), f
    el = pd.read_csv(f"{d1}/{name}", index_col=0)
    plain = pd.read_csv(f"{d0}/{name}", index_col=0)
    assert [c for c in el.columns if c not in plain.columns] == list(TAIL_KEYS)
    cols = list(el.columns)
    assert cols[cols.index("n_pairs_unresolved") + 1:][:2] == list(TAIL_KEYS)  # behind the grid columns
    assert el["n_pairs_tail"].dtype == np.int64 and el["n_pairs_tail"].tolist() == el["n_pairs_unresolved"].tolist()
    assert plain["n_pairs_unresolved"].tolist() == el["n_pairs_unresolved"].tolist()
    ok = el["grid_ok"] == 1
    for c in GRID_KEYS[:-1]:
        assert bool(np.isfinite(el[c][ok]).all()) and bool(el[c][~ok].isna().all()), c
    assert bool(np.isfinite(el["grid_tail_err"]).all())
    had = el["n_pairs_tail"] > 0
    barred = had & (el["grid_tail_err"] > 1e-3 * el["n_pairs_tail"])
    assert not bool((ok & barred).any())
    assert int((had & ok).sum()) >= 1
    # a target without tail pairs is what it was
    same = ~had
    assert plain[same].equals(el.drop(columns=list(TAIL_KEYS))[same])
    print(f"CLI: {int(had.sum())} of {len(el)} targets had tail pairs; {int((had & ok).sum())} of those have numbers; "
          f"{int(barred.sum())} refused by the tail bar; grid_tail_err {el['grid_tail_err'].tolist()}")
    lines = [r.getMessage() for r in caplog.records if "tail rule:" in r.getMessage()]
    assert len(lines) == 1 and f"{int(had.sum())} of {len(el)} targets" in lines[0] and "refused by the tail bar" in lines[0]
