"""The device's random draws against their host replay (``philox_reference.py``), element by element.  -m gpu.

The generator is counter based: the host recomputes the very draw the device exported from (seed, site, element, step)
alone.  A wrong word, key, stride or a truncated offset moves a draw by O(1); the tolerances here are ~1e-5.

* words: ``bean_hip_test_special`` op 25 returns the raw Philox block; bit-equal to ``block()``;
* the pair sampler, op level (ops 12 - 14, 18 - 20, 4, 6, 8): generator position equal and each value within its
  tolerance for every element the reference does not flag as undecided (at most 1e-4 of a case);
* the fit's draws: ``elbo_grad(step, seed)`` with ``dump_noise=True`` against the per-site replay;
* the other sites, one small case each, and one shard against the replay of the whole screen's keys.

Tolerances: words and positions exact; a float32 Box-Muller normal ``K 2^-24 max(1, radius)`` (``K_ROCRAND`` /
``K_GAMMA``, measured: every test prints its worst ratio in units of ``2^-24 max(1, radius)``); a gamma or pi value its
first-order sensitivity to that bound plus 1e-13 relative (and four float64 subnormal steps, where a value underflows).

Parameters whose exponential enters a concentration are set to values whose ``expf`` is settled in float32
(``settled_log``): the replay then takes the concentration from the parameter without depending on the device's
``expf``, and the rest of the concentration is formed in the order the kernels form it.
"""
import functools

import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
import philox_reference as pr
from bean_amd import parallel
from bean_amd.preprocessing.synthetic import (make_sorting_tiling_screen, make_sorting_variant_screen,
                                              make_survival_variant_screen)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_OP = pr.OP_N
SEED64 = pr.OP_SEED
SEEDS = (101, SEED64)
STEPS = (0, 1, 2 ** 26 + 5)  # the last: the pi offset exceeds 32 bits, the block counter's high word is not zero
MAX_UNDECIDED = 1e-4
SUBNORMAL = 4 * 5e-324
FLOOR_VALUE = {0: 0.0, 1: pr.FLT_MIN, 2: pr.DBL_MIN}
SHAPE_PAIRS = pr.OP_SHAPE_PAIRS
EXPORT_PAIRS = pr.OP_EXPORT_PAIRS


@pytest.fixture(scope="module")
def engine():
    from bean_amd import engine as eng

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return eng


def _as_f64(bits):
    return np.ascontiguousarray(np.asarray(bits, dtype=np.uint64)).view(np.float64)


def _seed_array(seed, n):
    x = np.zeros(n, np.uint64)
    x[0] = np.uint64(seed)
    return _as_f64(x)


def _words(engine, seed, sub, offset):
    """op 25: the device's block at (seed, sub[i], offset[i]) as four uint64 arrays of 32-bit words."""
    sub, offset = np.asarray(sub, np.uint64), np.asarray(offset, np.uint64)
    o0, o1 = engine.test_special(25, _as_f64(sub), _seed_array(seed, sub.size), _as_f64(offset))
    o0, o1 = o0.cpu().numpy().view(np.uint64), o1.cpu().numpy().view(np.uint64)
    return o0 & pr.M32, o0 >> np.uint64(32), o1 & pr.M32, o1 >> np.uint64(32)


def _assert_words(engine, seed, sub, offset):
    dev = _words(engine, seed, sub, offset)
    ref = pr.block(seed, sub, offset)
    for name, d, r in zip("xyzw", dev, ref):
        bad = np.nonzero(d != np.broadcast_to(r, d.shape))[0]
        assert bad.size == 0, (name, bad[:5], [hex(int(v)) for v in d[bad[:5]]])
    return dev


# ------------------------------------------------------------------------------------------------------- 1. words
def test_bit_patterns_pass_through_the_hook(engine):
    """Seeds, subsequences and offsets that are NaNs as doubles - quiet, signalling, with a payload, either sign - must
    reach the kernel bit for bit, and outputs that are NaN patterns must come back bit for bit: one canonicalised NaN
    changes a key or a counter, and with it all four words."""
    nans = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FF4000000000000, 0xFFFFFFFFFFFFFFFF,
                     0x7FFFFFFFFFFFFFFC, 0xFFF8000000000001, 0x7FF00000DEADBEEF], np.uint64)
    assert np.isnan(nans.view(np.float64)).all()
    sub = np.repeat(nans, nans.size)
    off = np.tile(nans & ~np.uint64(3), nans.size)
    for seed in (0xFFFFFFFFFFFFFFFF, 0x7FF0000000000001):
        _assert_words(engine, seed, sub, off)
    # outputs: of 2^16 blocks, ~64 have an (x, y) and ~64 a (z, w) that is a NaN as a double
    sub = pr.subsequence(pr.SITE_PI, np.arange(N_OP))
    x, y, z, w = _assert_words(engine, SEED64, sub, np.zeros(N_OP, np.uint64))
    n_nan = int(np.isnan(((y << np.uint64(32)) | x).view(np.float64)).sum() + np.isnan(((w << np.uint64(32)) | z).view(np.float64)).sum())
    print(f"NaN patterns among the outputs: {n_nan}")
    assert n_nan > 20


def test_words_at_the_known_answer_vectors(engine):
    """Random123's philox4x32-10 vectors through op 25.  The hook takes the block counter as a word offset
    (counter = offset >> 2), so a counter's top two bits cannot be set: the first vector is reached exactly; the second
    and third are taken with bits 30, 31 of their second counter word cleared and compared with ``philox4x32_10``,
    which ``test_philox_reference.py`` holds to all three vectors as published."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, None),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), None)]
    for (c0, c1, c2, c3), (k0, k1), out in kat:
        c1 &= 0x3FFFFFFF
        seed, sub, off = (k1 << 32) | k0, (c3 << 32) | c2, ((c1 << 32) | c0) << 2
        dev = _words(engine, seed, np.array([sub], np.uint64), np.array([off], np.uint64))
        ref = pr.philox4x32_10((c0, c1, c2, c3), (k0, k1))
        got = tuple(int(v[0]) for v in dev)
        assert got == tuple(int(v) for v in ref), [hex(v) for v in got]
        if out is not None:
            assert got == out


def test_words_at_random_keys(engine):
    """2^16 random (seed, subsequence, offset): offsets multiples of 4 up to 2^40, subsequences with the site bits set,
    seeds with a non-zero high half (the seed is one per launch: 16 launches of 2^12)."""
    rng = np.random.default_rng(25)
    for _ in range(16):
        n = N_OP // 16
        seed = int(rng.integers(1 << 32, 1 << 63)) | (1 << 63 if rng.random() < 0.5 else 0)
        site = rng.integers(1, 9, n).astype(np.uint64)
        sub = (site << np.uint64(48)) + rng.integers(0, 1 << 48, n).astype(np.uint64)
        off = rng.integers(0, (1 << 38) + 1, n).astype(np.uint64) * np.uint64(4)
        off[:2] = (0, 1 << 40)
        _assert_words(engine, seed, sub, off)


# ------------------------------------------------------------------------------------------- 2. the sampler, op level
def _pair_reference(site, a0, a1, floor):
    return pr.op_case(site, a0, a1, floor)


def _worst_ratio(dev, ref, tol, keep):
    """max |dev - ref| / tol over `keep`, and the same in units of 2^-24 max(1, radius) (the tolerance is K_GAMMA of
    those, to first order)."""
    err = np.abs(dev - ref)[keep]
    t = tol[keep] + SUBNORMAL
    r = float((err / t).max()) if err.size else 0.0
    return r, r * pr.K_GAMMA


@pytest.mark.parametrize("floor", [0, 1, 2])
@pytest.mark.parametrize("a0,a1", SHAPE_PAIRS)
def test_pair_sampler_values_and_positions(engine, a0, a1, floor):
    """Ops 12 - 14 (values, unfloored) and 18 - 20 (generator position) of the inlined sampler, FLOOR 0, 1, 2, at
    (seed, kSiteAux, element i, offset 0).  A FLOOR form's value is compared after its caller's floor (a component the
    shortcut took returns 0 or its underflowed boost factor, "0 stands for it")."""
    g0, g1, k, und, t0, t1 = _pair_reference(pr.SITE_AUX, a0, a1, floor)
    A, B = np.full(N_OP, a0), np.full(N_OP, a1)
    seed = _seed_array(SEED64, N_OP)
    d0, d1 = (t.cpu().numpy() for t in engine.test_special(12 + floor, A, seed, B))
    dk = engine.test_special(18 + floor, A, seed, B)[0].cpu().numpy()
    keep = ~und
    fl = FLOOR_VALUE[floor]
    r0, k0 = _worst_ratio(np.maximum(d0, fl), np.maximum(g0, fl), t0, keep)
    r1, k1 = _worst_ratio(np.maximum(d1, fl), np.maximum(g1, fl), t1, keep)
    print(f"({a0}, {a1}) FLOOR {floor}: undecided {und.mean():.2e}, positions differ in {int((dk != k)[keep].sum())} "
          f"(max {int(k.max())}), worst |dev - ref| / tol {max(r0, r1):.3g} = {max(k0, k1):.3g} x 2^-24 max(1, radius)")
    assert und.mean() <= MAX_UNDECIDED
    assert np.array_equal(dk[keep], k[keep].astype(np.float64))
    assert max(r0, r1) <= 1.0


@pytest.mark.parametrize("a0,a1", EXPORT_PAIRS)
def test_pair_sampler_exports(engine, a0, a1):
    """Op 4 (the clamped Dirichlet pair, kSiteAux), op 6 (float32 gammas floored at FLT_MIN, kSiteQ0) and op 8 (gammas
    floored at DBL_MIN, kSitePi), all from the plain sampler."""
    A, B = np.full(N_OP, a0), np.full(N_OP, a1)
    seed = _seed_array(SEED64, N_OP)
    worst = {}
    for op, site in ((4, pr.SITE_AUX), (6, pr.SITE_Q0), (8, pr.SITE_PI)):
        g0, g1, k, und, t0, t1 = _pair_reference(site, a0, a1, 0)
        assert und.mean() <= MAX_UNDECIDED
        if op == 4:
            g0, g1 = np.maximum(g0, pr.DBL_MIN), np.maximum(g1, pr.DBL_MIN)
            s = g0 + g1
            tt = (g1 * t0 + g0 * t1) / (s * s)
            g0, g1 = np.clip(g0 / s, pr.DBL_MIN, pr.ONE_MINUS), np.clip(g1 / s, pr.DBL_MIN, pr.ONE_MINUS)
            t0, t1 = tt + 1e-13 * g0, tt + 1e-13 * g1
        elif op == 6:
            g0, g1 = (np.maximum(g.astype(np.float32), np.float32(pr.FLT_MIN)).astype(np.float64) for g in (g0, g1))
            t0, t1 = t0 + 2.0 ** -23 * g0, t1 + 2.0 ** -23 * g1  # the float32 rounding may fall to the other side
        else:
            g0, g1 = np.maximum(g0, pr.DBL_MIN), np.maximum(g1, pr.DBL_MIN)
        d0, d1 = (t.cpu().numpy() for t in engine.test_special(op, A, seed, B))
        worst[op] = max(_worst_ratio(d0, g0, t0, ~und)[0], _worst_ratio(d1, g1, t1, ~und)[0])
    print(f"({a0}, {a1}): worst |dev - ref| / tol, ops 4, 6, 8: " + ", ".join(f"{v:.3g}" for v in worst.values()))
    assert max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------- 3. the fit's draws
def _normal_ratio(dev, ref, rad):
    return float((np.abs(dev - ref) / pr.normal_bound(1.0, rad)).max())


def _spread_alpha(G, A, seed):
    """(G, A) alpha_pi parameters and their settled exponentials, log-uniform over 1e-7 ... 50: with pi_a0 of a few
    units that gives concentrations above and below 1 and below the guide's 1e-5 clamp."""
    rng = np.random.default_rng(seed)
    la = rng.uniform(np.log(1e-7), np.log(50.0), (G, A))
    la = np.where(np.abs(la) < 0.5, la + 1.0, la)
    return pr.settled_log(np.exp(la))


def _pair_conc(alpha, pa0):
    """The guide-side concentrations of the variant families as the kernels form them: alpha pa0 / sum, clamped."""
    rs = (1.0 / (alpha[:, 0] + alpha[:, 1])) * pa0
    return np.maximum(alpha * rs[:, None], 1e-5)


def _screen130(with_acc):
    data = make_sorting_variant_screen(130, 2, seed=81, with_accessibility=with_acc)
    data.repguide_mask[1, 7] = False  # one masked (replicate, guide)
    return data


@functools.lru_cache(maxsize=None)
def _whole_screen_pi(seed, step):
    """The replay of the 130 x 2 screen's pi draws (the same alpha_pi in every test that uses them)."""
    data = _screen130(False)
    _, alpha = _spread_alpha(130, 2, 3)
    return pr.pi_pair_screen(seed, step, _pair_conc(alpha, data.pi_a0.numpy().astype(np.float64)), 2, K=pr.K_GAMMA)


def _check_pi(dev, ref, what):
    pi, k, und, tol = ref
    keep = np.broadcast_to(~und[..., None] if und.ndim < pi.ndim else ~und, pi.shape)
    ratio = float((np.abs(dev - pi)[keep] / (tol[keep] + SUBNORMAL)).max())
    print(f"{what}: pi worst |dev - ref| / tol {ratio:.3g} ({ratio * pr.K_GAMMA:.3g} x 2^-24 max(1, radius)), "
          f"undecided {int(und.sum())} of {und.size}, max position {int(k.max())}")
    assert int(k.max()) <= pr.MAX_ROUNDS
    assert int(und.sum()) <= max(1, int(MAX_UNDECIDED * und.size))
    assert ratio <= 1.0, what
    return ratio


@pytest.mark.parametrize("model", ["Normal", "MixtureNormal", "MixtureNormal+acc"])
def test_fit_draws_of_the_sorting_screen(engine, model):
    """130 guides x 2 replicates (two ragged tiles), seeds 101 and a 64-bit one, steps 0, 1 and 2^26 + 5: eps_mu, eps_sd,
    eps_noise and pi of ``elbo_grad(step, seed)``.  The masked (replicate, guide) (1, 7) exports its draw like every
    other pair (the mask acts on the likelihood)."""
    acc = model.endswith("+acc")
    family = model.split("+")[0]
    data = _screen130(acc)
    kw = dict(scale_by_accessibility=True) if acc else {}
    eng = engine.HipSVI(family, data.to(DEV), dump_noise=True, num_steps=50, **kw)
    T, G, R = eng.T, 130, 2
    assert T == 26
    if family == "MixtureNormal":
        p, alpha = _spread_alpha(G, 2, 3)
        eng.unconstrained["alpha_pi"].copy_(torch.as_tensor(p))
        conc = _pair_conc(alpha, data.pi_a0.numpy().astype(np.float64))
        assert (conc < 1.0).any() and (conc > 1.0).any() and (conc == 1e-5).any()
    worst_n, worst_pi = 0.0, 0.0
    for seed in SEEDS:
        for step in STEPS:
            eng.elbo_grad(step=step, seed=seed)
            d = {k: v.cpu().numpy() for k, v in eng.drawn_noise().items()}
            mu, sd, rad = pr.target_draws(seed, step, T)
            worst_n = max(worst_n, _normal_ratio(d["eps_mu"].reshape(-1), mu, rad),
                          _normal_ratio(d["eps_sd"].reshape(-1), sd, rad))
            if acc:
                en, rad = pr.noise_draws(seed, step, G)
                worst_n = max(worst_n, _normal_ratio(d["eps_noise"], en, rad))
            if family == "MixtureNormal":
                ref = pr.pi_pair_screen(seed, step, conc, R, K=pr.K_GAMMA) if acc else _whole_screen_pi(seed, step)
                worst_pi = max(worst_pi, _check_pi(d["pi"][:, 0], ref, f"{model} seed {seed:#x} step {step}"))
            else:
                assert "pi" not in d
    eng.close()
    print(f"{model}: normals worst {worst_n:.3g} x 2^-24 max(1, radius) (K_ROCRAND {pr.K_ROCRAND:g})")
    assert worst_n <= pr.K_ROCRAND


# ------------------------------------------------------------------------------------------------ 4. the other sites
def test_one_shard_draws_the_whole_screens_keys(engine):
    """The second of two target-aligned shards of the 130 x 2 screen (guides 65 ..., not a tile boundary), built as
    test_sharded_engines_reproduce_the_whole_screen_fit builds it: its draws are the whole screen's replay at its
    guides and targets - "independent of the number of GPUs" against the host, not against a second device run."""
    data = _screen130(False)
    shards = parallel.plan_shards(data.target_lengths.numpy(), 2)
    g0, g1, t0, t1 = shards[1]
    assert g0 % 64 and g1 == 130
    eng = engine.HipSVI("MixtureNormal", parallel.shard_screen(data, shards[1]).to(DEV), dump_noise=True, num_steps=50,
                        guide_offset=g0, target_offset=t0, n_guides_total=130)
    p, _ = _spread_alpha(130, 2, 3)
    eng.unconstrained["alpha_pi"].copy_(torch.as_tensor(p[g0:g1]))
    worst = 0.0
    for seed, step in ((101, 1), (SEED64, 2 ** 26 + 5)):
        eng.elbo_grad(step=step, seed=seed)
        d = {k: v.cpu().numpy() for k, v in eng.drawn_noise().items()}
        mu, sd, rad = pr.target_draws(seed, step, 26)
        worst = max(worst, _normal_ratio(d["eps_mu"].reshape(-1), mu[t0:t1], rad[t0:t1]),
                    _normal_ratio(d["eps_sd"].reshape(-1), sd[t0:t1], rad[t0:t1]))
        pi, k, und, tol = _whole_screen_pi(seed, step)
        _check_pi(d["pi"][:, 0], (pi[:, g0:g1], k[:, g0:g1], und[:, g0:g1], tol[:, g0:g1]), f"shard seed {seed:#x} step {step}")
    eng.close()
    print(f"shard: normals worst {worst:.3g} x 2^-24 max(1, radius)")
    assert worst <= pr.K_ROCRAND


def test_survival_screen_q0_and_baseline_draws(engine):
    """Survival MixtureNormal 130 x 2: ``mu_negctrl`` (kSiteAux), ``eps_mu``, ``pi``, and ``initial_abundance``: the
    export is the float32-floored gamma over its replicate's total (float32, clamped); the total is read from the
    exchange buffer's normaliser and itself held to the replayed gammas' sum."""
    data = make_survival_variant_screen(130, 2, seed=41)
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), dump_noise=True, num_steps=50)
    G, R = 130, 2
    rng = np.random.default_rng(5)
    q = np.exp(rng.uniform(np.log(1e-3), np.log(5.0), G))
    q = np.where(np.abs(np.log(q)) < 0.5, 3.0, q)
    p, conc_q = pr.settled_log(q)
    eng.unconstrained["q0"].copy_(torch.as_tensor(p))
    pa, alpha = _spread_alpha(G, 2, 9)
    eng.unconstrained["alpha_pi"].copy_(torch.as_tensor(pa))
    conc = _pair_conc(alpha, data.pi_a0.numpy().astype(np.float64))
    gsum = eng.exchange_buffers()["gsum"]
    m0, s0 = float(np.float32(0.0)), float(np.float32(0.1))
    worst_n = worst_g = 0.0
    for seed, step in ((101, 0), (SEED64, 2 ** 26 + 5)):
        eng.elbo_grad(step=step, seed=seed)
        d = {k: v.cpu().numpy() for k, v in eng.drawn_noise().items()}
        tot = gsum.cpu().numpy()[:R]
        mu, _, rad = pr.target_draws(seed, step, eng.T)
        worst_n = max(worst_n, _normal_ratio(d["eps_mu"].reshape(-1), mu, rad))
        eu, rad = pr.aux_draws(seed, step, G)
        worst_n = max(worst_n, _normal_ratio((d["mu_negctrl"] - m0) / s0, eu, rad))
        _check_pi(d["pi"][:, 0], pr.pi_pair_screen(seed, step, conc, R, K=pr.K_GAMMA), f"survival seed {seed:#x} step {step}")
        gam, k, und, tol = pr.q0_screen(seed, step, conc_q, R, K=pr.K_GAMMA)
        assert int(k.max()) <= pr.MAX_ROUNDS and int(und.sum()) <= 2
        keep = ~und.any(0)  # a guide's replicates share a loop
        if not und.any():  # (an undecided gamma would move its replicate's total by O(1))
            assert np.all(np.abs(tot - gam.sum(1)) <= tol.sum(1) + 2.0 ** -23 * gam.sum(1)), (tot, gam.sum(1))
        x_ref = np.clip((gam / tot[:, None]).astype(np.float32), np.float32(pr.FLT_MIN), np.float32(1 - 2.0 ** -24)).astype(np.float64)
        x_tol = (tol + 2.0 ** -23 * gam) / tot[:, None] + 2.0 ** -23 * x_ref
        ratio = float((np.abs(d["initial_abundance"] - x_ref)[:, keep] / x_tol[:, keep]).max())
        worst_g = max(worst_g, ratio)
        print(f"survival seed {seed:#x} step {step}: initial_abundance worst |dev - ref| / tol {ratio:.3g}, "
              f"on the float32 floor {float((x_ref == pr.FLT_MIN).mean()):.3f}, q0 positions up to {int(k.max())}")
    eng.close()
    print(f"survival: normals worst {worst_n:.3g} x 2^-24 max(1, radius)")
    assert worst_n <= pr.K_ROCRAND and worst_g <= 1.0


def test_covariate_draws(engine):
    """Sorting Normal with two sample covariates: ``eps_cov`` is kSiteCov, element = covariate."""
    data = make_sorting_variant_screen(130, 4, seed=23)
    g = torch.Generator().manual_seed(23)
    data.sample_covariates = ["cov0", "cov1"]
    data.n_sample_covariates = 2
    data.rep_by_cov = torch.randint(0, 2, (4, 2), generator=g)
    data.rep_by_cov[0, 0], data.rep_by_cov[-1, 0] = 1, 0
    eng = engine.HipSVI("Normal", data.to(DEV), dump_noise=True, num_steps=50)
    worst = 0.0
    for seed in SEEDS:
        for step in STEPS:
            eng.elbo_grad(step=step, seed=seed)
            d = {k: v.cpu().numpy() for k, v in eng.drawn_noise().items()}
            ec, rad = pr.cov_draws(seed, step, 2)
            mu, sd, rad_t = pr.target_draws(seed, step, eng.T)
            worst = max(worst, _normal_ratio(d["eps_cov"], ec, rad), _normal_ratio(d["eps_mu"].reshape(-1), mu, rad_t),
                        _normal_ratio(d["eps_sd"].reshape(-1), sd, rad_t))
    eng.close()
    print(f"covariates: normals worst {worst:.3g} x 2^-24 max(1, radius)")
    assert worst <= pr.K_ROCRAND


def _tiling_engine(engine, A, n_guides=70):
    data = make_sorting_tiling_screen(n_guides, 2, n_max_alleles=A, seed=6)
    data.repguide_mask[1, 3] = False
    eng = engine.HipSVI("MultiMixtureNormal", data.to(DEV), dump_noise=True, num_steps=50)
    mask = data.allele_mask.numpy()
    p, alpha = _spread_alpha(n_guides, A, 40 + A)
    par = eng.unconstrained["alpha_pi"].cpu().numpy()
    eng.unconstrained["alpha_pi"].copy_(torch.as_tensor(np.where(mask, p, par)))
    alpha = np.where(mask, alpha, 1e-5)  # a masked allele's concentration is the model's epsilon
    return data, eng, mask, alpha


def _check_tiling(eng, data, replay, alpha, what):
    G, A = alpha.shape
    pa0 = data.pi_a0.numpy().astype(np.float64)
    worst = 0.0
    for seed, step in ((101, 1), (SEED64, 2 ** 26 + 5)):
        eng.elbo_grad(step=step, seed=seed)
        d = {k: v.cpu().numpy() for k, v in eng.drawn_noise().items()}
        mu, sd, rad = pr.target_draws(seed, step, eng.T)  # per edit
        worst = max(worst, _normal_ratio(d["eps_mu"].reshape(-1), mu, rad), _normal_ratio(d["eps_sd"].reshape(-1), sd, rad))
        s = np.zeros(G)
        for a in range(A):  # the kernels add the slots up in order
            s = s + alpha[:, a]
        conc = alpha * ((1.0 / s) * pa0)[:, None]
        pi, k, und, tol = replay(seed, step, conc, 2, K=pr.K_GAMMA)
        dev = d["pi"][:, 0].copy()
        assert np.all(dev[1, 3] == 1.0 / A)  # the masked (replicate, guide) exports 1 / A
        und = und.copy()
        und[1, 3] = True
        _check_pi(dev, (pi, k, und, tol), f"{what} seed {seed:#x} step {step}")
    print(f"{what}: normals worst {worst:.3g} x 2^-24 max(1, radius)")
    assert worst <= pr.K_ROCRAND


def test_tiling_register_kernel_draws(engine):
    """Tiling A = 5: the register-resident kernel draws a guide's components two at a time on one generator, the odd
    last one paired with shape 1.0."""
    data, eng, mask, alpha = _tiling_engine(engine, 5)
    assert eng.dominant_kernel != "k_guide_tiling_wide"
    _check_tiling(eng, data, pr.pi_tiling_screen, alpha, "tiling A = 5")
    eng.close()


def test_tiling_wide_kernel_draws(engine):
    """Tiling A = 40: the allele-parallel kernel, one stream per allele ((r G_tot + g) 256 + a), double-floor sampler,
    every allele paired with shape 1.0 (no partner a + 64 below A)."""
    data, eng, mask, alpha = _tiling_engine(engine, 40)
    assert eng.dominant_kernel == "k_guide_tiling_wide"
    _check_tiling(eng, data, pr.pi_wide_screen, alpha, "tiling A = 40")
    eng.close()
