"""The host replay of the device's draws (``philox_reference.py``) settled without the device: Random123's known-answer
vectors, the laws of its samplers, the key layout enumerated for a sharded screen, and the share of elements it leaves
undecided at every case the GPU tests run (``test_gpu_draw_replay.py``)."""
import functools

import numpy as np
import pytest
import scipy.stats as st

import philox_reference as pr

P_MIN = 1e-4  # the project's own (test_gpu_samplers.py)
N = 1 << 17
SEED = 0x1234567887654321


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("counter,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_random123_known_answers(counter, key, out):
    assert " ".join(f"{int(v):08x}" for v in pr.philox4x32_10(counter, key)) == out
    # the same through arrays, and through block(): counter = (offset >> 2, sub), key = seed, low halves first
    got = pr.philox4x32_10(tuple(np.array([c, c]) for c in counter), key)
    assert all(f"{int(v[1]):08x}" == w for v, w in zip(got, out.split()))
    if counter[1] < 1 << 30:
        blk = pr.block((key[1] << 32) | key[0], (counter[3] << 32) | counter[2], ((counter[1] << 32) | counter[0]) << 2)
        assert " ".join(f"{int(v):08x}" for v in blk) == out


def test_block_counter_carries_into_its_high_word():
    """An offset of 2^34 words is block 2^32: the counter's second word is 1, its first 0."""
    x = pr.block(SEED, pr.subsequence(2, 7), 1 << 34)
    y = pr.philox4x32_10((0, 1, 7, 2 << 16), (SEED & 0xFFFFFFFF, SEED >> 32))
    assert [int(v) for v in x] == [int(v) for v in y]
    assert [int(v) for v in x] != [int(v) for v in pr.block(SEED, pr.subsequence(2, 7), 0)]


def test_to_unit_range():
    assert pr.to_unit(0, 0) == 2.0 ** -53 and pr.to_unit(0xFFFFFFFF, 0xFFFFFFFF) == 1.0
    assert pr.to_unit(0x80000000, 0) == 0.5 + 2.0 ** -53


# --------------------------------------------------------------------------------------------------------- laws
def _uncorrelated(a, b):
    r = np.corrcoef(a, b)[0, 1]
    assert abs(r) < 5 / np.sqrt(a.size), r
    return r


def test_rocrand_normal2_law():
    x, y, rad = pr.normal_at(SEED, pr.SITE_TARGET, np.arange(N), 3)
    for v in (x, y):
        assert st.kstest(v, "norm").pvalue > P_MIN
    _uncorrelated(x, y)
    x1, _, _ = pr.normal_at(SEED, pr.SITE_TARGET, np.arange(N), 4)  # the next step of the same elements
    _uncorrelated(x, x1)
    assert np.allclose(np.hypot(x, y), rad, rtol=1e-12)


def test_gamma_round_law():
    na, nb, rad, ua, ub = pr.gamma_round(pr.block(SEED, pr.subsequence(pr.SITE_PI, np.arange(N)), 0))
    for v in (na, nb):
        assert st.kstest(v, "norm").pvalue > P_MIN
    for v in (ua, ub):
        assert st.kstest(v, "uniform").pvalue > P_MIN and 0.0 < v.min() and v.max() < 1.0
    _uncorrelated(na, nb)
    _uncorrelated(na, ua)
    assert np.array_equal(na, na.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("shape", [0.05, 0.3, 1.0, float(np.nextafter(1.0, 0.0)), 2.5, 10.7, 333.0, 1e4])
def test_gamma_pair_law(shape):
    """2^17 elements: both components follow Gamma(shape), are uncorrelated, and so are consecutive steps."""
    sub = pr.subsequence(pr.SITE_PI, np.arange(N))
    g0, g1, k, und, t0, t1 = pr.gamma_pair(np.full(N, shape), np.full(N, shape), SEED, sub, 256 * 7, 0, pr.K_GAMMA)
    for g in (g0, g1):
        assert st.kstest(g, st.gamma(shape).cdf).pvalue > P_MIN
    _uncorrelated(np.log(g0), np.log(g1))
    h0 = pr.gamma_pair(np.full(N, shape), np.full(N, shape), SEED, sub, 256 * 8, 0, 0.0)[0]
    _uncorrelated(np.log(g0), np.log(h0))
    assert k.min() >= (2 if shape < 1 else 1) and k.max() <= pr.MAX_ROUNDS
    assert und.mean() <= 1e-4 and np.all(t0 >= 0) and np.all(t1 >= 0)


def test_gamma_pair_mixed_shapes_and_floors_keep_the_law():
    """One boosted and one plain component; the FLOOR forms return the plain sampler's values wherever those are above
    the caller's floor, and the same generator position unless a shortcut ended the draw early."""
    sub = pr.subsequence(pr.SITE_Q0, np.arange(N))
    a0, a1 = np.full(N, 0.02), np.full(N, 3.0)
    plain = pr.gamma_pair(a0, a1, SEED, sub, 0, 0)
    assert st.kstest(plain[0], st.gamma(0.02).cdf).pvalue > P_MIN and st.kstest(plain[1], st.gamma(3.0).cdf).pvalue > P_MIN
    for floor, fl in ((1, pr.FLT_MIN), (2, pr.DBL_MIN)):
        f = pr.gamma_pair(a0, a1, SEED, sub, 0, floor)
        assert np.array_equal(np.maximum(f[0], fl), np.maximum(plain[0], fl)) and np.array_equal(f[1], plain[1])
        assert np.all(f[2] <= plain[2])
        tiny = np.full(N, 1e-4)
        both = pr.gamma_pair(tiny, tiny, SEED, sub, 0, floor)
        assert (both[2] == 1).mean() > 0.5  # both components on the floor: the boost block alone
        p = pr.gamma_pair(tiny, tiny, SEED, sub, 0, 0)
        assert np.array_equal(np.maximum(both[0], fl), np.maximum(p[0], fl))
    # a shape of exactly 0 (the odd last replicate of the q0 site): factor 0, no round for it
    z = pr.gamma_pair(a1, np.zeros(N), SEED, sub, 0, 1)
    assert np.all(z[1] == 0) and np.array_equal(z[0], pr.gamma_pair(a1, a0, SEED, sub, 0, 1)[0])


def test_dirichlet_pair_law():
    sub = pr.subsequence(pr.SITE_PI, np.arange(N))
    for a, b in ((0.4, 2.0), (10.7, 333.0)):
        p0, p1, k, und, t0, t1 = pr.dirichlet_pair(np.full(N, a), np.full(N, b), SEED, sub, 0, 0, pr.K_GAMMA)
        assert st.kstest(p0, st.beta(a, b).cdf).pvalue > P_MIN
        assert np.allclose(p0 + p1, 1.0, rtol=1e-15) and p0.min() >= pr.DBL_MIN and p0.max() <= pr.ONE_MINUS
    # the clamps: a component that underflows sits on DBL_MIN, its partner on 1 - eps
    p0, p1, *_ = pr.dirichlet_pair(np.full(N, 1e-5), np.full(N, 3.0), SEED, sub, 0)
    assert (p0 == pr.DBL_MIN).mean() > 0.9 and np.all(p1[p0 == pr.DBL_MIN] == pr.ONE_MINUS)


def test_dirichlet_A_law_and_odd_last_component():
    """A = 5: every component's marginal is Beta(a_i, sum - a_i); the odd last component comes from a pair with shape
    1.0, i.e. from the generator position the first two pairs left."""
    n = 1 << 15
    conc = np.tile(np.array([3.0, 0.4, 1.5, 0.08, 2.2]), (n, 1))
    sub = pr.subsequence(pr.SITE_PI, np.arange(n))
    pi, k, und, tol = pr.dirichlet_A(conc, SEED, sub, 0, 0, pr.K_GAMMA)
    assert np.allclose(pi.sum(1), 1.0, rtol=1e-14)
    for a in range(5):
        assert st.kstest(pi[:, a], st.beta(conc[0, a], conc[0].sum() - conc[0, a]).cdf).pvalue > P_MIN
    g01 = pr.gamma_pair(conc[:, 0], conc[:, 1], SEED, sub, 0)
    g23 = pr.gamma_pair(conc[:, 2], conc[:, 3], SEED, sub, 4 * g01[2].astype(np.uint64))
    g4 = pr.gamma_pair(conc[:, 4], np.ones(n), SEED, sub, 4 * (g01[2] + g23[2]).astype(np.uint64))
    assert np.array_equal(k, g01[2] + g23[2] + g4[2])
    gam = np.stack([g01[0], g01[1], g23[0], g23[1], g4[0]], 1)
    assert np.allclose(pi, gam / gam.sum(1, keepdims=True), rtol=1e-15)


# ------------------------------------------------------------------------------------------------------- layout
def _windows(G_tot, R, T_tot, n_cov, shards, steps, wide_A=None):
    """(site, element, step) -> (subsequence, first block, blocks) of every draw of a variant screen's sites 1 - 6 (and,
    with ``wide_A``, of a wide tiling screen's per-allele pi streams), enumerated shard by shard from the documented
    keys.  A normal reads one block at block ``step``; a pi or q0 element owns blocks ``64 step ... 64 step + 63``."""
    out = {}

    def put(site, el, step, first, n):
        key = (site, int(el), step)
        val = (int(pr.subsequence(site, int(el))), first, n)
        assert out.setdefault(key, val) == val
    for g0, g1, t0, t1 in shards:
        for step in steps:
            for t in range(t1 - t0):
                put(pr.SITE_TARGET, t0 + t, step, step, 1)
            for i in range(n_cov):  # replicated on every shard: the same window
                put(pr.SITE_COV, i, step, step, 1)
            for g in range(g1 - g0):
                put(pr.SITE_NOISE, g0 + g, step, step, 1)
                put(pr.SITE_AUX, g0 + g, step, step, 1)
                for r in range(R):
                    el = r * G_tot + g0 + g
                    if wide_A is None:
                        put(pr.SITE_PI, el, step, 64 * step, 64)
                    else:
                        for a in range(min(wide_A, 64)):
                            put(pr.SITE_PI, el * pr.wide_stream_stride(wide_A) + a, step, 64 * step, 64)
                    if r % 2 == 0:
                        put(pr.SITE_Q0, el, step, 64 * step, 64)
    return out


@pytest.mark.parametrize("wide_A", [None, 40])
def test_no_two_windows_share_a_counter(wide_A):
    """130 guides x 3 replicates cut into two shards (65 + 65 guides, 13 + 13 targets), 4 steps, sites 1 - 6: no two
    (site, element, step) windows overlap, and the shards together enumerate exactly the whole screen's windows."""
    steps = (0, 1, 2, 2 ** 26 + 5)
    whole = _windows(130, 3, 26, 2, [(0, 130, 0, 26)], steps, wide_A)
    cut = _windows(130, 3, 26, 2, [(0, 65, 0, 13), (65, 130, 13, 26)], steps, wide_A)
    assert cut == whole
    spans = sorted(whole.values())
    for (s0, f0, n0), (s1, f1, n1) in zip(spans, spans[1:]):
        assert s0 != s1 or f0 + n0 <= f1, (hex(s0), f0, n0, f1)
    assert len(spans) == len(whole)
    # the keys a wrong layout would give DO collide or leave the whole screen's set: G for G_tot on the second shard
    wrong = {(r * 65 + 65 + g) for r in range(3) for g in range(65)}
    right = {(r * 130 + 65 + g) for r in range(3) for g in range(65)}
    assert wrong != right and (wrong & {r * 130 + g for r in range(3) for g in range(65)})


@functools.lru_cache(maxsize=None)
def _op_case_summary(a0, a1, floor):
    g0, g1, k, und, t0, t1 = pr.op_case(pr.SITE_AUX, a0, a1, floor)
    return int(k.max()), float(und.mean())


def test_every_replayed_draw_stays_inside_its_step():
    """The generator position after a draw is at most 64 blocks (the 256 words between two steps' offsets) at every
    shape the GPU tests replay, and for an A = 32 tiling guide whose masked alleles have shapes of 1e-6: 16 pairs on
    one running generator."""
    worst = max(_op_case_summary(a0, a1, fl)[0] for a0, a1 in pr.OP_SHAPE_PAIRS for fl in (0, 1, 2))
    n = 1 << 14
    rng = np.random.default_rng(32)
    conc = np.full((n, 32), 1e-6)
    conc[:, :6] = np.exp(rng.uniform(np.log(0.05), np.log(50.0), (n, 6)))
    pi, k, und, tol = pr.dirichlet_A(conc, SEED, pr.subsequence(pr.SITE_PI, np.arange(n)), 0)
    print(f"largest generator position: {worst} blocks at the op-level cases, {int(k.max())} (mean {k.mean():.1f}) for "
          f"A = 32 with 26 masked alleles")
    assert worst <= pr.MAX_ROUNDS and int(k.max()) <= pr.MAX_ROUNDS
    assert (pi[:, 6:] == pr.DBL_MIN).mean() > 0.99


# ------------------------------------------------------------------------------------------------ undecided shares
def test_undecided_share_at_every_gpu_case():
    """At K_GAMMA - the bound on a gamma_round normal, measured on the device - the reference leaves at most 1e-4 of a
    case's elements undecided, at every (shape pair, FLOOR form) and every export case of the GPU tests."""
    assert pr.K_GAMMA <= 2 ** 10 and pr.K_ROCRAND <= 2 ** 10
    worst = 0.0
    for a0, a1 in pr.OP_SHAPE_PAIRS:
        shares = [_op_case_summary(a0, a1, fl)[1] for fl in (0, 1, 2)]
        print(f"({a0}, {a1}): undecided share, FLOOR 0, 1, 2: " + ", ".join(f"{s:.2e}" for s in shares))
        worst = max(worst, *shares)
    for a0, a1 in pr.OP_EXPORT_PAIRS:
        for site in (pr.SITE_Q0, pr.SITE_PI):
            worst = max(worst, float(pr.op_case(site, a0, a1, 0)[3].mean()))
    print(f"worst undecided share {worst:.2e} at K_GAMMA = {pr.K_GAMMA:g}")
    assert worst <= 1e-4


def test_undecided_flags_what_a_perturbed_normal_would_change():
    """The flag does its job: with the normals moved by the whole bound either way, the elements whose position or
    values move by more than their tolerance are among the flagged ones (here at a K large enough to flag some)."""
    K = 8192.0
    a0, a1 = 0.3, 2.5
    g0, g1, k, und, t0, t1 = pr.op_case(pr.SITE_AUX, a0, a1, 0, K)
    assert 0 < und.sum() < 0.01 * und.size
    real = pr.gamma_round
    seen = np.zeros(und.size, bool)
    try:
        for sign in (-1.0, 1.0):
            def moved(blk, sign=sign):
                na, nb, rad, ua, ub = real(blk)
                dn = sign * pr.normal_bound(K, rad)
                return na + dn, nb + dn, rad, ua, ub
            pr.gamma_round = moved
            h0, h1, hk, *_ = pr.op_case(pr.SITE_AUX, a0, a1, 0, 0.0)
            changed = (hk != k) | (np.abs(h0 - g0) > 1.05 * t0) | (np.abs(h1 - g1) > 1.05 * t1)
            assert not np.any(changed & ~und), int((changed & ~und).sum())
            seen |= changed
    finally:
        pr.gamma_round = real
    assert seen.sum() > 0.2 * und.sum()


# -------------------------------------------------------------------- what a wrong assumption does to the replay
def test_wrong_layout_assumptions_move_the_replay_by_far_more_than_its_tolerance():
    """The four changes to the reference's device-facing assumptions, tried here on the host: three move the replayed
    draws by O(1) against tolerances of ~1e-5 - so the GPU tests, which hold the device to the unchanged reference,
    cannot pass with either - and one changes no draw at all: the squeeze is a shortcut INSIDE the log test's acceptance
    region (Marsaglia & Tsang's inequality), so 0.0332 - or 0.0330 - sends a few more or fewer rounds to the log test,
    which decides them the same way.  No comparison of draws can see that constant."""
    G, R = 130, 2
    rng = np.random.default_rng(3)
    conc = np.exp(rng.uniform(np.log(0.05), np.log(50.0), (G, 2)))
    far = lambda a, b: (np.abs(a[0] - b[0]) > 100 * (a[3] + b[3])).any(-1)
    good = pr.pi_pair_screen(SEED, 1, conc, R, K=pr.K_GAMMA)
    # a pi offset of 255 step: block 63 of step 0's window instead of block 64
    bad = pr.pi_pair_screen(SEED, 1, conc, R, K=pr.K_GAMMA, stride=255)
    assert far(good, bad).mean() > 0.99
    assert np.array_equal(pr.pi_pair_screen(SEED, 0, conc, R, stride=255)[0], pr.pi_pair_screen(SEED, 0, conc, R)[0])
    # G in place of G_tot on a shard: replicate 0 keeps its keys, every later replicate takes another guide's
    shard = pr.pi_pair_screen(SEED, 1, conc[65:], R, G_tot=130, g_off=65, K=pr.K_GAMMA)
    assert np.array_equal(shard[0], good[0][:, 65:])
    bad = pr.pi_pair_screen(SEED, 1, conc[65:], R, G_tot=65, g_off=65, K=pr.K_GAMMA)
    assert not far(shard, bad)[0].any() and far(shard, bad)[1].mean() > 0.99
    # a dropped boost block: the first round reuses the boost's words; a boosted element's position is one short (unless
    # the other words cost it a round more), and no other element changes
    boosted = (conc < 1).any(1)
    assert boosted.sum() > 10
    bad = pr.pi_pair_screen(SEED, 1, conc, R, K=pr.K_GAMMA, boost_block=False)
    assert not (bad[1] != good[1])[:, ~boosted].any() and (bad[1] != good[1])[:, boosted].mean() > 0.9
    assert far(good, bad)[:, boosted].mean() > 0.95
    # the squeeze constant: no draw and no position changes
    for sq in (0.0330, 0.0332):
        bad = pr.pi_pair_screen(SEED, 1, conc, R, squeeze=sq)
        same = pr.pi_pair_screen(SEED, 1, conc, R)
        assert np.array_equal(bad[0], same[0]) and np.array_equal(bad[1], same[1])
    for a0, a1 in ((0.3, 0.7), (2.5, 2.5)):
        b = pr.op_case(pr.SITE_AUX, a0, a1, 0, 0.0)
        s = pr.gamma_pair(np.full(pr.OP_N, a0), np.full(pr.OP_N, a1), pr.OP_SEED, pr.subsequence(pr.SITE_AUX, np.arange(pr.OP_N)),
                          0, 0, 0.0, squeeze=0.0332)
        assert np.array_equal(b[0], s[0]) and np.array_equal(b[1], s[1]) and np.array_equal(b[2], s[2])


def test_settled_log():
    target = np.exp(np.random.default_rng(1).uniform(-16, 4, 200))
    target = target[np.abs(np.log(target)) > 0.5]
    p, v = pr.settled_log(target)
    assert p.dtype == np.float32 and np.array_equal(v, v.astype(np.float32).astype(np.float64))
    e = np.exp(p.astype(np.float64))
    assert np.all(np.abs(e - v) < 0.02 * np.spacing(v.astype(np.float32)).astype(np.float64))
    assert np.all(np.abs(np.log(v / target)) < 1e-3)
