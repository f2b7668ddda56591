"""The Marsaglia-Tsang acceptance test settled in float32 (csrc/bean_special.hpp: mt_accept_f32, mt_accept) must decide
exactly as the float64 test (mt_accept_exact), lane for lane, and the sampler built on it must return the float64
sampler's draws and generator position.  -m gpu.

The test is ``log u < n^2 / 2 + d (1 - v + log v)``, ``v = (1 + n / sqrt(9 d))^3``.  The float32 form evaluates it
from two hardware float32 logs with an error bound ``E`` and hands the lanes within ``E`` of the turning point - and
those whose ``v`` is no normal float32 - to the float64 test.  ``bean_hip_test_special`` op 24 returns both decisions
and whether float32 settled it at arbitrary ``(d, n, u)``; ops 12 - 23 run the whole sampler in both forms.
"""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401

pytestmark = pytest.mark.gpu
GRID = 2.0 ** -32  # the sampler's acceptance uniforms: (k + 0.5) 2^-32
U_MIN, U_MAX = 0.5 * GRID, 1.0 - 0.5 * GRID


@pytest.fixture(scope="module")
def engine():
    from bean_amd import engine as eng

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return eng


def _decide(engine, d, n, u):
    exact, fast = engine.test_special(24, d, n, u)
    exact, fast = exact.cpu().numpy(), fast.cpu().numpy()
    tested = exact >= 0  # 1 + c n > 0: the sampler reaches the test
    assert np.array_equal(tested, fast >= 0)
    settled = fast >= 2
    return tested, exact == 1, (fast % 2) == 1, settled


def _rhs(d, n):
    c = 1.0 / np.sqrt(9.0 * d)
    y = 1.0 + c * n
    with np.errstate(invalid="ignore", divide="ignore"):
        v = y * y * y
        return y, 0.5 * n * n + d * (1.0 - v + np.log(v))


def test_decisions_on_random_points(engine):
    """2 10^6 points: d log-uniform in [0.67, 1e4], n a float32 normal, u on the sampler's grid.  Equal decisions
    everywhere; and where the product runs (d in [6, 400]: the metric screen has 10.7 ... 333) float32 settles more
    than 99 % of the lanes whose squeeze test failed - the float64 emulation of the bound leaves 0.27 % over, and so does the device."""
    rng = np.random.default_rng(2024)
    N = 2_000_000
    d = np.exp(rng.uniform(np.log(0.67), np.log(1e4), N))
    n = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    u = (rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.float64) + 0.5) * GRID
    tested, exact, fast, settled = _decide(engine, d, n, u)
    y, _ = _rhs(d, n)
    assert np.array_equal(tested, y > 0)
    squeeze_fails = tested & ~(u < 1.0 - 0.0331 * (n * n) * (n * n))
    band = squeeze_fails & (d >= 6.0) & (d <= 400.0)
    share = float((~settled[band]).mean())
    print(f"random points: {int(tested.sum())} tested, {int((exact != fast)[tested].sum())} decisions differ; "
          f"squeeze fails for {int(squeeze_fails.sum())} ({squeeze_fails.mean():.4f}), accepted there "
          f"{exact[squeeze_fails].mean():.4f}; d in [6, 400]: {int(band.sum())} lanes, undecided share {share:.5f}; "
          f"all d: undecided share {float((~settled[squeeze_fails]).mean()):.5f}")
    assert np.array_equal(exact[tested], fast[tested])
    assert band.sum() > 20_000
    assert share < 0.01, share


def test_decisions_at_the_turning_point(engine):
    """For 10^4 (d, n) the host finds by bisection the u* at which the float64 inequality turns, and the device decides
    at u* moved by 0, +-1, +-2, +-8 ulps and by relative 2^-30 ... 2^-10 either way, and at both ends of u's range."""
    rng = np.random.default_rng(7)
    M = 10_000
    d = np.exp(rng.uniform(np.log(0.67), np.log(1e4), M))
    n = rng.standard_normal(M).astype(np.float32).astype(np.float64) * 1.5
    y, rhs = _rhs(d, n)
    keep = (y > 0) & (rhs < np.log(U_MAX)) & (rhs > np.log(U_MIN))
    d, n, rhs = d[keep], n[keep], rhs[keep]
    assert d.size > 0.9 * M
    lo, hi = np.exp(rhs) * (1 - 1e-9), np.exp(rhs) * (1 + 1e-9)
    assert np.all(np.log(lo) < rhs) and np.all(~(np.log(hi) < rhs))
    for _ in range(64):  # to adjacent doubles: log(lo) < rhs, not log(hi) < rhs
        mid = 0.5 * (lo + hi)
        acc = np.log(mid) < rhs
        lo, hi = np.where(acc, mid, lo), np.where(acc, hi, mid)
    ustar = hi
    pts = []
    for k in (0, 1, 2, 8):
        up, dn = ustar.copy(), ustar.copy()
        for _ in range(k):
            up, dn = np.nextafter(up, 2.0), np.nextafter(dn, 0.0)
        pts += [up, dn] if k else [up]
    n_ulp = len(pts)
    for e in range(10, 31):
        pts += [ustar * (1.0 + 2.0 ** -e), ustar * (1.0 - 2.0 ** -e)]
    pts += [np.full_like(ustar, U_MIN), np.full_like(ustar, U_MAX)]
    raw = np.concatenate(pts)
    uu = np.clip(raw, U_MIN, U_MAX)
    dd, nn = np.tile(d, len(pts)), np.tile(n, len(pts))
    tested, exact, fast, settled = _decide(engine, dd, nn, uu)
    near = np.zeros(uu.size, bool)
    near[: n_ulp * d.size] = True
    print(f"turning points: {uu.size} points of {d.size} (d, n); {int((exact != fast).sum())} decisions differ; "
          f"accepted {exact.mean():.3f}; settled in float32 {settled.mean():.3f} of all, "
          f"{settled[near].mean():.5f} of those within 8 ulps")
    assert tested.all()
    assert np.array_equal(exact, fast)
    # within 8 ulps of the turning point |t| is far inside the bound: all of them take the float64 test, and it gives
    # both answers there; a relative 2^-10 away (the first pair after the ulp steps; those the clip to u's range did
    # not move back) |t| = 1e-3 is beyond the bound wherever d < 100 (E < 2^-19 (1 + 23 + 100 (1 + 1)) = 4e-4)
    assert not settled[near].any()
    assert 0.05 < exact[near].mean() < 0.95
    far = slice(n_ulp * d.size, (n_ulp + 2) * d.size)
    assert settled[far][(np.tile(d, 2) < 100.0) & (uu[far] == raw[far])].mean() > 0.9


def test_decisions_where_v_underflows_in_float32(engine):
    """y = 1 + c n just above 0: v = y^3 is below FLT_MIN (no normal float32, the hardware log of it is no number to
    rely on), so these lanes must go to the float64 test whatever u is - which rejects them all."""
    d = np.repeat(np.geomspace(0.67, 4.8, 40), 60)
    ytar = np.tile(np.geomspace(1e-16, 1e-11, 60), 40)
    n = -(1.0 - ytar) * np.sqrt(9.0 * d)
    dd, nn = np.tile(d, 3), np.tile(n, 3)
    uu = np.concatenate([np.full(d.size, U_MIN), np.full(d.size, 0.5), np.full(d.size, U_MAX)])
    tested, exact, fast, settled = _decide(engine, dd, nn, uu)
    y, _ = _rhs(dd, nn)
    small = tested & (y ** 3 < 1.0e-38)
    print(f"v underflow: {int(tested.sum())} of {dd.size} tested, {int(small.sum())} with v < 1e-38, "
          f"{int(settled[small].sum())} of them settled in float32, {int((exact != fast)[tested].sum())} decisions differ")
    assert small.sum() > 1000
    assert np.array_equal(exact[tested], fast[tested])
    assert not settled[small].any()
    assert not exact[tested].any()


@pytest.mark.parametrize("floor", [0, 1, 2])
def test_sampler_returns_the_float64_samplers_draws(engine, floor):
    """10^6 pairs (a0, a1), log-uniform in [1e-6, 1e4]^2, same seed: the inlined sampler with the float32 test (ops
    12 - 14) against the out-of-line one with the float64 test (15 - 17), every FLOOR form: both draws and the
    generator position after them."""
    rng = np.random.default_rng(100 + floor)
    N = 1_000_000
    a0 = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), N))
    a1 = np.exp(rng.uniform(np.log(1e-6), np.log(1e4), N))
    seed = np.zeros(N)
    seed[:1] = np.frombuffer(np.uint64(31337 + floor).tobytes(), dtype=np.float64)
    f0, f1 = engine.test_special(12 + floor, a0, seed, a1)
    e0, e1 = engine.test_special(15 + floor, a0, seed, a1)
    fk, _ = engine.test_special(18 + floor, a0, seed, a1)
    ek, _ = engine.test_special(21 + floor, a0, seed, a1)
    print(f"FLOOR {floor}: draws differ in {int((f0 != e0).sum())} + {int((f1 != e1).sum())} of {N}, positions in "
          f"{int((fk != ek).sum())}; mean rounds {float(ek.mean()):.3f}, zero draws {float((e0 == 0).double().mean()):.3f}")
    assert torch.equal(f0, e0) and torch.equal(f1, e1)
    assert torch.equal(fk, ek)
    assert float(ek.min()) >= 0 and float(ek.max()) > 2  # some lanes needed further rounds
    assert torch.isfinite(e0).all() and torch.isfinite(e1).all() and float((e0 > 0).double().mean()) > 0.5
