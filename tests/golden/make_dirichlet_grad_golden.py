"""Freeze the points at which the implicit Dirichlet gradient is held to its exact formula.

    python tests/golden/make_dirichlet_grad_golden.py

Everything comes from this repository's own tests/dirichlet_grad_reference.py: the branch of each point in exact
arithmetic, the formula's value at 60 digits, its first-order error budget, and - where the point lies within 1e-12 of a
branch edge - the value and budget of the other branch it reaches.  All arrays are float64:

    x, alpha, total     the inputs, x clamped to [DBL_MIN, nextafter(1, 0)] as the kernels clamp their draws
    branch, near_edge   index into dirichlet_grad_reference.BRANCHES; 1 where an edge is within 1e-12 relative
    ref, budget_rel     the value, and the budget divided by |value|
    branch2, ref2, budget2_rel   the second branch of a point near an edge (NaN elsewhere)
    exact_edge          1 where a planted edge point is exact in float64 (every evaluation must take `branch`)
    kind                0 bulk, 1 drawn from the same law to fill a stratum, 2 planted
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dirichlet_grad_reference as dr  # noqa: E402

OUT = os.path.join(HERE, "dirichlet_grad_cases.npz")
N_BULK = 1400
MAX_POINTS = 4000
# the strata of the fixture: (name, smallest count)
MIN_PER_BRANCH, MIN_HIGH, MIN_LOW, MIN_FLOOR, MIN_CEIL = 400, 300, 300, 100, 100
HIGH, LOW = 2e3, 1e-3
WINDOW_AB = ((7.0, 7.0), (50.0, 3e3), (3e4, 3e4), (9e4, 7.0))
MASKED_TOTALS = (0.5, 10.0, 7e4)
ABOVE_FLOOR = 1e-120  # a draw of Beta(1e-5, .) that stays above DBL_MIN


def candidates(n, seed=20):
    """alpha, beta log-uniform on [1e-5, 1e5]; x ~ Beta(alpha, beta), every tenth point from Beta(alpha / 4, beta / 4)
    (the tails a fit sees); clamped as the kernels clamp."""
    rng = np.random.default_rng(seed)
    al = np.exp(rng.uniform(np.log(1e-5), np.log(1e5), n))
    be = np.exp(rng.uniform(np.log(1e-5), np.log(1e5), n))
    wide = np.arange(n) % 10 == 9
    x = rng.beta(np.where(wide, al / 4, al), np.where(wide, be / 4, be))
    x = np.clip(np.where(np.isfinite(x), x, 0.0), dr.DBL_MIN, dr.ONE_MINUS)
    return x, al, al + be


def strata(x, alpha, total, branch):
    beta = total - alpha
    out = {f"branch {b}": branch == i for i, b in enumerate(dr.BRANCHES)}
    out["both above 2e3"] = (alpha > HIGH) & (beta > HIGH)
    out["one below 1e-3"] = (alpha < LOW) | (beta < LOW)
    out["x == DBL_MIN"] = x == dr.DBL_MIN
    out["x == nextafter(1, 0)"] = x == dr.ONE_MINUS
    return out


MINIMA = dict({f"branch {b}": MIN_PER_BRANCH for b in dr.BRANCHES}, **{
    "both above 2e3": MIN_HIGH, "one below 1e-3": MIN_LOW, "x == DBL_MIN": MIN_FLOOR, "x == nextafter(1, 0)": MIN_CEIL})


def drawn_points():
    """The bulk, then further draws of the same law, in order, for every stratum the bulk leaves thin."""
    x, al, tot = candidates(400_000)
    st = strata(x, al, tot, dr.branch64(x, al, tot))
    take = np.zeros(len(x), dtype=bool)
    take[:N_BULK] = True
    for name, least in MINIMA.items():
        want = int(1.05 * least) + 5  # (the exact branch of a few points may differ from the float64 one)
        have = int((st[name] & take).sum())
        more = np.nonzero(st[name] & ~take)[0][:max(0, want - have)]
        take[more] = True
    idx = np.nonzero(take)[0]
    return x[idx], al[idx], tot[idx], (idx >= N_BULK).astype(np.float64)


def planted_points():
    """(x, alpha, total, exact_edge) of every planted point."""
    import mpmath

    up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    pts = []
    # boundary = total x (1 - x) on 2.5 and on 0.75, in exactly representable values
    for alpha in (0.5, 3.0):
        pts.append((0.5, alpha, 10.0, 1))   # 2.5 exactly: not below it
        pts.append((0.5, alpha, 3.0, 1))    # 0.75 exactly at x = 0.5: the small-alpha series takes it first
        for x in (0.25, 0.75):
            pts.append((x, alpha, 4.0, 1))      # 0.75 exactly
            pts.append((x, alpha, 13.25, 1))    # 2.484375
            pts.append((x, alpha, 13.5, 1))     # 2.53125
        pts.append((0.5, alpha, down(10.0), 0))
        pts.append((0.75, alpha, down(4.0), 0))
    # alpha = 6 and one ulp either side (beta = 20 within an ulp of the total); beta = 6 and the nearest doubles that
    # total - alpha gives exactly (an ulp of the total, two of beta)
    for a6 in (down(6.0), 6.0, up(6.0)):
        pts.append((0.3, a6, a6 + 20.0, 1))
    for tot in (down(13.0), 13.0, up(13.0)):
        assert (tot - 7.0) + 7.0 == tot
        pts.append((0.4, 7.0, tot, 1))
    # the near-mean window: the doubles nearest mean +/- 0.1 sd, and the mean
    with mpmath.workdps(dr.DPS):
        for a, b in WINDOW_AB:
            am, bm = mpmath.mpf(a), mpmath.mpf(b)
            mean = am / (am + bm)
            sd = mpmath.sqrt(am * bm / (am + bm + 1)) / (am + bm)
            for v in (mean - mpmath.mpf(0.1) * sd, mean, mean + mpmath.mpf(0.1) * sd):
                pts.append((float(v), a, a + b, 0))
    # masked alleles (get_alpha's clamp of 1e-5) on the floor and above it, and their mirror at the ceiling
    for tot in MASKED_TOTALS:
        pts.append((dr.DBL_MIN, 1e-5, tot, 0))
        pts.append((ABOVE_FLOOR, 1e-5, tot, 0))
        pts.append((dr.ONE_MINUS, tot - 1e-5, tot, 0))
    # digamma(a + b) - digamma(b) with a tiny and b = 1e5, in either series
    for small in (1e-5, 1e-3):
        pts.append((dr.ONE_MINUS, 1e5, 1e5 + small, 0))
        pts.append((1.0 - 2.0 ** -20, 1e5, 1e5 + small, 0))
        pts.append((dr.DBL_MIN, small, small + 1e5, 0))
        pts.append((ABOVE_FLOOR, small, small + 1e5, 0))
    return tuple(np.array(c, dtype=np.float64) for c in zip(*pts))


def main():
    bx, ba, bt, bkind = drawn_points()
    px, pa, pt, pexact = planted_points()
    x, alpha, total = np.concatenate([bx, px]), np.concatenate([ba, pa]), np.concatenate([bt, pt])
    kind = np.concatenate([bkind, np.full(len(px), 2.0)])
    exact_edge = np.concatenate([np.zeros(len(bx)), pexact])
    rows = np.array([dr.reference_point(*p) for p in zip(x, alpha, total)])
    out = dict(x=x, alpha=alpha, total=total, branch=rows[:, 0], near_edge=rows[:, 1], ref=rows[:, 2],
               budget_rel=rows[:, 3], branch2=rows[:, 4], ref2=rows[:, 5], budget2_rel=rows[:, 6],
               exact_edge=exact_edge, kind=kind)
    check(out)
    np.savez_compressed(OUT, **out)
    print(f"{len(x)} points, {os.path.getsize(OUT)} bytes")


def check(f):
    """The strata and planted points the fixture promises (the test of the fixture runs this too)."""
    n = len(f["x"])
    assert n <= MAX_POINTS and all(v.dtype == np.float64 and v.shape == (n,) for v in f.values())
    assert (f["x"] >= dr.DBL_MIN).all() and (f["x"] <= dr.ONE_MINUS).all()
    st = strata(f["x"], f["alpha"], f["total"], f["branch"].astype(int))
    for name, least in MINIMA.items():
        assert int(st[name].sum()) >= least, (name, int(st[name].sum()))
    # the reference is a finite, normal, non-zero double at every point, in either branch: no NaN fallback fires
    for k in ("ref", "budget_rel"):
        assert np.isfinite(f[k]).all(), k
    assert (np.abs(f["ref"]) >= dr.DBL_MIN).all()
    two = ~np.isnan(f["branch2"])
    assert (f["near_edge"][two] == 1).all() and np.isfinite(f["ref2"][two]).all() and np.isfinite(f["budget2_rel"][two]).all()
    px, pa, pt, pexact = planted_points()
    pl = f["kind"] == 2
    for k, v in (("x", px), ("alpha", pa), ("total", pt), ("exact_edge", pexact)):
        assert np.array_equal(f[k][pl], v), k
    assert (f["near_edge"][pl] == 1).sum() >= 26  # 12 on the boundary, 6 on alpha | beta = 6, 8 on the window
    reached = set(f["branch"][pl].astype(int)) | set(f["branch2"][pl & two].astype(int))
    assert reached == set(range(5)), reached


if __name__ == "__main__":
    main()
