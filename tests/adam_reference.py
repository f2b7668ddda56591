"""What the direct ClippedAdam tests share (tests/test_adam_reference.py on the CPU, tests/test_gpu_adam.py on the GPU):
a float64 reference of ``pyro.optim.ClippedAdam``'s update on float32 inputs, per-element error bounds for a float32
evaluation of it, and the input set.  Not a test module.

The bounds are a first-order propagation of the roundings that ``adam_update`` (csrc/bean_kernels.hpp) performs, each
of them at most u |x| with u = 2^-24 for a normal float32 result x (correctly rounded *, fma, sqrtf, /):

    m9 = fl(0.9 m)                        u |m9|
    m' = fl(0.1 gc + m9)   (fma)          u |m'|                    => bm = u (|m9| + |m'|)
    g2 = fl(gc gc)                        u g2, scaled by 0.001
    v9 = fl(0.999 v)                      u v9
    v' = fl(0.001 g2 + v9) (fma)          u v'                      => bv = u (0.001 gc^2 + v9 + v')
    s  = fl(sqrt(v'))                     bv / (2 sqrt(v')) + u s    (the error of v' through d sqrt = 1 / (2 sqrt))
    D  = fl(s + eps)                      u D                       => bD = bv / (2 sqrt(v')) + u s + u D
    q  = fl(m' / D)                       u |q|                     => bq = bm / D + |q| bD / D + u |q|
    ss = float32(step_size)               u ss
    p' = fl(p - ss q)      (fma)          u |p'|                    => bp = ss bq + u ss |q| + u |p'|

bm / D carries the error of m' where 0.9 m + 0.1 g cancels (relative to m' it is unbounded; relative to the terms it
is u), and bv / (2 sqrt(v')) the error of v'.  Nothing here is fitted to an implementation.  All three are doubled:
the unrounded terms above are exact only to first order, and an evaluation that rounds an fma's sum twice (float64,
then float32) or splits an fma into * and + (torch on the CPU) makes at most one more rounding of the same size per
line, each of which the line's own terms dominate (|0.1 gc| <= |m9| + |m'|, 0.001 gc^2 <= v').
"""
import itertools

import numpy as np

F32 = np.float32
B1, A1 = float(F32(0.9)), float(F32(1 - 0.9))       # exp_avg.mul_(b1).add_(grad, alpha=1 - b1) on a float32 tensor
B2, A2 = float(F32(0.999)), float(F32(1 - 0.999))   # exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1 - b2)
EPS = float(F32(1e-8))
U = 2.0 ** -24
CLIP = 10.0


def lrd_of(gamma, num_steps):
    return float(gamma) ** (1.0 / int(num_steps))


def step_size(t, lr0=0.01, lrd=1.0):
    """``lr_t sqrt(1 - b2^t) / (1 - b1^t)`` with ``lr_t`` = lr0 multiplied by lrd t times, as Pyro does
    (``state["lr"] *= lrd`` once per update), betas (0.9, 0.999) as the Python floats Pyro holds."""
    lr = float(lr0)
    for _ in range(int(t)):
        lr *= float(lrd)
    return lr * np.sqrt(1.0 - 0.999 ** int(t)) / (1.0 - 0.9 ** int(t))


def clipped_adam_ref(p, m, v, g, t, lr0=0.01, lrd=1.0, clip=CLIP):
    """Pyro's update t (1-based) in float64 on float32 inputs: (p', m', v').  NaN passes the clamp (np.clip, as
    torch's clamp_), +-inf clamps to +-clip."""
    p, m, v, g = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, m, v, g))
    with np.errstate(invalid="ignore"):
        gc = np.clip(g, -float(clip), float(clip))
        m1 = B1 * m + A1 * gc
        v1 = B2 * v + A2 * gc * gc
        p1 = p - step_size(t, lr0, lrd) * m1 / (np.sqrt(v1) + EPS)
    return p1, m1, v1


def adam_bounds(p, m, v, g, t, lr0=0.01, lrd=1.0, clip=CLIP):
    """(bm, bv, bp): see the module docstring.  Finite wherever the reference is."""
    p, m, v, g = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (p, m, v, g))
    with np.errstate(invalid="ignore", divide="ignore"):
        gc = np.clip(g, -float(clip), float(clip))
        p1, m1, v1 = clipped_adam_ref(p, m, v, g, t, lr0, lrd, clip)
        ss = abs(step_size(t, lr0, lrd))
        bm = U * (np.abs(B1 * m) + np.abs(m1))
        bv = U * (A2 * gc * gc + B2 * v + v1)
        s = np.sqrt(v1)
        D = s + EPS
        q = m1 / D
        bs = np.where(bv > 0, bv / (2.0 * np.where(s > 0, s, 1.0)), 0.0) + U * s   # (v' = 0 only with bv = 0)
        bD = bs + U * D
        bq = bm / D + np.abs(q) * bD / D + U * np.abs(q)
        bp = ss * bq + U * ss * np.abs(q) + U * np.abs(p1)
    return 2.0 * bm, 2.0 * bv, 2.0 * bp


GRID_G = [0.0] + [s * x for x in (1e-15, 1e-8, 1e-3, 0.3, 1.0, 9.999999, 10.0, 10.000001, 1e4, 3e38, np.inf) for s in (1, -1)]
GRID_V = [0.0, 1e-30, 1e-16, 1e-6, 1.0, 1e6]   # 1e-16: sqrt(v) = eps
GRID_M = [0.0, 1e-3, -1e-3, 5.0, -5.0]
GRID_P = [0.0, 1.0, -1.0, 1e3, -3.7]
N_GRID = len(GRID_G) * len(GRID_V) * len(GRID_M) * len(GRID_P)


def _grid():
    rows = np.array(list(itertools.product(GRID_P, GRID_M, GRID_V, GRID_G)), dtype=np.float64)
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


def _log_uniform(rng, n, lo, hi):
    return np.exp(rng.uniform(lo, hi, n))


def adam_cases(n, seed):
    """n inputs (p, m, v, g) as float32 arrays.  n >= N_GRID: the whole grid GRID_P x GRID_M x GRID_V x GRID_G first.
    A shorter array takes n // 2 rows of the grid picked at random.  The rest are random draws: |g| log-uniform over
    e^-20 ... e^12 with a sign, v over e^-60 ... e^18, |m| over e^-20 ... e^2.3 with a sign, p ~ 3 N(0, 1); in every
    eighth of them g = -9 m (1 + d), d in {0, +-1e-7, +-1e-4}: 0.9 m + 0.1 g cancels.  Every nonzero intermediate
    of the update stays a normal float32 (0.001 g^2 >= 1e-33 is asserted), so that nothing depends on how subnormals
    are treated."""
    rng = np.random.default_rng(seed)
    gp, gm, gv, gg = _grid()
    if n < N_GRID:
        pick = rng.choice(N_GRID, size=n // 2, replace=False)
        gp, gm, gv, gg = gp[pick], gm[pick], gv[pick], gg[pick]
    k = n - gp.size
    g = _log_uniform(rng, k, -20.0, 12.0) * rng.choice([-1.0, 1.0], k)
    v = _log_uniform(rng, k, -60.0, 18.0)
    m = _log_uniform(rng, k, -20.0, 2.3) * rng.choice([-1.0, 1.0], k)
    p = 3.0 * rng.standard_normal(k)
    cancel = np.arange(k) % 8 == 7
    d = rng.choice([0.0, 1e-7, -1e-7, 1e-4, -1e-4], k)
    g = np.where(cancel, -9.0 * m * (1.0 + d), g)
    out = [np.concatenate([a, b]).astype(np.float32) for a, b in ((gp, p), (gm, m), (gv, v), (gg, g))]
    p32, m32, v32, g32 = out
    gc = np.clip(g32.astype(np.float64), -CLIP, CLIP)
    assert np.all((gc == 0) | (A2 * gc * gc >= 1e-33)) and np.all((v32 == 0) | (v32 >= 1e-33))
    assert np.all((m32 == 0) | (np.abs(m32) >= 1e-9))
    return p32, m32, v32, g32


def violations(got, ref, bound):
    """Elements of ``got`` outside ``ref`` +- ``bound`` (NaN in ``got`` or a non-finite reference counts), and the
    worst |got - ref| / bound over the elements with a nonzero bound."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(got - ref)
        bad = ~(err <= bound)
        ratio = np.where(bound > 0, err / bound, 0.0)
    return bad, float(np.nanmax(ratio)) if ratio.size else 0.0
