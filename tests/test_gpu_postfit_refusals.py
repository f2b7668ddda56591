"""The refusals of the nine post-fit entry points of the library (bean_hip_simulate, _simulate_members, _simulate_design,
_simulate_power, _log_weights, _log_weights_marginal, _marginal_grid, _marginal_grid_tail, _marginal_tail_nodes), pinned to
the full text of bean_hip_last_error() in one table: (entry point, handle, arguments, message).  Calls that are wrong
twice pin the order in which an entry point tests its refusals.  After every row the output buffers still hold their
fill (nothing was launched), and at the end every entry point takes its good arguments (the handle is usable).  -m gpu."""
import ctypes

import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd import _lib
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

from members_common import DEV, SEED

pytestmark = pytest.mark.gpu

FILL = -7
K, D, S, N_MU, N_Y = 3, 2, 3, 3, 2
N = N_MU * N_Y

TAKE = (" (bean_hip_predictive_supported): sorting variant Normal / MixtureNormal, unsharded, no sample covariates, "
        "one member, one particle")
SIM = ": the count simulator does not take this handle" + TAKE
LOGW = ": the importance weights do not take this handle" + TAKE
GRID = ": the grid posterior does not take this handle" + TAKE
ACC = (": a handle with accessibility (BEAN_FLAG_SCALE_BY_ACC) is refused: the guide noise is a further latent per "
       "guide, so the posterior of a target is not 2-D")
PREPARE = ": call bean_hip_prepare first"
NO_BC = ": xbc_out on a handle without BEAN_FLAG_USE_BCMATCH"
HAS_BC = ": this handle uses the barcode-matched counts: xbc_out must hold "
CENTRES = ": centre_mu, centre_y, step_mu and step_y must each hold (T) float64 on the device; one of them is null"

# the arguments of every entry point between the handle and the stream, in the order of include/bean_hip.h
ARGS = {
    "bean_hip_simulate": ("seed", "draw", "x", "x_b", "xbc", "xbc_b", "alpha", "alpha_b"),
    "bean_hip_simulate_members": ("seed", "draw", "k", "x", "x_b", "xbc", "xbc_b"),
    "bean_hip_simulate_design": ("seed", "draw", "k", "vals", "d", "x", "x_b", "xbc", "xbc_b"),
    "bean_hip_simulate_power": ("seed", "draw", "k", "vals", "d", "plant", "x", "x_b", "xbc", "xbc_b"),
    "bean_hip_log_weights": ("seed", "draw", "s", "logw", "logw_b", "mu", "mu_b", "y", "y_b", "pair", "pair_b"),
    "bean_hip_log_weights_marginal": ("seed", "draw", "s", "q", "logw", "logw_b", "mu", "mu_b", "y", "y_b", "pair",
                                      "pair_b", "un", "un_b"),
    "bean_hip_marginal_grid": ("q", "n_mu", "n_y", "c_mu", "c_y", "s_mu", "s_y", "lj", "lj_b", "pair", "pair_b", "un",
                               "un_b"),
    "bean_hip_marginal_grid_tail": ("q", "n_mu", "n_y", "c_mu", "c_y", "s_mu", "s_y", "lj", "lj_b", "pair", "pair_b",
                                    "un", "un_b", "te", "te_b"),
    "bean_hip_marginal_tail_nodes": ("cap", "pidx", "z", "lw", "side", "count"),
}
BUFFERS = ("x", "xbc", "alpha", "logw", "mu", "y", "pair", "un", "lj", "te", "pidx", "z", "lw", "side")


def _dbl(*v):
    return (ctypes.c_double * len(v))(*v)


def _table(R, B, G, T):
    """(entry point, handle, overrides of the good arguments, the message after the entry point's name)."""
    one = 4 * R * B * G
    nan, inf = float("nan"), float("inf")
    rows = []

    def add(entry, handle, message, **over):
        rows.append((entry, handle, over, message))

    # ---- the four simulators
    for entry, planes, shape in (
            ("bean_hip_simulate", 1, "(R, B, G) float32"),
            ("bean_hip_simulate_members", K, f"(K, R, B, G) float32 with K = {K}"),
            ("bean_hip_simulate_design", D * K, f"(D, K, R, B, G) float32 with D = {D}, K = {K}"),
            ("bean_hip_simulate_power", D * K, f"(D, K, R, B, G) float32 with D = {D}, K = {K}")):
        full = planes * one
        held = f"{shape}, {full} bytes"
        add(entry, None, ": null handle")
        add(entry, None, ": null handle", x=None, x_b=0)
        add(entry, "members", SIM)
        add(entry, "members", SIM, x=None, xbc_b=full + 4)
        add(entry, "unprepared", PREPARE, xbc=None, xbc_b=0)
        add(entry, "unprepared", PREPARE, x=None)  # (and xbc_out on a handle without the flag)
        add(entry, "mix", ": x_out must hold " + held, x_b=full - 4)
        add(entry, "mix", ": x_out must hold " + held, x_b=full + one)
        add(entry, "mix", ": x_out must hold " + held, x=None)
        add(entry, "mix", ": x_out must hold " + held, x=None, x_b=0)
        add(entry, "mix", ": x_out must hold " + held, x_b=full - 4, xbc_b=full - 4)
        add(entry, "mix", HAS_BC + held, xbc_b=full + 4)
        add(entry, "mix", HAS_BC + held, xbc=None)
        add(entry, "mix", HAS_BC + held, xbc=None, xbc_b=0)
        add(entry, "nobc", NO_BC)
        add(entry, "nobc", NO_BC, xbc=None, xbc_b=4)
        add(entry, "nobc", NO_BC, xbc_b=0)
        add(entry, "nobc", ": x_out must hold " + held, x_b=full - 4)  # x_out comes before xbc_out
    e = "bean_hip_simulate"
    alpha = f": alpha_out must be null or hold (2, R, B, G) float64, {4 * one} bytes"
    add(e, "mix", alpha, alpha_b=4 * one - 8)
    add(e, "mix", alpha, alpha=None, alpha_b=4 * one)
    add(e, "mix", HAS_BC + f"(R, B, G) float32, {one} bytes", xbc_b=0, alpha_b=8)  # xbc_out comes before alpha_out
    e = "bean_hip_simulate_members"
    for k in (0, -1, 65):
        add(e, "mix", f": n_draws must be in [1, 64], got {k}", k=k)
    add(e, "mix", ": n_draws must be in [1, 64], got 0", k=0, x=None)  # n_draws comes before the buffers
    add(e, "unprepared", PREPARE, k=0, xbc=None, xbc_b=0)  # ... and after the handle
    for e, what, bad, values in (
            ("bean_hip_simulate_design", "depths", "is not a finite factor > 0",
             ((0.0, "0.000000"), (-1.5, "-1.500000"), (nan, "nan"), (inf, "inf"), (-inf, "-inf"))),
            ("bean_hip_simulate_power", "effects", "is not a finite number", ((nan, "nan"), (inf, "inf"), (-inf, "-inf")))):
        add(e, "mix", f": {what} is null", vals=None)
        add(e, "mix", f": {what} is null", vals=None, d=0)  # the array comes before its length
        for d, k in ((2, 0), (2, -1), (0, 5), (-1, 5), (13, 5), (1, 65)):
            add(e, "mix", f": n_{what} >= 1, n_draws >= 1 and n_{what} * n_draws <= 64, got {d} x {k} = {d * k}",
                vals=_dbl(*[1.0 + i for i in range(max(d, 1))]), d=d, k=k)
        add(e, "mix", f": n_{what} >= 1, n_draws >= 1 and n_{what} * n_draws <= 64, got 0 x 3 = 0", vals=_dbl(nan), d=0)
        for v, text in values:
            add(e, "mix", f": {what}[1] = {text} {bad}", vals=_dbl(0.5, v))
            add(e, "mix", f": {what}[0] = {text} {bad}", vals=_dbl(v, v), x=None)  # the values come before the buffers
        add(e, "unprepared", PREPARE, vals=None, xbc=None, xbc_b=0)
    # ---- the importance weights
    nt, npair = 8 * S * T, 8 * S * R * G
    sn = f" float64 with n_draws = {S}, "
    for e, stem in (("bean_hip_log_weights", LOGW), ("bean_hip_log_weights_marginal", LOGW)):
        marg = e.endswith("marginal")
        add(e, None, ": null handle")
        add(e, "members", stem)
        add(e, "members", stem, s=0)
        add(e, "unprepared", PREPARE)
        add(e, "unprepared", PREPARE, s=0)
        for s in (0, -1, 4097):
            add(e, "mix", f": n_draws must be in [1, 4096], got {s}", s=s)
        add(e, "mix", ": n_draws must be in [1, 4096], got 0", s=0, logw=None)
        logw = f": logw_out must hold (n_draws, T){sn}{nt} bytes"
        mu = f": mu_out must hold (n_draws, T){sn}{nt} bytes"
        y = f": y_out must be null or hold (n_draws, T){sn}{nt} bytes"
        pair = f": pair_out (caller-owned scratch) must hold (n_draws, R, G){sn}{npair} bytes"
        add(e, "mix", logw, logw_b=nt - 8)
        add(e, "mix", logw, logw=None)
        add(e, "mix", logw, logw_b=nt + 8, mu_b=0, y_b=0, pair_b=0)  # logw, mu, y, pair in this order
        add(e, "mix", mu, mu_b=nt + 8)
        add(e, "mix", mu, mu=None, y_b=0, pair_b=0)
        add(e, "mix", y, y_b=nt - 8)
        add(e, "mix", y, y=None)
        add(e, "mix", y, y_b=0, pair=None)
        add(e, "mix", pair, pair_b=npair - 8)
        add(e, "mix", pair, pair=None, pair_b=0)
        if marg:
            un = f": unresolved_out must hold (T) int32, {4 * T} bytes"
            for q in (20, 0, 128):
                add(e, "mix", f": n_nodes must be 16, 32 or 64, got {q}", q=q)
            add(e, "mix", ": n_draws must be in [1, 4096], got 0", s=0, q=20)  # n_draws comes before n_nodes
            add(e, "mix", ": n_nodes must be 16, 32 or 64, got 20", q=20, logw=None)  # ... and n_nodes before the buffers
            add(e, "mix", un, un_b=4 * T + 4)
            add(e, "mix", un, un=None, un_b=0)
            add(e, "mix", pair, pair_b=0, un=None)  # pair_out comes before unresolved_out
    # ---- the grid posterior
    nl, ngp = 8 * N * T, 8 * N * R * G
    sn = f" float64 with N = n_mu * n_y = {N}, "
    for e in ("bean_hip_marginal_grid", "bean_hip_marginal_grid_tail"):
        add(e, None, ": null handle")
        add(e, "members", GRID)
        add(e, "members", GRID, q=20)
        add(e, "unprepared", PREPARE)
        add(e, "acc_unprepared", PREPARE)  # the prepare comes before the accessibility
        add(e, "acc", ACC)
        add(e, "acc", ACC, q=20, n_mu=0)
        for q in (20, 0, 128):
            add(e, "mix", f": n_nodes must be 16, 32 or 64, got {q}", q=q)
        add(e, "mix", ": n_nodes must be 16, 32 or 64, got 20", q=20, n_mu=0)  # n_nodes comes before the grid's size
        for nm, ny in ((0, 2), (3, 0), (-1, 2), (65, 64)):
            add(e, "mix", f": n_mu >= 1, n_y >= 1 and n_mu * n_y <= 4096, got {nm} x {ny} = {nm * ny}", n_mu=nm, n_y=ny)
        add(e, "mix", ": n_mu >= 1, n_y >= 1 and n_mu * n_y <= 4096, got 0 x 2 = 0", n_mu=0, c_mu=None)
        for key in ("c_mu", "c_y", "s_mu", "s_y"):
            add(e, "mix", CENTRES, **{key: None})
        add(e, "mix", CENTRES, s_y=None, lj_b=0)  # the centres and steps come before the buffers
        lj = f": lj_out must hold (N, T){sn}{nl} bytes"
        pair = f": pair_out (caller-owned scratch) must hold (N, R, G){sn}{ngp} bytes"
        un = f": unresolved_out must hold (T) int32 (N = {N}), {4 * T} bytes"
        add(e, "mix", lj, lj_b=nl - 8)
        add(e, "mix", lj, lj=None)
        add(e, "mix", lj, lj_b=0, pair_b=0, un_b=0)  # lj, pair, unresolved in this order
        add(e, "mix", pair, pair_b=ngp + 8)
        add(e, "mix", pair, pair=None, un=None)
        add(e, "mix", un, un_b=4 * T - 4)
        add(e, "mix", un, un=None)
        if e.endswith("tail"):
            te = f": tail_err_out must hold (N, T){sn}{nl} bytes"
            add(e, "mix", te, te_b=nl + 8)
            add(e, "mix", te, te=None)
            add(e, "mix", un, un_b=0, te=None)  # unresolved_out comes before tail_err_out
    e = "bean_hip_marginal_tail_nodes"
    add(e, None, ": null handle")
    add(e, "members", GRID)
    add(e, "members", GRID, count=None)
    add(e, "unprepared", PREPARE)
    add(e, "acc_unprepared", PREPARE)
    add(e, "acc", ACC)
    add(e, "acc", ACC, cap=-1)
    add(e, "mix", ": n_tail_out is null", count=None)
    add(e, "mix", ": n_tail_out is null", count=None, cap=-1)  # n_tail_out comes before the capacity
    add(e, "mix", ": capacity must not be negative, got -1", cap=-1)
    add(e, "mix", ": capacity must not be negative, got -5", cap=-5, z=None)
    for key in ("pidx", "z", "lw", "side"):
        add(e, "mix", ": with capacity > 0, pair_index_out, z_out, lw_out and side_out must not be null", **{key: None})
    return rows


def test_every_refusal_to_the_letter():
    from bean_amd import engine

    data = make_sorting_variant_screen(40, 2, seed=1).to(DEV)
    acc_data = make_sorting_variant_screen(40, 2, seed=1, with_accessibility=True).to(DEV)
    lib = _lib.load()
    R, B, G, T = data.n_reps, data.n_condits, data.n_guides, data.n_targets
    one = R * B * G

    engines = {
        "mix": engine.HipSVI("MixtureNormal", data, num_steps=10),
        "nobc": engine.HipSVI("MixtureNormal", data, num_steps=10, use_bcmatch=False),
        "members": engine.HipSVI("MixtureNormal", data, num_steps=10, n_members=2),
        "acc": engine.HipSVI("MixtureNormal", acc_data, num_steps=10, scale_by_accessibility=True, fit_noise=True),
    }
    assert engines["mix"].use_bcmatch and not engines["nobc"].use_bcmatch
    handles = {k: (v._h, v._sptr()) for k, v in engines.items()}
    handles[None] = (None, None)
    raw = {}
    for name, of in (("unprepared", "nobc"), ("acc_unprepared", "acc")):  # unprepared handles of the same shapes
        raw[name] = ctypes.c_void_p()
        assert lib.bean_hip_create(ctypes.byref(engines[of]._shape), ctypes.byref(raw[name])) == 0
        assert lib.bean_hip_predictive_supported(raw[name]) == 1
        handles[name] = (raw[name], None)

    f32 = lambda n: torch.full((n,), float(FILL), dtype=torch.float32, device=DEV)  # noqa: E731
    f64 = lambda n: torch.full((n,), float(FILL), dtype=torch.float64, device=DEV)  # noqa: E731
    i32 = lambda n: torch.full((n,), FILL, dtype=torch.int32, device=DEV)  # noqa: E731
    bufs = {"x": f32(D * K * one), "xbc": f32(D * K * one), "alpha": f64(2 * one), "logw": f64(S * T), "mu": f64(S * T),
            "y": f64(S * T), "pair": f64(N * R * G), "un": i32(T), "lj": f64(N * T), "te": f64(N * T), "pidx": i32(4),
            "z": f64(4 * _lib.TAIL_NODES), "lw": f64(4 * _lib.TAIL_NODES), "side": i32(4)}
    assert set(bufs) == set(BUFFERS)
    grid = {k: torch.full((T,), v, dtype=torch.float64, device=DEV)
            for k, v in (("c_mu", 0.0), ("c_y", 0.0), ("s_mu", 0.1), ("s_y", 0.1))}
    count = ctypes.c_int32(FILL)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def good(entry):
        planes = {"bean_hip_simulate": 1, "bean_hip_simulate_members": K}.get(entry, D * K)
        g = {"seed": SEED, "draw": 0, "k": K, "d": D, "plant": None, "s": S, "q": 32, "n_mu": N_MU, "n_y": N_Y, "cap": 4,
             "vals": _dbl(0.5, 2.0), "count": ctypes.byref(count),
             "x_b": 4 * planes * one, "xbc_b": 4 * planes * one, "alpha_b": 16 * one,
             "logw_b": 8 * S * T, "mu_b": 8 * S * T, "y_b": 8 * S * T, "un_b": 4 * T, "lj_b": 8 * N * T, "te_b": 8 * N * T,
             "pair_b": 8 * (N if "grid" in entry else S) * R * G}
        g.update({k: ptr(v) for k, v in bufs.items()})
        g.update({k: ptr(v) for k, v in grid.items()})
        return g

    def call(entry, handle, over):
        h, stream = handles[handle]
        args = dict(good(entry), **over)
        return getattr(lib, entry)(h, *[args[k] for k in ARGS[entry]], stream)

    def untouched():
        torch.cuda.synchronize()
        return count.value == FILL and all(bool((b == FILL).all()) for b in bufs.values())

    rows = _table(R, B, G, T)
    assert {r[0] for r in rows} == set(ARGS)
    for entry, handle, over, message in rows:
        what = f"{entry}({handle}, {over})"
        assert call(entry, handle, over) < 0, what
        assert lib.bean_hip_last_error().decode() == entry + message, what
        assert untouched(), what

    # the handles are as usable as before the refused calls
    for entry in ARGS:
        over = {"cap": 0} if entry.endswith("tail_nodes") else {}  # (the count query: any number of tail pairs passes)
        no_bc = {"xbc": None, "xbc_b": 0} if "simulate" in entry else {}
        assert call(entry, "mix", over) == 0, (entry, lib.bean_hip_last_error().decode())
        assert call(entry, "nobc", dict(over, **no_bc)) == 0, (entry, lib.bean_hip_last_error().decode())
    torch.cuda.synchronize()
    assert count.value >= 0 and not bool((bufs["x"] == FILL).any()) and not bool((bufs["lj"] == FILL).any())
    for h in raw.values():
        assert lib.bean_hip_destroy(h) == 0
    for eng in engines.values():
        eng.run(3, seed=SEED) if eng.n_members == 1 else eng.run_ensemble(3, [SEED, SEED + 1])
        torch.cuda.synchronize()
        eng.close()
