"""Count planes at the read depths a depth study hands to a refit, for the oracle-parity tests (test_count_regimes.py on
the host, test_gpu_count_regimes.py on the device).  A plain module imported by bare name; nothing here is code under
test and nothing here looks at a device.

``rewrite_counts(data, regime)`` returns a copy of a screen with ``X``, ``X_masked``, ``X_bcmatch`` and
``X_bcmatch_masked`` replaced and everything a depth study conditions on left as it is (the same tensor objects): size
factors, ``a0``, ``a0_bcmatch``, ``pi_a0``, ``allele_counts_control``, both masks, bounds, the tiling tables.  A pair is
a (replicate, guide); its total is the sum over the conditions.  Every plane is integer-valued float32, every pair total
at most 2^24 - 1 (``CAP``: the simulator's clamp and the last count float32 holds exactly next to its neighbours); the
barcode-matched plane is ``floor(0.8 X + 0.5)``.

* ``deep``: ``floor(f X + 0.5)`` with the screen's largest pair total exactly ``CAP`` (the rounding of that pair is
  settled in its largest bin; any other pair that rounding pushes over is cut back in its largest bin).
* ``shallow``: ``floor(f X + 0.5)`` with the smallest ``f`` whose median pair total reaches 12: bins of 0 ... 12 (the
  exact product form of ``lgamma_digamma_diff_inl``), totals on both sides of the ``> 10`` mask threshold.
* ``mixed``: guides 0 ... 63 deep; from guide 64 on even guides deep, odd guides shallow - waves that hold both kinds of
  lane next to waves that hold only deep ones.  The deep guides' bins are raised to at least 13 (a bin the screen has
  at 0 stays 0 under ``deep``), so that no lane of an all-deep wave sends it through the one-chain function.
* ``edges``: the screen's own depth; bin ``g mod B`` of guide ``g`` set to the ``(g div B) mod 4``-th of {0, 1, 12, 13}
  in every replicate; and the last three guides that ``repguide_mask`` keeps in every replicate are, in this order, a
  guide with a pair total of exactly 11 (kept), one with exactly 10 (masked by the ``> 10`` rule) and one with all
  ``CAP`` reads in bin 0.  ``repguide_mask`` is conditioned on, so zero bins stay inside pairs it keeps.

``generated_deep(maker, **gen_kw)`` is no rewrite: the generator itself at ``depth_per_guide = 2e5`` (pair totals of
1e6 ... 4e6, a refitted ``a0`` of 1.5e4 ... 1e6 - both arguments of the count likelihood large).  Its ``pi_a0`` is
clamped to ``PI_A0_MAX = 2e3``: the generators give up to 7e4 there, and above concentrations of 2e3 torch's implicit
Dirichlet gradient - the oracle's - is up to 6e-8 off the formula it evaluates (1e-5 in the small-beta series: its own
rounding inside cancelling intermediates, tests/dirichlet_grad_reference.py), so it cannot serve as the reference, and
the constants of grad_bounds.py were pinned on [1e-3, 2e3] only.

``generated_deep_unclamped(maker, **gen_kw)`` is that screen with ``pi_a0`` as the generator gives it.  Its tests take
``dirichlet_grad_reference.port64`` as the oracle's implicit gradient and hold each evaluation to the error budget of
its own inputs (tests/dirichlet_grad_reference.py) in place of the two pathwise constants.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import grad_bounds as gb

CAP = (1 << 24) - 1
MASK_THRES = 10
PI_A0_MAX = 2e3
DEEP_DEPTH = 2e5
REGIMES = ("deep", "shallow", "mixed", "edges")
EDGE_VALUES = (0.0, 1.0, 12.0, 13.0)
COUNT_PLANES = ("X", "X_masked", "X_bcmatch", "X_bcmatch_masked")


def pair_totals(x) -> np.ndarray:
    """(R, G) float64 totals of an (R, B, G) plane."""
    return np.asarray(x, dtype=np.float64).sum(1)


def _scaled(x: np.ndarray, f: float) -> np.ndarray:
    return np.floor(f * x + 0.5)


def _deep(x: np.ndarray) -> np.ndarray:
    n = pair_totals(x)
    r, g = np.unravel_index(int(np.argmax(n)), n.shape)
    out = _scaled(x, CAP / n[r, g])
    tot = out.sum(1)
    out[r, int(np.argmax(out[r, :, g])), g] += CAP - tot[r, g]
    return _cut_to_cap(out)


def _cut_to_cap(out: np.ndarray) -> np.ndarray:
    tot = out.sum(1)
    for rr, gg in zip(*np.nonzero(tot > CAP)):
        out[rr, int(np.argmax(out[rr, :, gg])), gg] -= tot[rr, gg] - CAP
    return out


def _shallow(x: np.ndarray) -> np.ndarray:
    lo, hi = 0.0, 24.0 / max(float(np.median(pair_totals(x))), 1.0)
    for _ in range(60):  # the median total is monotone in f
        mid = 0.5 * (lo + hi)
        if float(np.median(_scaled(x, mid).sum(1))) >= 12.0:
            hi = mid
        else:
            lo = mid
    return _scaled(x, hi)


def _spread(total: int, B: int) -> np.ndarray:
    out = np.zeros(B)
    for i in range(total):
        out[i % B] += 1.0
    return out


def edge_guides(data):
    """(kept, masked, one_bin): the last three guides that ``repguide_mask`` keeps in every replicate."""
    ok = np.nonzero(data.repguide_mask.cpu().numpy().all(0))[0]
    assert len(ok) >= 3, "the screen has fewer than three guides kept in every replicate"
    return int(ok[-3]), int(ok[-2]), int(ok[-1])


def _edges(x: np.ndarray, data) -> np.ndarray:
    out = x.copy()
    R, B, G = out.shape
    for g in range(G):
        out[:, g % B, g] = EDGE_VALUES[(g // B) % 4]
    kept, masked, one_bin = edge_guides(data)
    out[:, :, kept] = _spread(MASK_THRES + 1, B)[None]
    out[:, :, masked] = _spread(MASK_THRES, B)[None]
    out[:, :, one_bin] = 0.0
    out[:, 0, one_bin] = float(CAP)
    return out


def with_counts(data, x):
    """A copy of ``data`` whose four count planes come from the (R, B, G) integer-valued plane ``x``: the
    barcode-matched plane is floor(0.8 x + 0.5), the masked planes are those times ``sample_mask``; every other
    attribute is the object ``data`` holds."""
    x = np.asarray(x, dtype=np.float64)
    assert np.array_equal(x, np.floor(x)) and x.min() >= 0 and x.sum(1).max() <= CAP
    out = copy.copy(data)
    dev = data.X.device
    xt = torch.as_tensor(x, dtype=torch.float32, device=dev)
    xbc = torch.as_tensor(np.floor(0.8 * x + 0.5), dtype=torch.float32, device=dev)
    sm = data.sample_mask[:, :, None].to(torch.float32)
    out.X, out.X_masked = xt, xt * sm
    out.X_bcmatch, out.X_bcmatch_masked = xbc, xbc * sm
    return out


def rewrite_counts(data, regime: str):
    x = data.X.detach().cpu().double().numpy()
    if regime == "deep":
        new = _deep(x)
    elif regime == "shallow":
        new = _shallow(x)
    elif regime == "mixed":
        deep, shallow = _cut_to_cap(np.maximum(_deep(x), 13.0)), _shallow(x)
        g = np.arange(x.shape[2])
        new = np.where(((g >= 64) & (g % 2 == 1))[None, None, :], shallow, deep)
    elif regime == "edges":
        new = _edges(x, data)
    else:
        raise ValueError(f"unknown regime {regime!r}: one of {REGIMES}")
    return with_counts(data, new)


def generated_deep(maker, **gen_kw):
    """The generator's own screen at ``DEEP_DEPTH`` reads per guide, ``pi_a0`` clamped to ``PI_A0_MAX`` (see the module
    docstring for why the clamp is there)."""
    gen_kw = dict(gen_kw, depth_per_guide=DEEP_DEPTH)
    data = maker(**gen_kw)
    data.pi_a0 = data.pi_a0.clamp(max=PI_A0_MAX)
    return data


def generated_deep_unclamped(maker, **gen_kw):
    """The generator's own screen at ``DEEP_DEPTH`` reads per guide, ``pi_a0`` as generated (up to 7e4)."""
    return maker(**dict(gen_kw, depth_per_guide=DEEP_DEPTH))


def regime_screen(maker, gen_kw, regime: str):
    """The screen of a regime name: one of ``REGIMES`` rewrites ``maker(**gen_kw)``, ``generated_deep`` and
    ``generated_deep_unclamped`` generate."""
    if regime == "generated_deep":
        return generated_deep(maker, **gen_kw)
    if regime == "generated_deep_unclamped":
        return generated_deep_unclamped(maker, **gen_kw)
    return rewrite_counts(maker(**gen_kw), regime)


# ---------------------------------------------------------------- draws for the host tests
def host_noise(kind: str, data, params, kw=None, seed: int = 5):
    """The draws of one ELBO evaluation, made on the host with torch's samplers (the device tests use the engine's own
    dumped draws): float64, Dirichlet draws floored where the device floors its own (DBL_MIN for pi, FLT_MIN for the
    survival families' initial abundance) and renormalised."""
    kw = kw or {}
    g = torch.Generator().manual_seed(seed)
    randn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)  # noqa: E731
    R, G = data.n_reps, data.n_guides
    survival = kind.startswith("survival")
    shape = tuple(params["mu_loc"].shape)
    noise = {"eps_mu": randn(*shape)}
    if not survival:
        noise["eps_sd"] = randn(*shape)
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        if "alpha_pi" in params:
            c, _ = gb.variational_concentrations(data, params["alpha_pi"], survival)
            pi = torch.distributions.Dirichlet(c[None, None].expand(R, 1, -1, -1)).sample().clamp(min=2.3e-308)
            noise["pi"] = pi / pi.sum(-1, keepdim=True)
        if "q0" in params:
            q0 = params["q0"].detach().double().exp()
            x0 = torch.distributions.Dirichlet(q0[None].expand(R, -1)).sample().clamp(min=1.17549435e-38)
            noise["initial_abundance"] = x0 / x0.sum(-1, keepdim=True)
    finally:
        torch.random.set_rng_state(state)
    if survival:
        noise["mu_negctrl"] = 0.1 * randn(G)
    if kw.get("scale_by_accessibility"):
        noise["eps_noise"] = randn(G)
    return noise
