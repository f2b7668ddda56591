"""k_svi_async with the targets' part of a finish started before the finisher's poll (csrc/bean_async_v2.hpp, "the
targets' part ahead of the poll"): a finisher that has taken a position stages the bin edges, the first pass's target
descriptors and next-draw normals in its LDS and - where the completed-step words of step s - 1 are seen at one look
(the gate) - the first pass's state and what follows from it alone, all before the tile's last wave has arrived.
None of this may change a bit: the fitted parameters must equal the two launches per step (BEAN_HIP_STEP=pair) exactly
and the loss history to its granule, on the smallest shapes that reach every path - one tile with four passes of which
only the first is prepared; straddlers on both boundaries (neighbour gates, a prepared target the boundary counter gives
away, a pass that starts at t0 + 1 and finds its slots four lanes up); more than 16 targets per tile; R = 5 with a
ragged last tile; a shard with empty head lanes - under BEAN_HIP_ASYNC_EARLY = 0 (nothing early), 1 (the default) and 2
(static inputs only: every gate counts as not open), with and without finisher roles, with the finish as one or two
positions, with eight resident item waves (finishers take positions steps ahead: the gate is really found closed; no
finisher: every finish is a stolen one and nothing is prepared early), over windows of 1, 2, 3 steps and a resumed chain
(the gate at a call's first step), with the accessibility noise site, and for every family the asynchronous path
accepts.  Every case is at most 40 steps of at most 500 guides.  -m gpu."""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 40
KNOBS = ("BEAN_HIP_ASYNC_BLOCKS", "BEAN_HIP_ASYNC_FIN", "BEAN_HIP_ASYNC_SPLIT", "BEAN_HIP_ASYNC_EARLY")
EARLY = [0, 1, 2]

# guides, replicates, guides per target
SHAPES = {
    "one_tile": (64, 1, 1),        # one tile, four passes of 16 targets: only the first is prepared early
    "straddle": (200, 2, 3),       # straddlers on both boundaries: neighbour gates, a discarded slot, a pass from t0 + 1
    "mixed": (461, 3, 7),          # straddling targets and more than 16 targets in a tile
    "five_reps": (130, 5, 1),      # R = 5 and a last tile that does not end at a multiple of 64
}
_screens, _pair = {}, {}


def _screen(name, acc=False):
    key = (name, acc)
    if key not in _screens:
        g, r, gpt = SHAPES[name]
        _screens[key] = make_sorting_variant_screen(g, r, seed=900 + g, guides_per_target=gpt, with_accessibility=acc,
                                                    mask_fraction=0.05 if r > 1 else 0.0)
    return _screens[key]


def _fit(monkeypatch, mode, data, chunks, resume=False, knobs=None, family="MixtureNormal", eng_kw=None, **shard_kw):
    from bean_amd import engine

    monkeypatch.setenv("BEAN_HIP_STEP", mode)
    for key in KNOBS:
        val = (knobs or {}).get(key)
        if val is None or mode == "pair":
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))
    eng = engine.HipSVI(family, data.to(DEV), num_steps=sum(chunks), **(eng_kw or {}), **shard_kw)
    assert eng.dominant_kernel == ("k_guide_wave2" if mode == "pair" else "k_svi_async")
    for n in chunks:
        eng.run(n, seed=5, resume=resume)
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
    loss = np.array(eng.losses())
    eng.close()
    return out, loss


def _pair_fit(monkeypatch, name, chunks, resume=False, acc=False):
    """The pair path's fit of a shape: computed once, shared by every case that compares against it, never changed."""
    key = (name, tuple(chunks), resume, acc)
    if key not in _pair:
        _pair[key] = _fit(monkeypatch, "pair", _screen(name, acc), chunks, resume,
                          eng_kw=dict(scale_by_accessibility=True) if acc else None)
    return _pair[key]


def _check(ref, lref, got, lgot, n):
    assert np.all(np.isfinite(lref)) and len(lref) == n == len(lgot)
    for k in ref:
        assert torch.equal(ref[k], got[k]), (k, (ref[k] - got[k]).abs().max().item())
    assert np.max(np.abs(lref - lgot) / np.abs(lref)) < 1e-12


def _same(monkeypatch, name, chunks=(STEPS,), resume=False, acc=False, **knobs):
    ref, lref = _pair_fit(monkeypatch, name, chunks, resume, acc)
    got, lgot = _fit(monkeypatch, "async", _screen(name, acc), chunks, resume, knobs,
                     eng_kw=dict(scale_by_accessibility=True) if acc else None)
    _check(ref, lref, got, lgot, sum(chunks))


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_at_the_default_grid(monkeypatch, name, early):
    _same(monkeypatch, name, BEAN_HIP_ASYNC_EARLY=early)


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("fin", [0, 8, 64, -1])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_finishers_and_finish_forms(monkeypatch, name, fin, split, early):
    """The last arriver finishes (0: nothing is early); dedicated finishers take positions in advance (8, 64: capped at
    the tiles); roles without a finisher (-1: waiting item waves take the oldest filled position and prepare inline)."""
    _same(monkeypatch, name, BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=split, BEAN_HIP_ASYNC_EARLY=early)


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("fin", [64, -1])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_eight_resident_item_waves(monkeypatch, name, fin, split, early):
    """One item wave per group works through all R items of its tiles.  With finishers (64, capped at the tiles) the
    positions are taken steps ahead of the items, so the gate is looked at long before step s - 1 is finished and is
    found closed: the state takes the late path behind early static inputs.  With no finisher resident (-1) every finish
    is one a waiting item wave has taken when it was already filled: prepare runs inline."""
    _same(monkeypatch, name, BEAN_HIP_ASYNC_BLOCKS=8, BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=split,
          BEAN_HIP_ASYNC_EARLY=early)


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("chunks,resume", [((1,), False), ((2,), False), ((3,), False), ((1, 2, 3, 17, 17), True)])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_windows_and_a_resumed_chain(monkeypatch, name, chunks, resume, early):
    """The gate at a call's first step is open by itself (the state comes from the previous call in stream order):
    windows of 1, 2, 3 steps, and a chain of resumed windows."""
    _same(monkeypatch, name, chunks=chunks, resume=resume, BEAN_HIP_ASYNC_FIN=8, BEAN_HIP_ASYNC_SPLIT=1,
          BEAN_HIP_ASYNC_EARLY=early)


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("fin", [0, 8])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_with_accessibility(monkeypatch, name, fin, early):
    """The accessibility noise site's state (the guides' part, beside an early targets' part)."""
    _same(monkeypatch, name, acc=True, BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=1, BEAN_HIP_ASYNC_EARLY=early)


def _families():
    data = make_sorting_variant_screen(461, 3, seed=978, guides_per_target=7, with_accessibility=True, mask_fraction=0.05)
    T = data.n_targets
    g = torch.Generator().manual_seed(0)
    prior = {
        "mu_loc": torch.randn((T, 1), generator=g, dtype=torch.float64) * 0.2,
        "mu_scale": torch.rand((T, 1), generator=g, dtype=torch.float64) + 0.5,
        "sd_loc": torch.randn((T, 1), generator=g, dtype=torch.float64) * 0.1,
        "sd_scale": torch.rand((T, 1), generator=g, dtype=torch.float64) * 0.05 + 0.01,
    }
    return data, {
        "mixture_acc": ("MixtureNormal", dict(scale_by_accessibility=True)),
        "mixture_acc_prior_noise": ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=False)),
        "normal": ("Normal", {}),
        "normal_no_bcmatch": ("Normal", dict(use_bcmatch=False)),
        "mixture_prior_params": ("MixtureNormal", dict(prior_params=prior)),  # the Normal prior on mu, per-target scales
    }


_fam_ref = {}


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("which", ["mixture_acc", "mixture_acc_prior_noise", "normal", "normal_no_bcmatch",
                                   "mixture_prior_params"])
def test_every_family_of_the_asynchronous_path(monkeypatch, which, early):
    data, fams = _families()
    family, kw = fams[which]
    if which not in _fam_ref:
        _fam_ref[which] = _fit(monkeypatch, "pair", data, (STEPS,), family=family, eng_kw=kw)
    ref, lref = _fam_ref[which]
    got, lgot = _fit(monkeypatch, "async", data, (STEPS,), family=family, eng_kw=kw,
                     knobs=dict(BEAN_HIP_ASYNC_FIN=8, BEAN_HIP_ASYNC_SPLIT=1, BEAN_HIP_ASYNC_EARLY=early))
    _check(ref, lref, got, lgot, STEPS)


@pytest.mark.parametrize("early", EARLY)
def test_loss_history_is_the_same_twice(monkeypatch, early):
    """Who finishes a straddling target - and whether its finisher found the gate open - depends on timing; the loss
    history must not."""
    data = _screen("straddle")
    knobs = dict(BEAN_HIP_ASYNC_FIN=8, BEAN_HIP_ASYNC_SPLIT=1, BEAN_HIP_ASYNC_EARLY=early)
    p1, l1 = _fit(monkeypatch, "async", data, (STEPS,), knobs=knobs)
    p2, l2 = _fit(monkeypatch, "async", data, (STEPS,), knobs=knobs)
    assert np.all(np.isfinite(l1)) and np.array_equal(l1, l2)
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k


_shard_ref = {}


@pytest.mark.parametrize("early", EARLY)
@pytest.mark.parametrize("fin", [0, 8])
def test_a_shard_whose_offset_is_no_multiple_of_64(monkeypatch, fin, early):
    """Tiles follow the global guide index: the head lanes of the shard's first tile are empty."""
    from bean_amd import parallel

    # (two shards of 83 targets each: a shard of fewer than 64 targets takes the pair path whatever is asked for)
    data = make_sorting_variant_screen(498, 2, seed=911, guides_per_target=3, mask_fraction=0.05)
    shards = parallel.plan_shards(data.target_lengths.numpy(), 2)
    assert all(sh[0] % 64 for sh in shards[1:])
    for sh in shards[1:]:
        sub = parallel.shard_screen(data, sh)
        kw = dict(guide_offset=sh[0], target_offset=sh[2], n_guides_total=data.n_guides)
        if tuple(sh) not in _shard_ref:
            _shard_ref[tuple(sh)] = _fit(monkeypatch, "pair", sub, (STEPS,), **kw)
        ref, lref = _shard_ref[tuple(sh)]
        got, lgot = _fit(monkeypatch, "async", sub, (STEPS,),
                         knobs=dict(BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=1, BEAN_HIP_ASYNC_EARLY=early), **kw)
        _check(ref, lref, got, lgot, STEPS)
