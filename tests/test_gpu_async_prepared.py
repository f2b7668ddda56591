"""k_svi_async with finish positions known in advance (csrc/bean_async_v2.hpp): position p of a group's finish sequence
stands for a fixed (step, tile, part), a finisher that takes p prepares the tile's finish before the tile's last wave has
arrived, and the wave that completes a tile fills that tile's slot(s).  None of this may change a bit: the fitted
parameters must equal the two launches per step (BEAN_HIP_STEP=pair) exactly - on the smallest shapes that reach every
path of the finish (one tile without neighbours and several passes of 16 targets; targets that straddle one or both
boundaries of a tile; tiles that end inside a group of 64; empty lanes at the head of a shard's first tile), with and
without finisher roles, with the finish as one or two positions, with so few resident waves that positions are taken
long before they are filled and waiting item waves take the filled ones, over windows of 1, 2, 3 steps and a resumed
chain, and with the accessibility noise site.  Every case is at most 40 steps of at most 500 guides.  -m gpu."""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 40
KNOBS = ("BEAN_HIP_ASYNC_BLOCKS", "BEAN_HIP_ASYNC_FIN", "BEAN_HIP_ASYNC_SPLIT")

# guides, replicates, guides per target
SHAPES = {
    "one_tile": (64, 1, 1),        # one tile, no neighbour; 64 targets: four passes of 16, three of them not prepared
    "straddle": (200, 2, 3),       # targets straddle both boundaries of the middle tiles
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


def _fit(monkeypatch, mode, data, chunks, resume=False, knobs=None, eng_kw=None, **shard_kw):
    from bean_amd import engine

    monkeypatch.setenv("BEAN_HIP_STEP", mode)
    for key in KNOBS:
        val = (knobs or {}).get(key)
        if val is None or mode == "pair":
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))
    eng = engine.HipSVI("MixtureNormal", data.to(DEV), num_steps=sum(chunks), **(eng_kw or {}), **shard_kw)
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


def _same(monkeypatch, name, chunks=(STEPS,), resume=False, acc=False, **knobs):
    ref, lref = _pair_fit(monkeypatch, name, chunks, resume, acc)
    got, lgot = _fit(monkeypatch, "async", _screen(name, acc), chunks, resume, knobs,
                     eng_kw=dict(scale_by_accessibility=True) if acc else None)
    assert np.all(np.isfinite(lref)) and len(lref) == sum(chunks) == len(lgot)
    for k in ref:
        assert torch.equal(ref[k], got[k]), (k, (ref[k] - got[k]).abs().max().item())
    assert np.max(np.abs(lref - lgot) / np.abs(lref)) < 1e-12


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_at_the_default_grid(monkeypatch, name):
    _same(monkeypatch, name)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("fin", [0, 8, 64, -1])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_finishers_and_finish_forms(monkeypatch, name, fin, split):
    """The last arriver finishes (0); dedicated finishers take positions in advance (8, 64: capped at the tiles); roles
    without a finisher (-1: waiting item waves take the oldest filled position, and join the finishers at the end)."""
    _same(monkeypatch, name, BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=split)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("fin", [8, -1])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_eight_resident_item_waves(monkeypatch, name, fin, split):
    """One item wave per group works through all R items of its tiles: a finisher holds its position for a whole item
    round before the slot is filled (fin = 8), and with no finisher resident (fin = -1) every finish is one that a
    waiting item wave has taken."""
    _same(monkeypatch, name, BEAN_HIP_ASYNC_BLOCKS=8, BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=split)


@pytest.mark.parametrize("chunks,resume", [((1,), False), ((2,), False), ((3,), False), ((1, 2, 3, 17, 17), True)])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_windows_and_a_resumed_chain(monkeypatch, name, chunks, resume):
    """A call's positions start at its own first step: windows of 1, 2, 3 steps, and a chain of resumed windows."""
    _same(monkeypatch, name, chunks=chunks, resume=resume, BEAN_HIP_ASYNC_FIN=8, BEAN_HIP_ASYNC_SPLIT=1)


@pytest.mark.parametrize("fin", [0, 8])
@pytest.mark.parametrize("name", ["straddle", "mixed"])
def test_with_accessibility(monkeypatch, name, fin):
    """The guides' part with the accessibility noise site."""
    _same(monkeypatch, name, acc=True, BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=1)


def test_loss_history_is_the_same_twice(monkeypatch):
    """Who finishes a straddling target depends on timing; the loss history must not."""
    data = _screen("straddle")
    knobs = dict(BEAN_HIP_ASYNC_FIN=8, BEAN_HIP_ASYNC_SPLIT=1)
    p1, l1 = _fit(monkeypatch, "async", data, (STEPS,), knobs=knobs)
    p2, l2 = _fit(monkeypatch, "async", data, (STEPS,), knobs=knobs)
    assert np.all(np.isfinite(l1)) and np.array_equal(l1, l2)
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k


@pytest.mark.parametrize("fin", [0, 8])
def test_a_shard_whose_offset_is_no_multiple_of_64(monkeypatch, fin):
    """Tiles follow the global guide index: the head lanes of the shard's first tile are empty."""
    from bean_amd import parallel

    # (two shards of 83 targets each: a shard of fewer than 64 targets takes the pair path whatever is asked for)
    data = make_sorting_variant_screen(498, 2, seed=911, guides_per_target=3, mask_fraction=0.05)
    shards = parallel.plan_shards(data.target_lengths.numpy(), 2)
    assert all(sh[0] % 64 for sh in shards[1:])
    for sh in shards[1:]:
        sub = parallel.shard_screen(data, sh)
        kw = dict(guide_offset=sh[0], target_offset=sh[2], n_guides_total=data.n_guides)
        ref, lref = _fit(monkeypatch, "pair", sub, (STEPS,), **kw)
        got, lgot = _fit(monkeypatch, "async", sub, (STEPS,),
                         knobs=dict(BEAN_HIP_ASYNC_FIN=fin, BEAN_HIP_ASYNC_SPLIT=1), **kw)
        for k in ref:
            assert torch.equal(ref[k], got[k]), (sh, k)
        assert np.max(np.abs(lref - lgot) / np.abs(lref)) < 1e-12
