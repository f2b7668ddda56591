"""k_svi_async prepares an item before its dependencies are met (csrc/bean_async_v2.hpp, "prepare"; guide_wave2_prepare /
guide_wave2_stage / guide_wave2_rest in csrc/bean_guide_v2.hpp): the loads of everything no wave of the launch writes are
issued - and put into the wave's LDS - before the wave polls, the rest runs after the poll has matched.  Same loads,
same arithmetic: BEAN_HIP_STEP=pair against =async as in test_gpu_async.py, at the places where a prepared item can go
wrong - an item whose wait ended in a stolen finish (which uses the same LDS) and is prepared again; the clamped
addresses at the ends of a shard, a target that straddles two tiles; every static input that has a second code path;
state across launches.

What is compared: parameters and both ClippedAdam moments bit for bit.  The loss history of the two PATHS agrees to the
2^-40 granule of its fixed-point parts, as test_gpu_async.py's header explains (the prior / entropy terms of a tile's
targets are rounded to the granule per finishing wave here and per block of k_param there: 1e-12 relative is that
granule, not a tolerance of the arithmetic); bit for bit it is compared where it can be - the asynchronous run against a
second asynchronous run on another grid, every finish by the last arriver.  -m gpu."""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENV = ("BEAN_HIP_ASYNC_BLOCKS", "BEAN_HIP_ASYNC_FIN", "BEAN_HIP_ASYNC_SPLIT")


def _fit(monkeypatch, mode, family, data, steps, eng_kw=None, chunks=None, resume=False, grid=None, shard=None,
         n_total=0):
    from bean_amd import engine

    monkeypatch.setenv("BEAN_HIP_STEP", mode)
    for key, val in zip(ENV, grid or (None, None, None)):
        if val is not None and mode == "async":
            monkeypatch.setenv(key, str(val))
        else:
            monkeypatch.delenv(key, raising=False)
    kw = dict(eng_kw or {})
    if shard is not None:
        kw.update(guide_offset=shard[0], target_offset=shard[2], n_guides_total=n_total)
    eng = engine.HipSVI(family, data.to(DEV), num_steps=steps, **kw)
    assert eng.dominant_kernel == ("k_guide_wave2" if mode == "pair" else "k_svi_async")
    for n in (chunks or [steps]):
        eng.run(n, seed=5, resume=resume)
    torch.cuda.synchronize()
    out = {}
    for name, group in (("p", eng.unconstrained), ("m", eng._m), ("v", eng._v)):
        for k, v in group.items():
            out[f"{name}.{k}"] = v.detach().cpu().clone()
    loss = np.array(eng.losses())
    eng.close()
    return out, loss


def _check(a, la, b, lb, lb2, steps):
    assert np.all(np.isfinite(la)) and len(la) == steps == len(lb)
    print("max |loss pair - loss async| / |loss| =", float(np.max(np.abs(la - lb) / np.abs(la))))
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())
    assert np.max(np.abs(la - lb) / np.abs(la)) < 1e-12
    assert np.array_equal(lb, lb2)


def _same(monkeypatch, family, data, steps, eng_kw=None, grid=None, pair_chunks=None, async_chunks=None, resume=False,
          shard=None, n_total=0):
    a, la = _fit(monkeypatch, "pair", family, data, steps, eng_kw, pair_chunks, resume, None, shard, n_total)
    b, lb = _fit(monkeypatch, "async", family, data, steps, eng_kw, async_chunks, resume, grid, shard, n_total)
    # (the loss history, bit for bit: the same fit on another grid - few waves, every finish by the tile's last arriver)
    _, lb2 = _fit(monkeypatch, "async", family, data, steps, eng_kw, async_chunks, resume, (16, 0, None), shard, n_total)
    _check(a, la, b, lb, lb2, steps)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("blocks", [8, 64])
def test_item_is_prepared_again_after_a_stolen_finish(monkeypatch, blocks, split):
    """Roles on and no finisher resident: every finish is taken by an item wave that waits (it prepared its item, staged
    it, and now runs a finish over the same LDS) or is done after the items have run out."""
    data = make_sorting_variant_screen(461, 3, seed=901, guides_per_target=7)
    _same(monkeypatch, "MixtureNormal", data, 25, grid=(blocks, -1, split))


@pytest.mark.parametrize("n_reps", [1, 5])
def test_edges_of_the_clamped_static_loads(monkeypatch, n_reps):
    """Shards of a screen whose guide count is no multiple of 64: the second starts inside a tile (its first tile is
    partly empty, the lanes in front of its first guide read guide 0's values), both end inside one; three guides per
    target, so targets straddle tile boundaries (the first target of a tile began in the tile before)."""
    from bean_amd import parallel

    data = make_sorting_variant_screen(500, n_reps, seed=902 + n_reps, guides_per_target=3,
                                       mask_fraction=0.05 if n_reps > 1 else 0.0)
    shards = parallel.plan_shards(data.target_lengths.numpy(), 2)
    assert data.n_guides % 64 != 0 and shards[1][0] % 64 != 0
    off = data.target_offsets.numpy()
    assert any(o % 64 != 0 and o // 64 != (o2 - 1) // 64 for o, o2 in zip(off[:-1], off[1:]))  # a straddling target
    for sh in shards:
        _same(monkeypatch, "MixtureNormal", parallel.shard_screen(data, sh), 20, shard=sh, n_total=data.n_guides)


@pytest.mark.parametrize("n_bins,n_guides", [(11, 300), (19, 280)])
def test_more_conditions_than_the_register_batch(monkeypatch, n_bins, n_guides):
    """12 conditions: the per-bin constants are staged in two rounds (bins 8 ...); 20: the counts of the conditions
    beyond the 16 the register batch holds are loaded where they are staged."""
    edges = np.linspace(0, 1, n_bins + 1)
    bins = tuple((float(edges[i]), float(edges[i + 1])) for i in range(n_bins))
    data = make_sorting_variant_screen(n_guides, 2, bins=bins, seed=903 + n_bins, guides_per_target=4)
    assert data.n_condits == n_bins + 1
    _same(monkeypatch, "MixtureNormal", data, 20)


def test_control_conditions(monkeypatch):
    """Two control conditions (the second one's allele counts are read where the counts are staged), and none: a
    MixtureNormal fit needs at least one (bean_hip_create), so the kernel sees C = 0 with the Normal family only."""
    data = make_sorting_variant_screen(333, 2, seed=905, guides_per_target=5)
    second = torch.flip(data.allele_counts_control, dims=[2]) + 1.0
    data.allele_counts_control = torch.cat([data.allele_counts_control, second], dim=1).contiguous()
    assert data.allele_counts_control.shape[1] == 2
    _same(monkeypatch, "MixtureNormal", data, 20)
    _same(monkeypatch, "Normal", make_sorting_variant_screen(333, 2, seed=905, guides_per_target=5), 20)


@pytest.mark.parametrize("family,kw,acc,mask", [
    ("MixtureNormal", dict(use_bcmatch=False), False, 0.0),
    ("Normal", dict(use_bcmatch=False), False, 0.0),
    ("MixtureNormal", dict(scale_by_accessibility=True), True, 0.0),
    ("MixtureNormal", {}, False, 0.1),
])
def test_static_inputs_with_a_second_path(monkeypatch, family, kw, acc, mask):
    """Without the barcode-matched likelihood (zeros staged in its place), with the accessibility transform (kacc is
    static, the noise draw is not), with masked (replicate, guide) pairs and a masked sample."""
    data = make_sorting_variant_screen(300, 3, seed=906, guides_per_target=4, with_accessibility=acc, mask_fraction=mask)
    _same(monkeypatch, family, data, 20, kw)


def test_three_resumed_windows_are_one_call(monkeypatch):
    """The first items of a launch have no previous step in it: they take the same path and poll nothing.  Three
    resumed windows of 7 steps against ONE call of 21 on the pair path."""
    data = make_sorting_variant_screen(461, 3, seed=907, guides_per_target=7, mask_fraction=0.05)
    _same(monkeypatch, "MixtureNormal", data, 21, async_chunks=[7, 7, 7], resume=True)
