"""A fit with the implicit gradient's x-free factors tabulated once per guide and step (DevArgs::dgt, the default) and the
same fit with every call forming them itself (BEAN_HIP_DIRGRAD_TAB=0, read at create), in one build: every parameter array
and the loss history must be equal bit for bit - on the two launches per step, in k_svi_async with 8 resident item waves,
across a resumed window, with and without accessibility, and in the survival variant's wave kernel.  192 guides are
three tiles; with three guides per target (64 targets: k_svi_async needs that many) a target straddles each tile
boundary.  -m gpu."""
import numpy as np
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen, make_survival_variant_screen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIVE_BINS = ((0.0, 0.2), (0.2, 0.4), (0.4, 0.6), (0.6, 0.8), (0.8, 1.0))


def _fit(monkeypatch, tab, family, data, windows, resume, kw, mode, kernel, blocks=None):
    from bean_amd import engine

    if tab:
        monkeypatch.delenv("BEAN_HIP_DIRGRAD_TAB", raising=False)
    else:
        monkeypatch.setenv("BEAN_HIP_DIRGRAD_TAB", "0")
    if mode is None:
        monkeypatch.delenv("BEAN_HIP_STEP", raising=False)
    else:
        monkeypatch.setenv("BEAN_HIP_STEP", mode)
    if blocks is None:
        monkeypatch.delenv("BEAN_HIP_ASYNC_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("BEAN_HIP_ASYNC_BLOCKS", str(blocks))
    eng = engine.HipSVI(family, data.to(DEV), num_steps=sum(windows), **kw)
    assert eng.dominant_kernel == kernel, eng.dominant_kernel
    for n in windows:
        eng.run(n, seed=13, resume=resume)
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().clone() for k, v in eng.unconstrained.items()}
    loss = np.array(eng.losses())
    eng.close()
    return out, loss


def _same(monkeypatch, family, data, windows=(5,), resume=False, kw=None, mode="pair", kernel="k_guide_wave2", blocks=None):
    a, la = _fit(monkeypatch, True, family, data, windows, resume, kw or {}, mode, kernel, blocks)
    b, lb = _fit(monkeypatch, False, family, data, windows, resume, kw or {}, mode, kernel, blocks)
    assert len(la) == sum(windows) == len(lb) and np.all(np.isfinite(la))
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())
    assert np.array_equal(la, lb), np.max(np.abs(la - lb))
    return a


@pytest.fixture(scope="module")
def screens():
    return {acc: make_sorting_variant_screen(192, 2, bins=FIVE_BINS, guides_per_target=3, seed=501 + acc,
                                             with_accessibility=bool(acc), mask_fraction=0.05) for acc in (0, 1)}


@pytest.mark.parametrize("acc", [0, 1])
def test_pair_path(monkeypatch, screens, acc):
    out = _same(monkeypatch, "MixtureNormal", screens[acc], kw=dict(scale_by_accessibility=True) if acc else {})
    # the screen reaches the tabulated branch: most guides have both concentrations above 6
    al = out["alpha_pi"].double().exp()
    cq = al / al.sum(-1, keepdim=True) * screens[acc].pi_a0.reshape(-1, 1).double()
    assert (cq > 6.0).all(-1).float().mean() > 0.5


@pytest.mark.parametrize("acc", [0, 1])
def test_async_on_eight_item_waves(monkeypatch, screens, acc):
    _same(monkeypatch, "MixtureNormal", screens[acc], kw=dict(scale_by_accessibility=True) if acc else {}, mode="async",
          kernel="k_svi_async", blocks=8)


@pytest.mark.parametrize("mode,kernel,blocks", [("pair", "k_guide_wave2", None), ("async", "k_svi_async", 8)])
def test_resumed_window(monkeypatch, screens, mode, kernel, blocks):
    _same(monkeypatch, "MixtureNormal", screens[0], windows=(3, 2), resume=True, mode=mode, kernel=kernel, blocks=blocks)


def test_survival_wave_kernel(monkeypatch):
    data = make_survival_variant_screen(192, 2, guides_per_target=3, seed=503, mask_fraction=0.05)
    _same(monkeypatch, "MixtureNormal", data, mode=None, kernel="k_guide_survival_wave")
