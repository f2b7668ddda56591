"""How many updates a call makes: the host code cuts the n steps of a call into eager launches and replays of a ladder
of graphs (top_rung / build_ladder / replay_pairs, the resume ladder's head of `n mod 4 else 4` pairs; csrc/bean_hip.hip).
A miscut ladder leaves finite, plausible parameters that are a step or a few off.  Here n walks through every carry of
the ladders - 1 ... 20 and both sides of 32, 64 and 128 - at graph chunks that give ladders of one to eight rungs,
through bean_hip_svi_run, bean_hip_svi_resume (one window and two) and bean_hip_svi_run_ensemble; every fit must be,
bit for bit, the eager fit (graph_chunk = 0) of the same n, which tests/test_gpu_adam.py and
tests/test_gpu_parity.py pin to the stepwise loop: parameters, both moments, the n losses - and the loss slot behind
them untouched.  -m gpu."""
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = list(range(1, 21)) + [31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
CHUNKS = [1, 2, 3, 4, 6, 8, 50, 64, 128]
SEEDS = (9, 2_000_000_011)
SENTINEL = -7.0


class _Fits:
    """One screen, its initial state, and the eager fits every other fit is compared with (computed once per n)."""

    def __init__(self):
        self.data = make_sorting_variant_screen(300, 2, seed=91, mask_fraction=0.05).to(DEV)
        self.eager = {seed: self.engine() for seed in SEEDS}
        e = self.eager[SEEDS[0]]
        self.init = {k: v.detach().clone() for k, v in e.unconstrained.items()}
        self._ref = {}

    def engine(self, **kw):
        from bean_amd import engine

        eng = engine.HipSVI("MixtureNormal", self.data, num_steps=2000, **kw)
        assert eng.dominant_kernel == "k_guide_wave2"   # the {k_param, guide} pairs the ladders are made of
        return eng

    def reset(self, eng):
        """Initial parameters, zero moments, the loss history at the sentinel - through torch: a new fit."""
        for k, v in eng.unconstrained.items():
            v.copy_(self.init[k].expand_as(v))
            eng._m[k].zero_()
            eng._v[k].zero_()
        eng.loss_hist.fill_(SENTINEL)
        # the write is seen by the engine (version counters), which would send the next run(resume=True) through
        # bean_hip_svi_run: but this is the first window of a NEW fit - first_step 0 is never the step the previous
        # fit's last window prepared (its n >= 1), so bean_hip_svi_resume takes its full head by itself
        eng._resume_versions = None
        eng._resume_broken = False

    @staticmethod
    def state(eng, n, member=None):
        pick = (lambda t: t) if member is None else (lambda t: t[member])
        flat = torch.cat([pick(v).detach().reshape(-1) for d in (eng.unconstrained, eng._m, eng._v) for v in d.values()])
        return flat.clone(), pick(eng.loss_hist)[: n + 1].clone()

    def ref(self, n, seed=SEEDS[0]):
        if (n, seed) not in self._ref:
            eng = self.eager[seed]
            self.reset(eng)
            eng.run(n, seed=seed, graph_chunk=0, first_step=0)
            torch.cuda.synchronize()
            flat, loss = self.state(eng, n)
            assert torch.isfinite(flat).all() and torch.isfinite(loss[:n]).all() and loss[n].item() == SENTINEL
            self._ref[(n, seed)] = (flat, loss)
        return self._ref[(n, seed)]

    def same(self, eng, n, what, member=None, seed=SEEDS[0]):
        torch.cuda.synchronize()
        flat, loss = self.state(eng, n, member)
        ref_flat, ref_loss = self.ref(n, seed)
        # (int32 views: bitwise, and a NaN would not compare equal to itself)
        assert torch.equal(flat.view(torch.int32), ref_flat.view(torch.int32)), (
            what, "parameters / moments", int((flat != ref_flat).sum()))
        assert torch.equal(loss[:n], ref_loss[:n]), (what, "losses", (loss[:n] - ref_loss[:n]).abs().max().item())
        assert loss[n].item() == SENTINEL, (what, "the loss slot behind the call was written", loss[n].item())


@pytest.fixture(scope="module")
def fits():
    f = _Fits()
    yield f
    for e in f.eager.values():
        e.close()


def test_eager_fits_of_consecutive_counts_differ(fits):
    """The yardstick itself: one step more is another state (so an off-by-one cannot hide), and a repeated eager fit
    gives the same bits."""
    for n in (1, 2, 3, 4, 127, 128):
        assert not torch.equal(fits.ref(n)[0], fits.ref(n + 1)[0]), n
    again = fits.eager[SEEDS[0]]
    fits.reset(again)
    again.run(5, seed=SEEDS[0], graph_chunk=0, first_step=0)
    fits.same(again, 5, "eager, again")


@pytest.mark.parametrize("chunk", CHUNKS)
def test_run_step_counts(fits, chunk):
    eng = fits.engine()
    for n in COUNTS:
        fits.reset(eng)
        eng.run(n, seed=SEEDS[0], graph_chunk=chunk, first_step=0)
        fits.same(eng, n, ("run", chunk, n))
    eng.close()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_resume_step_counts(fits, chunk):
    eng = fits.engine()
    for n in COUNTS:
        fits.reset(eng)
        eng.run(n, seed=SEEDS[0], graph_chunk=chunk, first_step=0, resume=True)
        fits.same(eng, n, ("resume, one window", chunk, n))
        if n >= 3:
            fits.reset(eng)
            eng.run(n // 3, seed=SEEDS[0], graph_chunk=chunk, first_step=0, resume=True)
            eng.run(n - n // 3, seed=SEEDS[0], graph_chunk=chunk, resume=True)   # continues: a resumed window
            assert eng.steps_done == n
            fits.same(eng, n, ("resume, two windows", chunk, n))
    eng.close()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_ensemble_step_counts(fits, chunk):
    eng = fits.engine(n_members=2)
    for n in COUNTS:
        fits.reset(eng)
        eng.run_ensemble(n, SEEDS, graph_chunk=chunk, first_step=0)
        for k, seed in enumerate(SEEDS):
            fits.same(eng, n, ("run_ensemble, member", k, chunk, n), member=k, seed=seed)
    eng.close()


def test_the_top_rung_repeats(fits):
    """n = 300 at chunk 8: 37 replays of the largest graph behind the smaller rungs."""
    n = 300
    for what, fit, kw in (
        ("run", lambda e: e.run(n, seed=SEEDS[0], graph_chunk=8, first_step=0), {}),
        ("resume", lambda e: e.run(n, seed=SEEDS[0], graph_chunk=8, first_step=0, resume=True), {}),
        ("run_ensemble", lambda e: e.run_ensemble(n, SEEDS, graph_chunk=8, first_step=0), dict(n_members=2)),
    ):
        eng = fits.engine(**kw)
        fits.reset(eng)
        fit(eng)
        if kw:
            for k, seed in enumerate(SEEDS):
                fits.same(eng, n, (what, "member", k), member=k, seed=seed)
        else:
            fits.same(eng, n, what)
        eng.close()
