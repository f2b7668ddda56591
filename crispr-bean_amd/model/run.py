"""``run_inference`` and model selection for the HIP engine.

Mirrors the public surface of ``bean/model/run.py``: ``run_inference`` (347-396),
``identify_model_guide`` (399-457) and ``identify_negctrl_model_guide``
(460-474), with the same argument meaning, return structure and error behaviour.
The per-step loop the reference runs through ``pyro.infer.SVI`` is executed by
``libbean_hip`` (``bean_hip_svi_run``).
"""
from __future__ import annotations

import logging
import pickle as pkl
import sys
from functools import partial
from typing import Dict

import torch

from ..engine import HipSVI
from . import model as sorting_model
from .jackknife import (bootstrap_plan, design_plan, guide_plan, particle_seeds, power_plan, replicate_plan,  # noqa: F401
                        sample_plan, seed_plan, stack_counts, stack_masks)
from .model import ModelSpec

logger = logging.getLogger(__name__)
info, error = logger.info, logger.error

SEED = 101  # pyro.set_rng_seed(101) at import of bean/model/run.py:36


class ParamStore:
    """Minimal stand-in for ``pyro.get_param_store()`` as the reference consumes
    it (``bean/model/readwrite.py:66-98``, ``bean/cli/run.py:258-267``):
    ``store[name]`` is the *constrained* tensor; ``keys()``; ``in``; ``items()``."""

    def __init__(self, constrained: Dict[str, torch.Tensor]):
        self._c = constrained

    def __getitem__(self, name):
        return self._c[name]

    def __contains__(self, name):
        return name in self._c

    def keys(self):
        return self._c.keys()

    def items(self):
        return self._c.items()

    def __iter__(self):
        return iter(self._c)

    def __len__(self):
        return len(self._c)


def _resolve(obj) -> ModelSpec:
    if isinstance(obj, ModelSpec):
        return obj
    spec = obj()
    if not isinstance(spec, ModelSpec):
        raise TypeError(f"{obj!r} is not a crispr-bean_amd model/guide descriptor")
    return spec


def build_engine(model, guide, data, initial_lr=0.01, gamma=0.1, num_steps=2000, **engine_kw) -> HipSVI:
    m, g = _resolve(model), _resolve(guide)
    if m.family != g.family and not (m.family == "MixtureNormalConstPi"):
        raise ValueError(f"model family {m.family} does not match guide family {g.family}")
    if m.selection != getattr(data, "selection", "sorting"):
        raise ValueError(f"{m.selection} model used with a {getattr(data, 'selection', 'sorting')} screen")
    if m.selection == "survival":
        neg = m.get("mu_negctrl", (0.0, 0.1))
        if m.family in ("MixtureNormal", "MultiMixtureNormal"):
            engine_kw = dict(engine_kw, mu_negctrl=(float(neg[0]), float(neg[1])))
    return HipSVI(
        m.family,
        data,
        use_bcmatch=bool(m.get("use_bcmatch", True)),
        scale_by_accessibility=bool(m.get("scale_by_accessibility", False)),
        fit_noise=bool(g.get("fit_noise", False)),
        sd_scale=float(m.get("sd_scale", 0.01)),
        prior_params=m.get("prior_params"),
        mask_thres=int(m.get("mask_thres", 10)),
        # the guide runs first, so its `alpha_prior` is the one pyro.param("alpha_pi", ...) is created with
        alpha_prior=float(g.get("alpha_prior", m.get("alpha_prior", 1)) or 1),
        initial_lr=initial_lr,
        gamma=gamma,
        num_steps=num_steps,
        **engine_kw,
    )


def run_inference(model, guide, data, initial_lr=0.01, gamma=0.1, num_steps=2000, autoguide=False,
                  seed: int = SEED, report_every: int = 100, verbose: bool = True, num_particles: int = 1):
    """Run SVI for the given model and guide (``bean/model/run.py:347-396``).

    Returns ``(param_store, {"loss": [float] * num_steps, "params": {name: cpu
    tensor}})`` where ``param_store[name]`` and ``params[name]`` are the
    constrained values, exactly the structure the reference returns.
    A non-finite loss halts the fit at the end of its report window (100 steps) and raises
    ``ValueError`` after dumping the parameters to ``tmp_result.pkl``, as the reference does on a
    ``ValueError`` inside the loop (there at the failing step itself; here the dump holds the parameters
    as they were at the start of the failing window, i.e. at most 99 steps earlier and finite).

    When ``torch.distributed`` is initialised with more than one rank the guides
    are sharded on target boundaries (``parallel.run_sharded``): every rank fits
    its shard on its own GPU and all ranks return the whole-screen result.

    ``num_particles=P`` > 1 (Pyro's ``Trace_ELBO(num_particles=P)``, which the reference never passes): every step
    draws every latent site P times, particle p with ``particle_seeds(seed, P)[p]``, and applies one update with the
    mean of the P gradients (``HipSVI.run_particles``); ``loss`` holds the particles' mean loss.  One fit, the same
    return structure, the same halt.  Not combined with guide sharding over several ranks.
    """
    import torch.distributed as dist

    from .. import parallel
    from .._lib import MAX_MEMBERS

    num_particles = int(num_particles)
    if not 1 <= num_particles <= MAX_MEMBERS:
        raise ValueError(f"num_particles must be in [1, {MAX_MEMBERS}], got {num_particles}")
    if num_particles > 1:
        _single_rank_only("run_inference(num_particles > 1)")
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    device = torch.device("cuda", torch.cuda.current_device())
    spec = _resolve(model)
    # ControlNormal has screen-wide scalar parameters and only sees the (small)
    # negative-control subset: every rank fits it redundantly instead of sharding (the engine can
    # shard it - bean_hip_sharded_* - but a per-step collective costs more than the fit).
    redundant = spec.family == "ControlNormal"
    sharded = world > 1 and not redundant
    engines = []

    def factory(shard_data, shard, n_total, **extra):
        if spec.family == "MultiMixtureNormal":
            # tiling: this engine's guides ordered by their number of alleles (parallel.order_by_alleles); draws
            # and returned parameters are those of the screen order
            shard_data, ids = parallel.order_by_alleles(shard_data, shard[0])
            if ids is not None:
                extra = dict(extra, guide_ids=ids)
        eng = build_engine(
            model, guide, shard_data.to(device), initial_lr=initial_lr, gamma=gamma, num_steps=num_steps,
            device=device, guide_offset=shard[0], target_offset=shard[2], n_guides_total=n_total, **extra,
        )
        engines.append(eng)
        return eng

    def report(step, loss):
        if verbose:
            print(f"loss {loss} @ iter {step}")

    rank = dist.get_rank() if world > 1 else 0
    try:
        if sharded:
            constrained, losses = parallel.run_sharded(
                factory, data, num_steps, seed=seed, report_every=report_every, on_report=report)
        else:
            whole = (0, data.n_guides, 0, getattr(data, "n_targets", 0))
            particles = dict(n_particles=num_particles) if num_particles > 1 else {}
            eng = factory(data, whole, data.n_guides, **particles)  # configuration errors surface as they are
            done = 0
            while done < num_steps:
                k = min(report_every, num_steps - done)
                eng.window_start = eng.snapshot()  # what a halt inside this window dumps
                if num_particles > 1:
                    eng.run_particles(k, seed)
                else:
                    eng.run(k, seed=seed, resume=True)
                # the reference halts at the failing step (run.py:375-390); here at the end of its report window
                window = eng.loss_hist[done:done + k]
                parallel.check_window_finite(window, done)
                report(done, float(window[0]))
                done += k
            losses = eng.losses()
            constrained = eng.constrained()
        if not all(l == l and abs(l) != float("inf") for l in losses):
            bad = next(i for i, l in enumerate(losses) if not (l == l and abs(l) != float("inf")))
            raise FloatingPointError(f"non-finite loss at iteration {bad}")
    except FloatingPointError as exc:
        # the reference dumps the parameter store when the fit itself fails (run.py:381-390); every
        # rank holds its own shard's parameters, so the file name carries the rank when there are several
        name = "tmp_result.pkl" if world == 1 else f"tmp_result.rank{rank}.pkl"
        error(f"Error occurred during fitting. Saving temporary output at {name}.")
        with open(name, "wb") as handle:
            # the parameters as they were at the START of the failing report window: the device loop has
            # applied up to report_every - 1 further (NaN) updates since the failing step, the reference
            # stops at the failing step itself (run.py:375-390)
            dump = {}
            if engines:
                eng = engines[-1]
                dump = {k: v.cpu() for k, v in eng.constrained(getattr(eng, "window_start", None)).items()}
            pkl.dump({"param": dump}, handle)
        raise ValueError(
            f"Fitting halted for command: {' '.join(sys.argv)} with following error: \n {exc}"
        )
    finally:
        for e in engines:
            e.close()
    store = ParamStore(constrained)
    out = {"loss": losses, "params": {k: v.detach().cpu() for k, v in constrained.items()}}
    return store, out


def _fit_members(model, guide, data, plan, run, common, report_every, verbose, batch_survival=False):
    """One engine run of ``_fit_plan``: the members ``run`` of ``plan`` (member i of the engine is member ``run[i]`` of
    the plan).  Returns their ``(param_store, {"loss", "params"})`` pairs, or ``None`` where the batched kernels do not
    take the shape - a survival screen without ``batch_survival`` among them; halts as ``_fit_plan`` says."""
    from .. import parallel
    from .._lib import MAX_MEMBERS
    from ..engine import EnsembleUnsupported

    n = len(run)
    seeds = [plan.seeds[k] for k in run]
    spec = _resolve(model)
    if spec.family in ("MultiMixtureNormal", "ControlNormal") or n > MAX_MEMBERS:
        return None
    if spec.selection == "survival" and not batch_survival:
        return None
    extra = {}
    if plan.differ_in:
        screens = [plan.screen(k) for k in run]
        extra["member_masks"] = stack_masks(screens)
        if "counts" in plan.differ_in:
            x, x_bc = stack_counts(screens)
            # (the barcode-matched counts travel only where the fit uses them: build_engine's reading of the model)
            extra["member_counts"] = (x, x_bc if bool(spec.get("use_bcmatch", True)) else None)
    device = torch.device("cuda", torch.cuda.current_device())
    try:
        eng = build_engine(model, guide, data.to(device), device=device, n_guides_total=data.n_guides,
                           n_members=n, **extra, **common)
    except EnsembleUnsupported:
        return None
    num_steps = common["num_steps"]
    try:
        done = 0
        while done < num_steps:
            k = min(report_every, num_steps - done)
            window_start = eng.snapshot()  # what a halt inside this window dumps
            eng.run_ensemble(k, seeds)
            windows = eng.loss_hist[:, done:done + k]
            for member in range(n):
                try:
                    parallel.check_window_finite(windows[member], done)
                except FloatingPointError as exc:
                    what = plan.labels[run[member]]
                    name = f"tmp_result.{plan.tags[run[member]]}.pkl"
                    error(f"Error occurred during fitting ({what}, seed {seeds[member]}). "
                          f"Saving temporary output at {name}.")
                    with open(name, "wb") as handle:
                        dump = {p: v.cpu() for p, v in eng.constrained(window_start, member=member).items()}
                        pkl.dump({"param": dump, **plan.dump_extra[run[member]]}, handle)
                    raise ValueError(f"Fitting halted for command: {' '.join(sys.argv)} with following error: \n "
                                     f"{what} (seed {seeds[member]}): {exc}")
            if verbose:
                print(f"loss {' '.join(str(float(v)) for v in windows[:, 0])} @ iter {done}")
            done += k
        losses = eng.losses()
        results = []
        for member in range(n):
            constrained = {p: v.clone() for p, v in eng.constrained(member=member).items()}
            results.append((ParamStore(constrained),
                            {"loss": losses[member].tolist(), "params": {p: v.detach().cpu() for p, v in constrained.items()}}))
    finally:
        eng.close()
    return results


def _fit_plan(model, guide, data, plan, common, report_every, verbose, skip_first=False, batch_survival=False):
    """The K fits of a ``MemberPlan`` (``model/jackknife.py``): the list of what ``run_inference`` returns for
    ``plan.screen(k)`` with ``plan.seeds[k]`` - bit for bit.  This is the fit behind ``run_inference_ensemble`` and the
    three jackknives.

    Where the batched kernels take the shape (the sorting variant families: ``bean_hip_ensemble_supported``) the fits
    are members of one engine - with their own masks and counts where the plan's screens differ in them
    (``HipSVI(member_masks=..., member_counts=...)``, member 0 = the screen itself) - stepped by the same launches, in
    report windows.  With ``plan.per_run`` an engine run holds member 0 and at most that many further members; member
    0's result is the first run's.  The survival variant Normal / MixtureNormal families have member kernels of their
    own (``bean_hip_survival_members_supported``) and go the same way where the caller opts in with
    ``batch_survival=True`` (``run_survival_bootstrap`` does; ``run_inference_ensemble`` and the three jackknives do
    not yet, and fit a survival screen's members one after the other).  Every other family (tiling, ControlNormal, sample
    covariates, screens large enough for the one-launch stepper) and more than ``MAX_MEMBERS`` members in one run are
    fitted one after the other through ``run_inference``.  A non-finite loss of ANY member halts the fit at the end of its report window with the
    ``ValueError`` of ``run_inference``: the message names ``plan.labels[k]`` and the seed, and the parameters as they
    were at the start of the window go to ``tmp_result.<plan.tags[k]>.pkl`` together with ``plan.dump_extra[k]``.  (One
    after the other a halt is ``run_inference``'s own: it dumps to ``tmp_result.pkl``, and with ``plan.label_halts`` the
    label is appended to its message.)

    ``skip_first``: the caller holds member 0's fit already and gets the fits of members 1 ... K - 1 alone.  An engine
    run still steps member 0 next to the others - member 0 of every engine is the screen itself - and its result is
    dropped; one after the other it is not fitted."""
    K = len(plan.seeds)
    results = {}
    for at in range(1, max(K, 2), plan.per_run or K):
        run = [0] + list(range(at, min(at + (plan.per_run or K), K)))
        # (the opt-in travels by name, and only where it is given: the call is otherwise the one it has always been)
        opt_in = {"batch_survival": True} if batch_survival else {}
        fitted = _fit_members(model, guide, data, plan, run, common, report_every, verbose, **opt_in)
        if fitted is None:
            break
        for k, fit in zip(run, fitted):
            results.setdefault(k, fit)  # (member 0: the first run's)
    else:
        return [results[k] for k in range(1 if skip_first else 0, K)]
    results = []  # one after the other
    for k, seed in enumerate(plan.seeds):
        if skip_first and k == 0:
            continue
        try:
            results.append(run_inference(model, guide, plan.screen(k), seed=seed, report_every=report_every,
                                         verbose=verbose, **common))
        except ValueError as exc:
            if not plan.label_halts or "Fitting halted" not in str(exc):
                raise
            raise ValueError(f"{exc} ({plan.labels[k]})") from exc
    return results


def _single_rank_only(who):
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError(f"{who} does not combine with guide sharding over several ranks")


def run_inference_ensemble(model, guide, data, seeds, initial_lr=0.01, gamma=0.1, num_steps=2000,
                           report_every: int = 100, verbose: bool = True):
    """``len(seeds)`` independent SVI fits of one screen, member k with the random streams of ``seeds[k]``.

    Returns a list of ``(param_store, {"loss", "params"})`` pairs, each exactly what
    ``run_inference(..., seed=seeds[k])`` returns - bit for bit: all members stepped by the same launches where the
    batched kernels take the shape, else seed after seed (``_fit_plan``).  A non-finite loss of ANY member halts the fit;
    message and dump file (``tmp_result.member<k>.pkl``) name the member.  Not combined with guide sharding over
    several ranks."""
    plan = seed_plan(data, seeds)
    _single_rank_only("run_inference_ensemble")
    return _fit_plan(model, guide, data, plan, dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps),
                     report_every, verbose)


def run_inference_jackknife(model, guide, data, seed: int = SEED, initial_lr=0.01, gamma=0.1, num_steps=2000,
                            report_every: int = 100, verbose: bool = True):
    """Replicate jackknife: the fit of the screen and one fit per replicate with that replicate masked
    (``model/jackknife.py``), all with the same ``seed`` - common random numbers, so the fits differ through the data
    and not through the stream.

    Returns ``(full, loo, left_out)``: ``full`` is exactly what ``run_inference(..., seed=seed)`` returns, ``loo[j]``
    exactly what it returns for ``leave_out(data, left_out[j])`` - bit for bit - and ``left_out`` lists the replicates
    that are not already fully masked (fewer than two: ``ValueError``).  The 1 + len(left_out) fits differ in their
    masks only: members of one engine where the batched kernels take the shape, else mask after mask (``_fit_plan``).
    A non-finite loss of any member halts the fit; message and dump file (``tmp_result.full.pkl`` /
    ``tmp_result.without_replicate<r>.pkl``, with ``"left_out": r``) name the left-out replicate.  Not combined with
    guide sharding over several ranks."""
    _single_rank_only("run_inference_jackknife")
    plan = replicate_plan(data, seed)
    results = _fit_plan(model, guide, data, plan, dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps),
                        report_every, verbose)
    return (results[0], results[1:], *plan.chosen)


def run_inference_guide_jackknife(model, guide, data, seed: int = SEED, initial_lr=0.01, gamma=0.1, num_steps=2000,
                                  report_every: int = 100, verbose: bool = True, max_positions: int = 63):
    """Guide jackknife: the fit of the screen and, for every position j a target's guides can have, one fit with the
    guide at position j of EVERY target masked (``model/jackknife.py``), all with the same ``seed`` - common random
    numbers.

    Returns ``(full, loo, positions, included)``: ``full`` is exactly what ``run_inference(..., seed=seed)`` returns,
    ``loo[i]`` exactly what it returns for ``leave_out_guides(data, <the guides at positions[i]>)`` - bit for bit -
    and ``positions`` / ``included`` are those of ``guide_positions(data, max_positions)`` (no included pair:
    ``ValueError``; targets with more than ``max_positions`` guides take no part, their number is logged).

    In the sorting variant families the batched kernels take (``Normal`` without sample covariates, ``MixtureNormal``
    in all its options) the targets share no parameter and the streams are keyed by global index: target t's slice of
    ``loo[i]`` is, bit for bit, its slice of the fit with only guide (t, positions[i]) masked, and a target without a
    guide at that position keeps the full fit's bits.  There the 1 + len(positions) fits are members of one engine
    that differ in ``repguide_mask`` only (``_fit_plan``).  Everywhere else the masks are fitted one after the other,
    with the same return value - but survival variant screens couple their targets through ``q0`` and sorting
    ``Normal`` with sample covariates through ``mu_cov``: a member is then "position j left out everywhere", NOT a set
    of single-guide fits.  Tiling families are refused (an edit's guides are not a target's guides), as are several
    ranks.  A non-finite loss of any member halts the fit; message and dump file (``tmp_result.full.pkl`` /
    ``tmp_result.without_guide_position<j>.pkl``, with ``"left_out_position": j``) name the position."""
    spec = _resolve(model)
    if spec.family == "MultiMixtureNormal" or getattr(data, "library_design", "variant") == "tiling":
        raise ValueError("a guide jackknife needs targets that own their guides: not defined for tiling screens "
                         "(an edit's guides are not a target's guides)")
    _single_rank_only("run_inference_guide_jackknife")
    plan = guide_plan(data, seed, max_positions)
    n_long = int((data.target_lengths.detach().cpu() > int(max_positions)).sum())
    if n_long:
        info(f"Guide jackknife: {n_long} target(s) with more than {int(max_positions)} guides take no part.")
    results = _fit_plan(model, guide, data, plan, dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps),
                        report_every, verbose)
    return (results[0], results[1:], *plan.chosen)


def run_inference_sample_jackknife(model, guide, data, by: str = "sample", seed: int = SEED, initial_lr=0.01, gamma=0.1,
                                   num_steps=2000, report_every: int = 100, verbose: bool = True,
                                   max_groups_per_run: int = 63):
    """Sample jackknife: the fit of the screen and one fit per sample (``by="sample"``: one condition of one replicate)
    or per condition (``by="condition"``: that condition of every replicate) with it masked as the reference masks a
    sample - ``sample_mask`` and the counts zeroed (``model/jackknife.py::leave_out_samples``) - all with the same
    ``seed``: common random numbers.

    Returns ``(full, loo, groups, names)``: ``full`` is exactly what ``run_inference(..., seed=seed)`` returns,
    ``loo[j]`` exactly what it returns for ``leave_out_samples(data, groups[j])`` - bit for bit - and ``groups`` /
    ``names`` are those of ``sample_groups(data, by)`` (fewer than two groups: ``ValueError``).  The fits differ in
    ``sample_mask`` AND in their counts: members of one engine where the batched kernels take the shape - more than
    ``max_groups_per_run`` groups (at most 63: the full screen is member 0 of every run) in several such runs, ``full``
    coming from the first - else screen after screen (``_fit_plan``).  A non-finite loss of any member halts the fit;
    message and dump file (``tmp_result.full.pkl`` / ``tmp_result.without_<name>.pkl``, with ``"left_out": [[r, b],
    ...]``) name the group.  Not combined with guide sharding over several ranks."""
    _single_rank_only("run_inference_sample_jackknife")
    plan = sample_plan(data, by, seed, max_groups_per_run)
    results = _fit_plan(model, guide, data, plan, dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps),
                        report_every, verbose)
    return (results[0], results[1:], *plan.chosen)


def _predictive_refusal(spec, data, world: int = 1):
    """Why the count simulator does not take this model / screen, or None (``bean_hip_predictive_supported``)."""
    design = getattr(data, "library_design", "variant")
    if spec.family == "MultiMixtureNormal" or design == "tiling":
        return "tiling screens (MultiMixtureNormal)"
    if spec.selection == "survival" or getattr(data, "selection", "sorting") == "survival":
        return f"survival screens ({spec.family})"
    if spec.family == "ControlNormal":
        return "the negative-control model (ControlNormal)"
    if getattr(data, "sample_covariates", None) is not None:
        return f"screens with sample covariates ({spec.family})"
    if world > 1:
        return f"guide-sharded fits over {world} ranks ({spec.family})"
    return None


def load_parameters(eng: HipSVI, param_store) -> None:
    """Write the constrained values of ``param_store`` (what ``run_inference`` returns, or the ``params`` of a
    ``--save-raw`` pickle that ``--load-existing`` reads) into the engine's unconstrained parameter tensors.  The draw
    and tables a previous window left on the device belong to other values: the chain of resumed windows is broken."""
    from ..engine import POSITIVE

    for name, dst in eng.unconstrained.items():
        if name not in param_store:
            raise ValueError(f"the parameter store has no {name!r}: it is not a fit of this model")
        v = torch.as_tensor(param_store[name]).detach().to(dst.device, torch.float32)
        if v.numel() != dst.numel():
            raise ValueError(f"parameter {name!r} has {v.numel()} entries, this screen needs {dst.numel()}")
        dst.copy_((v.log() if name in POSITIVE else v).reshape(dst.shape))
    eng.invalidate_resume()


def run_posterior_predictive(model, guide, data, param_store, n_draws: int = 200, seed: int = SEED):
    """Posterior predictive check of a fit (``model/predictive.py``): an engine for ``data`` with the fitted parameters
    of ``param_store`` loaded, ``n_draws`` replicate screens drawn on the device from guide and likelihood, and the
    summary of their discrepancy statistics against the observed counts (a dict of device tensors).

    Raises ``PredictiveUnsupported`` - the message names the family - for tiling and survival screens,
    ``ControlNormal``, sample covariates and several ranks."""
    import torch.distributed as dist

    from ..engine import PredictiveUnsupported
    from .predictive import posterior_predictive

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _predictive_refusal(spec, data, world)
    if why is not None:
        raise PredictiveUnsupported(f"a posterior predictive check is not available for {why}: the count simulator "
                                    "serves the sorting variant Normal and MixtureNormal models on one GPU")
    device = torch.device("cuda", torch.cuda.current_device())
    eng = build_engine(model, guide, data.to(device), num_steps=1, device=device, n_guides_total=data.n_guides)
    try:
        load_parameters(eng, param_store)
        summary = posterior_predictive(eng, n_draws=n_draws, seed=seed)
        torch.cuda.synchronize(device)
    finally:
        eng.close()
    return summary


def _survival_predictive_refusal(spec, data, world: int = 1):
    """Why the survival count simulator does not take this model / screen, or None
    (``bean_hip_survival_predictive_supported``)."""
    design = getattr(data, "library_design", "variant")
    if spec.family == "MultiMixtureNormal" or design == "tiling":
        return "tiling screens (MultiMixtureNormal)"
    if not (spec.selection == "survival" or getattr(data, "selection", "sorting") == "survival"):
        return f"sorting screens ({spec.family})"
    if spec.family == "ControlNormal":
        return "the negative-control model (ControlNormal)"
    if getattr(data, "sample_covariates", None) is not None:
        return f"screens with sample covariates ({spec.family})"
    if world > 1:
        return f"guide-sharded fits over {world} ranks ({spec.family})"
    return None


def run_survival_predictive(model, guide, data, param_store, n_draws: int = 200, seed: int = SEED):
    """Posterior predictive check of a survival fit (``model/predictive.py::survival_predictive``): an engine for
    ``data`` built as ``run_posterior_predictive`` builds it - the same model / guide partials, so the ``mu_negctrl`` of
    the control fit is the fit's - with the fitted parameters of ``param_store`` loaded, ``n_draws`` replicate screens
    drawn on the device, and the summary against the observed counts (a dict of device tensors).

    Raises ``PredictiveUnsupported`` - the message names the family - for sorting screens, tiling, ``ControlNormal``
    and several ranks."""
    import torch.distributed as dist

    from ..engine import PredictiveUnsupported
    from .predictive import survival_predictive

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _survival_predictive_refusal(spec, data, world)
    if why is not None:
        raise PredictiveUnsupported(f"a survival predictive check is not available for {why}: the survival count "
                                    "simulator serves the survival variant Normal and MixtureNormal models on one GPU")
    device = torch.device("cuda", torch.cuda.current_device())
    eng = build_engine(model, guide, data.to(device), num_steps=1, device=device, n_guides_total=data.n_guides)
    try:
        load_parameters(eng, param_store)
        summary = survival_predictive(eng, n_draws=n_draws, seed=seed)
        torch.cuda.synchronize(device)
    finally:
        eng.close()
    return summary


def run_importance_check(model, guide, data, param_store, n_draws: int = 1000, seed: int = SEED, integrate_pi=None,
                         tail_rule: bool = False):
    """Importance-sampling check of a fit's mean-field posterior (``model/importance.py``): an engine for ``data`` with
    the fitted parameters of ``param_store`` loaded, ``n_draws`` draws from the guide weighted per target by
    ``p(x, z) / q(z)`` on the device, and their summary - per target ``psis_k``, ``is_ess``, ``mu_is``, ``mu_sd_is``,
    ``n_is`` (a dict of device tensors).  No refit.  ``integrate_pi=Q`` (16, 32 or 64 nodes) merges in the summary of the
    weights of ``(mu_t, sd_t)`` alone, ``pi`` integrated out of the model: ``psis_k_marg``, ``mu_is_marg``,
    ``mu_sd_is_marg``, ``is_ess_marg`` (NaN where ``n_pairs_unresolved > 0``) and ``n_pairs_unresolved``.  ``tail_rule``:
    the Gauss-Jacobi rule for the unresolved pairs in those weights (``importance_check(tail_rule=True)``), which adds
    ``n_pairs_tail`` and ``is_tail_err`` and fills the four values where ``is_tail_err <= 1e-3 n_pairs_tail``.

    Raises ``PredictiveUnsupported`` - the message names the family - for tiling and survival screens,
    ``ControlNormal``, sample covariates and several ranks."""
    import torch.distributed as dist

    from ..engine import PredictiveUnsupported
    from .importance import importance_check

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _predictive_refusal(spec, data, world)
    if why is not None:
        raise PredictiveUnsupported(f"an importance-sampling check is not available for {why}: the per-target weights "
                                    "serve the sorting variant Normal and MixtureNormal models on one GPU")
    device = torch.device("cuda", torch.cuda.current_device())
    eng = build_engine(model, guide, data.to(device), num_steps=1, device=device, n_guides_total=data.n_guides)
    try:
        load_parameters(eng, param_store)
        summary = importance_check(eng, n_draws=n_draws, seed=seed, integrate_pi=integrate_pi,
                                   **({"tail_rule": True} if tail_rule else {}))
        torch.cuda.synchronize(device)
    finally:
        eng.close()
    return summary


def run_grid_posterior(model, guide, data, param_store, nodes: int = 32, tail_rule: bool = False):
    """Grid posterior of ``(mu, sd)`` per target (``model/grid_posterior.py``): an engine for ``data`` with the fitted
    parameters of ``param_store`` loaded - they place the first zoom box and nothing else - and the summary of the log
    joint on every target's own grid, ``pi`` integrated out by ``nodes``-point quadrature: ``mu_grid``, ``mu_sd_grid``,
    ``sd_grid``, ``p_mu_pos_grid``, ``log_evidence_grid``, ``log_bf10_grid`` (NaN where ``grid_ok`` is false),
    ``grid_ok``, ``n_pairs_unresolved`` and the diagnostics (a dict of device tensors).  No refit.  ``tail_rule``: the
    Gauss-Jacobi rule for the unresolved pairs in every pass (``grid_posterior(tail_rule=True)``), which adds
    ``n_pairs_tail`` and ``grid_tail_err``.

    Raises ``PredictiveUnsupported`` - the message names the reason - for tiling and survival screens,
    ``ControlNormal``, sample covariates, several ranks and accessibility scaling."""
    import torch.distributed as dist

    from ..engine import PredictiveUnsupported
    from .grid_posterior import grid_posterior

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _predictive_refusal(spec, data, world)
    if why is None and spec.get("scale_by_accessibility", False):
        why = f"fits with accessibility scaling ({spec.family}): the guide noise is a further latent per guide"
    if why is not None:
        raise PredictiveUnsupported(f"a grid posterior is not available for {why}: the posterior of a target is a "
                                    "function of (mu, sd) alone in the sorting variant Normal and MixtureNormal models "
                                    "without accessibility, on one GPU")
    device = torch.device("cuda", torch.cuda.current_device())
    eng = build_engine(model, guide, data.to(device), num_steps=1, device=device, n_guides_total=data.n_guides)
    try:
        load_parameters(eng, param_store)
        summary = grid_posterior(eng, nodes=int(nodes), **({"tail_rule": True} if tail_rule else {}))
        torch.cuda.synchronize(device)
    finally:
        eng.close()
    return summary


def bootstrap_engine(model, guide, data, param_store) -> HipSVI:
    """The engine a parametric bootstrap draws its screens from: built for ``data`` as ``run_posterior_predictive``
    builds its own, the fitted parameters of ``param_store`` loaded, and zero standard-normal draws injected into every
    per-target and per-guide Normal site the family has (``mu``, ``sd`` and, with accessibility scaling, the guide noise
    site) - the plug-in: the global latents sit at their guide's locations, only the per-(replicate, guide) ``pi`` draws
    and the counts are fresh per screen.  The caller closes it."""
    device = torch.device("cuda", torch.cuda.current_device())
    eng = build_engine(model, guide, data.to(device), num_steps=1, device=device, n_guides_total=data.n_guides)
    try:
        load_parameters(eng, param_store)
        zeros = lambda n: torch.zeros(int(n), dtype=torch.float64, device=device)  # noqa: E731
        noise = {"eps_mu": zeros(eng.T), "eps_sd": zeros(eng.T)}
        if eng.scale_by_accessibility:
            noise["eps_noise"] = zeros(data.n_guides)
        eng.set_noise(noise)
    except BaseException:
        eng.close()
        raise
    return eng


def bootstrap_screens(eng: HipSVI, n_boot: int, boot_seed: int = SEED):
    """``(X (n_boot, R, B, G), X_bcmatch or None)``, device tensors: screen j is draw j of
    ``eng.simulate_members(..., seed=boot_seed)`` whatever the batching - calls of at most ``MAX_MEMBERS`` screens, each
    starting at the number of screens already drawn."""
    from .._lib import MAX_MEMBERS

    xs, xbcs = [], []
    done = 0
    while done < n_boot:
        k = min(MAX_MEMBERS, n_boot - done)
        sim = eng.simulate_members(done, k, seed=boot_seed)
        xs.append(sim["X"])
        if "X_bcmatch" in sim:
            xbcs.append(sim["X_bcmatch"])
        done += k
    return torch.cat(xs), (torch.cat(xbcs) if xbcs else None)


def run_inference_bootstrap(model, guide, data, n_boot: int = 32, seed: int = SEED, boot_seed: int = SEED, initial_lr=0.01,
                            gamma=0.1, num_steps=2000, report_every: int = 100, verbose: bool = True,
                            max_per_run: int = 63):
    """Parametric bootstrap: fit the screen, draw ``n_boot`` screens from the fitted model on the device, and refit
    every one of them with the same ``seed`` (``model/jackknife.py::bootstrap_plan``) - how far would ``mu`` move if the
    experiment were repeated under the model just fitted.

    The screens come from the plug-in (``bootstrap_engine``): ``mu``, ``sd`` and the guide noise at their fitted
    locations; per (replicate, guide) a fresh ``pi ~ q(pi)``, ``p ~ Dirichlet(alpha)`` and ``x ~ Multinomial(n_obs, p)``
    with the streams of ``boot_seed``, screen j being draw j.  Masks, size factors, ``a0``, ``pi_a0``, the control allele
    counts and every (replicate, guide) total are the observed screen's: the bootstrap conditions on them.

    Returns ``(full, boots)``: ``full`` is exactly what ``run_inference(..., seed=seed)`` returns, ``boots[j]`` exactly
    what it returns for the screen with the counts of draw j - bit for bit.  The refits are members of one engine next
    to the screen, at most ``max_per_run`` (1 ... 63) per engine run, where the batched kernels take the shape; else one
    after the other (``_fit_plan``).  Raises ``PredictiveUnsupported`` - the message names the family - for tiling and
    survival screens, ``ControlNormal``, sample covariates and several ranks; ``n_boot < 2`` is a ``ValueError``.  A
    non-finite loss of any member halts the fit; message and dump file (``tmp_result.full.pkl`` /
    ``tmp_result.bootstrap<j>.pkl``, with ``"bootstrap": j``) name the screen."""
    import dataclasses

    import torch.distributed as dist

    from ..engine import PredictiveUnsupported
    from .jackknife import MAX_GUIDE_POSITIONS

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _predictive_refusal(spec, data, world)
    if why is not None:
        raise PredictiveUnsupported(f"a parametric bootstrap is not available for {why}: the count simulator serves the "
                                    "sorting variant Normal and MixtureNormal models on one GPU")
    n_boot, per_run = int(n_boot), int(max_per_run)
    if n_boot < 2:
        raise ValueError(f"a parametric bootstrap needs at least 2 screens, got {n_boot}")
    if not 1 <= per_run <= MAX_GUIDE_POSITIONS:
        raise ValueError(f"max_per_run must be in [1, {MAX_GUIDE_POSITIONS}] (the screen is member 0 of every run), "
                         f"got {per_run}")
    common = dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps)
    first = run_inference(model, guide, data, seed=seed, report_every=report_every, verbose=verbose, **common)
    eng = bootstrap_engine(model, guide, data, first[0])
    try:
        x, x_bc = bootstrap_screens(eng, n_boot, boot_seed)
        torch.cuda.synchronize(eng.device)
    finally:
        eng.close()
    home = lambda t, like: None if t is None else t.to(like.device, like.dtype)  # noqa: E731
    plan = bootstrap_plan(data, seed, home(x, data.X_masked),
                          home(x_bc, data.X_bcmatch_masked) if x_bc is not None else None)
    plan = dataclasses.replace(plan, per_run=per_run)
    results = _fit_plan(model, guide, data, plan, common, report_every, verbose)
    return results[0], results[1:]


def survival_bootstrap_engine(model, guide, data, param_store) -> HipSVI:
    """The engine a survival screen's parametric bootstrap draws its screens from: built for ``data`` as
    ``run_survival_predictive`` builds its own - the same model / guide partials, so the ``mu_negctrl`` location and scale
    a control fit handed to the model are the fit's - the fitted parameters of ``param_store`` loaded, and the plug-in
    injected: zero standard-normal draws into ``eps_mu`` and, with accessibility scaling, ``eps_noise`` - every Normal
    site a survival family has (``sd`` is not a latent of the survival models: the library has no ``eps_sd`` slot for
    them and refuses to bind one); for the NormalModel ``q_0`` at the mean of its Dirichlet,
    ``initial_abundance / sum(initial_abundance)`` for every replicate.  ``eps_u`` is NOT injected: the baseline
    ``u_g ~ Normal(m0, s0)`` of the MixtureNormal model has no variational factor - the model draws it afresh every
    step - so every screen draws its own, as it draws its own ``pi``.  The caller closes the engine."""
    device = torch.device("cuda", torch.cuda.current_device())
    eng = build_engine(model, guide, data.to(device), num_steps=1, device=device, n_guides_total=data.n_guides)
    try:
        load_parameters(eng, param_store)
        zeros = lambda n: torch.zeros(int(n), dtype=torch.float64, device=eng.device)  # noqa: E731
        noise = {"eps_mu": zeros(eng.T)}
        if eng.scale_by_accessibility:
            noise["eps_noise"] = zeros(data.n_guides)
        if eng.surv_normal:
            ia = torch.as_tensor(param_store["initial_abundance"]).detach().to(eng.device, torch.float64).reshape(-1)
            noise["q_0"] = (ia / ia.sum()).expand(data.n_reps, data.n_guides).contiguous()
        eng.set_noise(noise)
    except BaseException:
        eng.close()
        raise
    return eng


def survival_bootstrap_screens(eng: HipSVI, n_boot: int, boot_seed: int = SEED):
    """``(X (n_boot, R, B, G), X_bcmatch or None)``, device tensors: screen j is draw j of
    ``eng.simulate_survival_members(..., seed=boot_seed)`` whatever the batching - calls of at most ``MAX_MEMBERS``
    screens, each starting at the number of screens already drawn (the batching of ``bootstrap_screens``)."""
    from .._lib import MAX_MEMBERS

    xs, xbcs = [], []
    done = 0
    while done < n_boot:
        k = min(MAX_MEMBERS, n_boot - done)
        sim = eng.simulate_survival_members(done, k, seed=boot_seed)
        xs.append(sim["X"])
        if "X_bcmatch" in sim:
            xbcs.append(sim["X_bcmatch"])
        done += k
    return torch.cat(xs), (torch.cat(xbcs) if xbcs else None)


def run_survival_bootstrap(model, guide, data, n_boot: int = 32, seed: int = SEED, boot_seed: int = SEED, initial_lr=0.01,
                           gamma=0.1, num_steps=2000, report_every: int = 100, verbose: bool = True, batch_refits: bool = True):
    """Parametric bootstrap of a survival screen: fit the screen, draw ``n_boot`` screens from the fitted model on the
    device in one launch per ``MAX_MEMBERS`` screens (``HipSVI.simulate_survival_members``), and refit every one of them
    with the same ``seed`` (``model/jackknife.py::bootstrap_plan``) - how far would ``mu`` move if the experiment were
    repeated under the model just fitted.

    The screens come from the plug-in (``survival_bootstrap_engine``): ``mu`` and the guide noise at their fitted
    locations, the NormalModel's ``q_0`` at the mean of its Dirichlet; per screen a fresh baseline
    ``u_g ~ Normal(m0, s0)`` (MixtureNormal: the site has no variational factor), per (replicate, guide) a fresh
    ``pi ~ q(pi)``, ``p ~ Dirichlet(alpha)`` over the timepoints and ``x ~ Multinomial(n_obs, p)`` with the streams of
    ``boot_seed``, screen j being draw j.

    Conditioned on - the observed screen's, shared by every refit: both masks; the size factors; ``a0`` /
    ``a0_bcmatch``; ``pi_a0`` and the control allele counts; every (replicate, guide) total over the timepoints;
    ``data.X``, which is left untouched - the observed initial abundance of the MixtureNormal engine reads it, and the
    drawn ``q_0`` does not enter the count concentrations, so the screens carry no information to redraw it from; and the
    ``mu_negctrl`` location and scale that a control fit handed to the model partial.

    Returns ``(full, boots)``: ``full`` is the first fit, exactly what ``run_inference(..., seed=seed)`` returns,
    ``boots[j]`` exactly what it returns for a ``copy.copy(data)`` with the counts of draw j - bit for bit.  The refits
    are members 1 ... of engines whose member 0 is the screen (``_fit_plan(skip_first=True, batch_survival=True)``, at
    most 63 screens per engine run): the survival member kernels step them in the same launches
    (``HipSVI.survival_members_supported``); member 0 is stepped next to them and dropped - ``full`` stays the
    ``run_inference`` fit.  Where the engine cannot be built (``EnsembleUnsupported``: ``BEAN_HIP_SURVIVAL=block``, more
    timepoints than the member launch takes) the refits go one after the other through ``run_inference``, the screen
    not among them; ``batch_refits=False`` asks for that path (same results; the members measured faster at every shape
    tried, up to 4.6 waves per SIMD in a single fit's guide launch: DESIGN.md section 29).  Raises ``PredictiveUnsupported`` - the message names the family - for sorting screens, tiling,
    ``ControlNormal``, sample covariates and several ranks; ``n_boot < 2`` is a ``ValueError``.  A non-finite loss of a
    batched refit halts as the sorting bootstrap's do: at the end of its report window, the parameters as they were at
    its start go to ``tmp_result.bootstrap<j>.pkl`` and the message names ``bootstrap screen j`` and the seed; one after
    the other it halts as ``run_inference`` halts (``tmp_result.pkl``, the message ends with ``(bootstrap screen
    j)``)."""
    import torch.distributed as dist

    from ..engine import PredictiveUnsupported

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _survival_predictive_refusal(spec, data, world)
    if why is not None:
        raise PredictiveUnsupported(f"a survival bootstrap is not available for {why}: the survival count simulator "
                                    "serves the survival variant Normal and MixtureNormal models on one GPU")
    n_boot = int(n_boot)
    if n_boot < 2:
        raise ValueError(f"a survival bootstrap needs at least 2 screens, got {n_boot}")
    common = dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps)
    full = run_inference(model, guide, data, seed=seed, report_every=report_every, verbose=verbose, **common)
    eng = survival_bootstrap_engine(model, guide, data, full[0])
    try:
        x, x_bc = survival_bootstrap_screens(eng, n_boot, boot_seed)
        torch.cuda.synchronize(eng.device)
    finally:
        eng.close()
    home = lambda t, like: None if t is None else t.to(like.device, like.dtype)  # noqa: E731
    plan = bootstrap_plan(data, seed, home(x, data.X_masked),
                          home(x_bc, data.X_bcmatch_masked) if x_bc is not None else None)
    # member 0 of the plan is the screen itself: `full` is that fit already
    return full, _fit_plan(model, guide, data, plan, common, report_every, verbose, skip_first=True,
                           batch_survival=bool(batch_refits))


def design_depths(depths):
    """The depth factors of a depth study as floats, depth 1 - the baseline of every ratio - put in front where it is
    absent.  An empty list, a factor that is not a finite number > 0 and a factor given twice are each a ``ValueError``."""
    import math

    out = [float(f) for f in depths]
    if not out:
        raise ValueError("a depth study needs at least one depth factor")
    for f in out:
        if not (math.isfinite(f) and f > 0):
            raise ValueError(f"a depth factor must be a finite number > 0, got {f:g}")
    twice = sorted({f for f in out if out.count(f) > 1})
    if twice:
        raise ValueError(f"depth factor {twice[0]:g} is given more than once")
    return out if 1.0 in out else [1.0] + out


def design_screens(eng: HipSVI, depths, n_screens: int, design_seed: int = SEED):
    """``(X (D, K, R, B, G), X_bcmatch or None)``, device tensors: screen (i, j) is depth ``depths[i]``, draw j of
    ``eng.simulate_design(..., seed=design_seed)`` whatever the batching - calls of at most ``MAX_MEMBERS`` screens,
    chunked over the depths (``D_c * K <= MAX_MEMBERS``) and, where ``K > MAX_MEMBERS``, over j with ``first_draw``
    advancing as ``bootstrap_screens`` advances it."""
    from .._lib import MAX_MEMBERS

    depths = [float(f) for f in depths]
    K = int(n_screens)
    rows_x, rows_bc = [], []
    for j0 in range(0, K, MAX_MEMBERS):
        k = min(MAX_MEMBERS, K - j0)
        per_call = max(MAX_MEMBERS // k, 1)
        xs, xbcs = [], []
        for i0 in range(0, len(depths), per_call):
            sim = eng.simulate_design(j0, k, depths[i0:i0 + per_call], seed=design_seed)
            xs.append(sim["X"])
            if "X_bcmatch" in sim:
                xbcs.append(sim["X_bcmatch"])
        rows_x.append(torch.cat(xs))
        if xbcs:
            rows_bc.append(torch.cat(xbcs))
    return torch.cat(rows_x, 1), (torch.cat(rows_bc, 1) if rows_bc else None)


def run_inference_design(model, guide, data, depths, n_screens: int = 8, seed: int = SEED, design_seed: int = SEED,
                         initial_lr=0.01, gamma=0.1, num_steps=2000, report_every: int = 100, verbose: bool = True,
                         max_per_run: int = 63):
    """Depth study: fit the screen, draw ``n_screens`` screens from the fitted model at each read depth of ``depths`` on
    the device, and refit every one of them with the same ``seed`` (``model/jackknife.py::design_plan``) - would
    sequencing deeper tighten ``mu``, or is its spread set by the dispersion ``a0`` and not by the read count.

    The screens are the parametric bootstrap's (``bootstrap_engine``: the plug-in, zero noise in every Normal site) with
    one change: at depth f every (replicate, guide) draws ``floor(f * n_obs + 0.5)`` reads.  Screen (i, j) uses the pi,
    Dirichlet and categorical streams of draw j of ``design_seed`` at every depth (common random numbers across depths).
    Masks, size factors, ``a0``, ``pi_a0`` and the control allele counts are the observed screen's: the same cells, other
    read counts.  Depth 1 is added in front of ``depths`` where absent (``design_depths``).

    Returns ``(full, fits)``: ``full`` is exactly what ``run_inference(..., seed=seed)`` returns, ``fits[i][j]`` exactly
    what it returns for the screen with the counts of depth i, draw j - bit for bit; ``fits`` follows
    ``design_depths(depths)``, and its depth-1 row is the ``boots`` of ``run_inference_bootstrap(n_boot=n_screens,
    boot_seed=design_seed)``.  The refits are members of one engine next to the screen, at most ``max_per_run``
    (1 ... 63) per engine run, where the batched kernels take the shape; else one after the other (``_fit_plan``).
    Raises ``PredictiveUnsupported`` - the message names the family - as ``run_inference_bootstrap`` does;
    ``n_screens < 2``, no depth, a depth given twice and a depth that is not > 0 are each a ``ValueError``.  A halt's
    message and dump file (``tmp_result.depth<f>_<j>.pkl``, with ``"depth": f, "screen": j``) name the screen."""
    import dataclasses

    import torch.distributed as dist

    from ..engine import PredictiveUnsupported
    from .jackknife import MAX_GUIDE_POSITIONS

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _predictive_refusal(spec, data, world)
    if why is not None:
        raise PredictiveUnsupported(f"a depth study is not available for {why}: the count simulator serves the sorting "
                                    "variant Normal and MixtureNormal models on one GPU")
    n_screens, per_run = int(n_screens), int(max_per_run)
    if n_screens < 2:
        raise ValueError(f"a depth study needs at least 2 screens per depth, got {n_screens}")
    depths = design_depths(depths)
    if not 1 <= per_run <= MAX_GUIDE_POSITIONS:
        raise ValueError(f"max_per_run must be in [1, {MAX_GUIDE_POSITIONS}] (the screen is member 0 of every run), "
                         f"got {per_run}")
    common = dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps)
    first = run_inference(model, guide, data, seed=seed, report_every=report_every, verbose=verbose, **common)
    eng = bootstrap_engine(model, guide, data, first[0])
    try:
        x, x_bc = design_screens(eng, depths, n_screens, design_seed)
        torch.cuda.synchronize(eng.device)
    finally:
        eng.close()
    home = lambda t, like: None if t is None else t.to(like.device, like.dtype)  # noqa: E731
    plan = design_plan(data, seed, depths, home(x, data.X_masked),
                       home(x_bc, data.X_bcmatch_masked) if x_bc is not None else None)
    plan = dataclasses.replace(plan, per_run=per_run)
    results = _fit_plan(model, guide, data, plan, common, report_every, verbose)
    return results[0], [results[1 + i * n_screens:1 + (i + 1) * n_screens] for i in range(len(depths))]


def power_effects(effects):
    """The planted effects of a power study as floats, effect 0 - the null, whose detection rate is the false-positive
    rate every power is read against - put in front where it is absent.  An empty list, an effect that is not finite and
    an effect given twice are each a ``ValueError``."""
    import math

    out = [float(e) for e in effects]
    if not out:
        raise ValueError("a power study needs at least one effect")
    for e in out:
        if not math.isfinite(e):
            raise ValueError(f"a planted effect must be a finite number, got {e:g}")
    twice = sorted({e for e in out if out.count(e) > 1})
    if twice:
        raise ValueError(f"effect {twice[0]:g} is given more than once")
    return out if 0.0 in out else [0.0] + out


def power_screens(eng: HipSVI, effects, n_screens: int, power_seed: int = SEED, plant=None):
    """``(X (D, K, R, B, G), X_bcmatch or None)``, device tensors: screen (i, j) is planted effect ``effects[i]``, draw j
    of ``eng.simulate_power(..., plant=plant, seed=power_seed)`` whatever the batching - calls of at most ``MAX_MEMBERS``
    screens, chunked over the effects (``D_c * K <= MAX_MEMBERS``) and, where ``K > MAX_MEMBERS``, over j with
    ``first_draw`` advancing as ``bootstrap_screens`` advances it."""
    from .._lib import MAX_MEMBERS

    effects = [float(e) for e in effects]
    K = int(n_screens)
    rows_x, rows_bc = [], []
    for j0 in range(0, K, MAX_MEMBERS):
        k = min(MAX_MEMBERS, K - j0)
        per_call = max(MAX_MEMBERS // k, 1)
        xs, xbcs = [], []
        for i0 in range(0, len(effects), per_call):
            sim = eng.simulate_power(j0, k, effects[i0:i0 + per_call], plant=plant, seed=power_seed)
            xs.append(sim["X"])
            if "X_bcmatch" in sim:
                xbcs.append(sim["X_bcmatch"])
        rows_x.append(torch.cat(xs))
        if xbcs:
            rows_bc.append(torch.cat(xbcs))
    return torch.cat(rows_x, 1), (torch.cat(rows_bc, 1) if rows_bc else None)


def run_inference_power(model, guide, data, effects, n_screens: int = 8, seed: int = SEED, power_seed: int = SEED,
                        plant=None, initial_lr=0.01, gamma=0.1, num_steps=2000, report_every: int = 100,
                        verbose: bool = True, max_per_run: int = 63):
    """Power study: fit the screen, draw ``n_screens`` screens from the fitted model on the device with each effect of
    ``effects`` planted - ``mu_t = effect``, the value itself, on every target (or on those ``plant`` marks: T booleans)
    - and refit every one of them with the same ``seed`` (``model/jackknife.py::power_plan``): how large must a variant's
    effect be for this screen to have called it, and how often does a variant with no effect cross the threshold.

    The screens are the parametric bootstrap's (``bootstrap_engine``: the plug-in, zero noise in every Normal site) with
    one change: the guides of a planted target sort with the planted mean and the target's fitted ``sd``.  Screen (i, j)
    uses the pi, Dirichlet and categorical streams of draw j of ``power_seed`` at every effect (common random numbers
    across effects).  Masks, size factors, ``a0``, ``pi_a0``, editing rates, totals and the control allele counts are the
    observed screen's.  The variant families share no parameter between targets, so every target is planted at once and
    each target's refit is still its own experiment.  Effect 0 is added in front of ``effects`` where absent
    (``power_effects``).

    Returns ``(full, fits)``: ``full`` is exactly what ``run_inference(..., seed=seed)`` returns, ``fits[i][j]`` exactly
    what it returns for the screen with the counts of effect i, draw j - bit for bit; ``fits`` follows
    ``power_effects(effects)``.  The refits are members of one engine next to the screen, at most ``max_per_run``
    (1 ... 63) per engine run, where the batched kernels take the shape; else one after the other (``_fit_plan``).
    Raises ``PredictiveUnsupported`` - the message names the family - as ``run_inference_bootstrap`` does;
    ``n_screens < 2``, no effect, an effect given twice and an effect that is not finite are each a ``ValueError``.  A
    halt's message and dump file (``tmp_result.effect<e>_<j>.pkl``, with ``"effect": e, "screen": j``) name the screen."""
    import dataclasses

    import torch.distributed as dist

    from ..engine import PredictiveUnsupported
    from .jackknife import MAX_GUIDE_POSITIONS

    spec = _resolve(model)
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    why = _predictive_refusal(spec, data, world)
    if why is not None:
        raise PredictiveUnsupported(f"a power study is not available for {why}: the count simulator serves the sorting "
                                    "variant Normal and MixtureNormal models on one GPU")
    n_screens, per_run = int(n_screens), int(max_per_run)
    if n_screens < 2:
        raise ValueError(f"a power study needs at least 2 screens per effect, got {n_screens}")
    effects = power_effects(effects)
    if not 1 <= per_run <= MAX_GUIDE_POSITIONS:
        raise ValueError(f"max_per_run must be in [1, {MAX_GUIDE_POSITIONS}] (the screen is member 0 of every run), "
                         f"got {per_run}")
    common = dict(initial_lr=initial_lr, gamma=gamma, num_steps=num_steps)
    first = run_inference(model, guide, data, seed=seed, report_every=report_every, verbose=verbose, **common)
    eng = bootstrap_engine(model, guide, data, first[0])
    try:
        x, x_bc = power_screens(eng, effects, n_screens, power_seed, plant=plant)
        torch.cuda.synchronize(eng.device)
    finally:
        eng.close()
    home = lambda t, like: None if t is None else t.to(like.device, like.dtype)  # noqa: E731
    plan = power_plan(data, seed, effects, home(x, data.X_masked),
                      home(x_bc, data.X_bcmatch_masked) if x_bc is not None else None)
    plan = dataclasses.replace(plan, per_run=per_run)
    results = _fit_plan(model, guide, data, plan, common, report_every, verbose)
    return results[0], [results[1 + i * n_screens:1 + (i + 1) * n_screens] for i in range(len(effects))]


def identify_model_guide(args):
    """Model label and (model, guide) descriptors for the parsed ``bean run``
    arguments (``bean/model/run.py:399-457``), including the reference's
    always-truthy ``use_bcmatch`` tuple and ``~bool`` ``fit_noise``."""
    if args.selection == "sorting":
        m = sorting_model
    else:
        from . import survival_model as m  # noqa: WPS433
    if args.library_design == "tiling":
        info("Using Mixture Normal model...")
        return (
            f"MultiMixtureNormal{'+Acc' if args.scale_by_acc else ''}",
            partial(m.MultiMixtureNormalModel, scale_by_accessibility=args.scale_by_acc,
                    use_bcmatch=(not args.ignore_bcmatch,)),
            partial(m.MultiMixtureNormalGuide, scale_by_accessibility=args.scale_by_acc,
                    fit_noise=~args.dont_fit_noise),
        )
    if args.uniform_edit:
        if args.guide_activity_col is not None:
            raise ValueError("Can't use the guide activity column while constraining uniform edit.")
        info("Using Normal model...")
        return ("Normal", partial(m.NormalModel, use_bcmatch=(not args.ignore_bcmatch)), m.NormalGuide)
    elif args.const_pi:
        if args.guide_activity_col is not None:
            raise ValueError("--guide-activity-col to be used as constant pi is not provided.")
        info("Using Mixture Normal model with constant weight ...")
        return (
            "MixtureNormalConstPi",
            partial(m.MixtureNormalConstPiModel, use_bcmatch=(not args.ignore_bcmatch)),
            m.MixtureNormalGuide,
        )
    else:
        info(f"Using Mixture Normal model {'with accessibility normalization' if args.scale_by_acc else ''}...")
        return (
            f"{'_' if args.dont_fit_noise else ''}MixtureNormal{'+Acc' if args.scale_by_acc else ''}",
            partial(m.MixtureNormalModel, scale_by_accessibility=args.scale_by_acc,
                    use_bcmatch=(not args.ignore_bcmatch,)),
            partial(m.MixtureNormalGuide, scale_by_accessibility=args.scale_by_acc,
                    fit_noise=(not args.dont_fit_noise)),
        )


def identify_negctrl_model_guide(args, data_has_bcmatch):
    """``bean/model/run.py:460-474``."""
    if args.selection == "sorting":
        m = sorting_model
    else:
        from . import survival_model as m  # noqa: WPS433
    negctrl_model = partial(m.ControlNormalModel, use_bcmatch=(not args.ignore_bcmatch and data_has_bcmatch))
    negctrl_guide = partial(m.ControlNormalGuide, use_bcmatch=(not args.ignore_bcmatch and data_has_bcmatch))
    return negctrl_model, negctrl_guide


# --------------------------------------------------------------------------
# argument validation and table helpers of `bean run`
# (bean/model/run.py:39-178 check_args, 181-216 _get_guide_target_info,
#  219-308 _get_guide_info, 480-542 _check_prior_params)
# --------------------------------------------------------------------------
import os  # noqa: E402

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402

warn = logger.warning


def check_args(args, bdata):
    """Validate the parsed arguments against the screen and derive ``args.popt``,
    ``args.adjust_confidence_by_negative_control`` and a default ``repguide_mask``."""
    g, s = bdata.guides, bdata.samples
    if args.scale_by_acc:
        if args.acc_col is None and args.acc_bw_path is None:
            raise ValueError(
                "--scale-by-acc not accompanied by --acc-col nor --acc-bw-path to use. Pass either one.")
        if args.acc_col is not None and args.acc_bw_path is not None:
            warn("Both --acc-col and --acc-bw-path is specified. --acc-bw-path is ignored.")
            args.acc_bw_path = None
        elif args.acc_bw_path is not None and "genomic_pos" not in g.columns:
            if "start_pos" not in g.columns:
                raise ValueError("Guides' positions not provided in ReporterScreen.guides['start_pos']. "
                                 "Please check the input.")
            g["genomic_pos"] = g["start_pos"]
            warn("'genomic_pos' not in ReporterScreen.guides.columns, using 'start_pos' to retrieve "
                 "accessibility from the bigWig file.")
    if args.outdir is None:
        args.outdir = os.path.dirname(args.bdata_path)
    if args.fit_negctrl and args.negctrl_col not in g.columns:
        raise ValueError(f"--negctrl-col argument '{args.negctrl_col}' not in ReporterScreen.guides.columns "
                         f"{g.columns}. Please check the input or do not provide --fit-negctrl flag if you don't "
                         "have the negative controls.")
    if args.selection == "sorting":
        for flag, col in (("--sorting-bin-upper-quantile-col", args.sorting_bin_upper_quantile_col),
                          ("--sorting-bin-lower-quantile-col", args.sorting_bin_lower_quantile_col)):
            if col not in s.columns:
                raise ValueError(f"{flag} argument '{col}' not in ReporterScreen.samples.columns {s.columns}. "
                                 "Please check the input.")
    elif args.selection == "survival":
        if args.time_col not in s.columns:
            raise ValueError(f"--time-col argument '{args.time_col}' not in ReporterScreen.samples.columns "
                             f"{s.columns}. Please check the input.")
        try:
            pd.to_numeric(s[args.time_col])
        except ValueError as exc:
            raise ValueError(f"ReporterScreen.samples['{args.time_col}'] provided is not numeric "
                             f"({s[args.time_col]}). Please check the input .h5ad file or your --time-col "
                             "argument.") from exc
    if args.library_design == "variant":
        args.adjust_confidence_by_negative_control = args.fit_negctrl and (
            not args.dont_adjust_confidence_by_negative_control)
    elif args.library_design == "tiling":
        args.adjust_confidence_by_negative_control = not args.dont_adjust_confidence_by_negative_control
        if args.allele_df_key is None:
            key, n = "allele_counts", len(bdata.uns["allele_counts"])
            for k, df in bdata.uns.items():
                if "allele_counts" in k and isinstance(df, pd.DataFrame) and len(df) < n:
                    key, n = k, len(df)
            warn(f"--allele-df-key not provided for tiling screen. Using the most filtered allele counts with "
                 f"{n} alleles stored in '{key}'.")
            args.allele_df_key = key
        elif args.allele_df_key not in bdata.uns:
            raise ValueError(f"--allele-df-key '{args.allele_df_key}' not in ReporterScreen.uns. Check your input.")
    else:
        raise ValueError("Invalid library_design provided. Select either 'variant' or 'tiling'.")
    if args.fit_negctrl:
        n_neg = int((g[args.negctrl_col].map(lambda v: str(v).lower()) == args.negctrl_col_value.lower()).sum())
        if not n_neg >= 10:
            raise ValueError(f"Not enough negative control guide in the input data: {n_neg}. "
                             "Please check your input arguments.")
    if args.repguide_mask is not None and args.repguide_mask not in bdata.uns.keys():
        bdata.uns[args.repguide_mask] = pd.DataFrame(
            1, index=g.index, columns=pd.unique(s[args.replicate_col]))
        warn(f"{args.bdata_path} does not have replicate x guide outlier mask. All guides are included in analysis.")
    if args.sample_mask_col == "":
        args.sample_mask_col = None
    if args.sample_mask_col is not None and args.sample_mask_col not in s.columns.tolist():
        raise ValueError(f"{args.bdata_path} does not have specified sample mask column "
                         f"`{args.sample_mask_col}` in .samples")
    if args.condition_col not in s.columns:
        raise ValueError(f"Condition column `{args.condition_col}` set by `--condition-col` not in "
                         f"ReporterScreen.samples.columns:{s.columns}. Check your input.")
    if args.selection == "survival" and args.condition_col == args.time_col:
        raise ValueError(f"Invalid to have the same `--condition-col` ({args.condition_col}) and `--time-col` "
                         f"({args.time_col}).")
    present = s[args.condition_col].astype(str).tolist()
    for c in args.control_condition.split(","):
        if c not in present:
            raise ValueError(f"No sample has control label `{args.control_condition}` (set by "
                             f"`--control-condition`)  in ReporterScreen.samples[{args.condition_col}]: "
                             f"{s[args.condition_col]}. Check your input.")
    if args.replicate_col not in s.columns:
        raise ValueError(f"Condition column set by `--replicate-col` {args.replicate_col} not in "
                         f"ReporterScreen.samples.columns:{s.columns}. Check your input.")
    if args.control_guide_tag is not None:
        if args.library_design == "variant":
            raise ValueError("`--control-guide-tag` is not used for the variant mode. Make sure you provide the "
                             "separate `target` column for negative control guide that targets different negative "
                             "control variant.")
        if not g.index.map(lambda n: args.control_guide_tag in n).any():
            raise ValueError(f"Negative control guide label `{args.control_guide_tag}` provided by "
                             "`--control-guide-tag` doesn't appear in any of the guide names. Check your input.")
    args.popt = None
    if args.alpha_if_overdispersion_fitting_fails is not None:
        try:
            b0, b1 = args.alpha_if_overdispersion_fitting_fails.split(",")
            args.popt = (float(b0), float(b1))
        except (TypeError, ValueError):
            raise ValueError(f"Input --alpha-if-overdispersion-fitting-fails "
                             f"`{args.alpha_if_overdispersion_fitting_fails}` is malformatted! "
                             "Provide [float].[float] format.")
    return args, bdata


def _get_guide_target_info(bdata, args, cols_include=()):
    """One row per target: the guide columns that are constant within a target
    (``target_*``) plus ``cols_include``, ``n_guides`` and the editing-rate summary."""
    guides = bdata.guides.copy()
    tcol = args.target_col
    n_targets = guides[tcol].nunique()
    keep = [c for c in guides.columns
            if c != tcol and (c in cols_include or (c.startswith("target_")
                                                   and len(guides[[tcol, c]].drop_duplicates()) == n_targets))]
    info_df = guides[[tcol] + keep].drop_duplicates().set_index(tcol, drop=True)
    info_df["n_guides"] = guides.groupby("target", observed=True).size()  # literal "target", as the reference
    if "edit_rate" in guides.columns:
        er = guides[[tcol, "edit_rate"]].groupby(tcol, sort=False, observed=True).agg({"edit_rate": ["mean", "std"]})
        er.columns = ["edit_rate_mean", "edit_rate_std"]
        info_df = info_df.join(er)
    return info_df


def _get_guide_info(bdata, args, guide_lfc_pseudocount: int = 5):
    """sgRNA table: editing rate and per-replicate log fold change between the extreme
    sorting bins (sorting) or the latest and earliest timepoints (survival)."""
    s = bdata.samples
    kw = dict(rep_col=args.replicate_col, compare_col=args.condition_col, pseudocount=guide_lfc_pseudocount)
    if args.selection == "sorting":
        uq, lq = args.sorting_bin_upper_quantile_col, args.sorting_bin_lower_quantile_col
        cond = s[[args.condition_col, lq, uq]].drop_duplicates()
        top = cond.loc[cond[uq] == cond[uq].max()]
        highest = top.loc[top[lq] == top[lq].max(), args.condition_col].item()
        bottom = cond.loc[cond[uq] == cond[uq].min()]
        lowest = bottom.loc[bottom[lq] == bottom[lq].min(), args.condition_col].item()
        lfc = bdata.log_fold_change_reps(highest, lowest, **kw)
    else:
        cond = s[[args.condition_col, args.time_col]].drop_duplicates()
        t = cond[args.time_col].astype(float)
        latest = cond.loc[t == t.max(), args.condition_col].item()
        earliest = cond.loc[t == t.min(), args.condition_col].item()
        lfc = bdata.log_fold_change_reps(latest, earliest, **kw)
        if args.plasmid_condition is not None:
            sel = cond.loc[cond[args.condition_col].astype(str) != args.plasmid_condition]
            ts = sel[args.time_col].astype(float)
            first_sel = sel.loc[ts == ts.min(), args.condition_col].item()
            if first_sel != earliest:
                lfc = pd.concat([lfc, bdata.log_fold_change_reps(latest, first_sel, **kw)], axis=1)
    if "edit_rate" in bdata.guides.columns:
        return pd.concat([bdata.guides[["edit_rate"]], lfc], axis=1)
    return lfc


def _check_prior_params(param_path: str, ndata):
    """Load ``--prior-params`` and bring its entries to shape ``(n_targets, 1)``."""
    if not os.path.exists(param_path):
        raise ValueError(f"Specified prior parameter file --prior-params {param_path} is not found.")
    with open(param_path, "rb") as f:
        prior = pkl.load(f)
    T = ndata.n_targets
    keys = ("sd_loc", "sd_scale", "mu_loc", "mu_scale") if ndata.selection == "sorting" else ("mu_loc", "mu_scale")
    for k in keys:
        if k not in prior or not hasattr(prior[k], "__len__"):
            continue
        if tuple(prior[k].shape) == (T,):
            prior[k] = prior[k].reshape(-1, 1)
        elif tuple(prior[k].shape) != (T, 1):
            raise ValueError(f"Specified prior parameter --prior-params {param_path}: prior_params['{k}'].shape "
                             f"{tuple(prior[k].shape)} does not match the number of target variants {(T, 1)}.")
    if ndata.selection != "sorting" and "initial_abundance" in prior:
        if tuple(prior["initial_abundance"].shape) != (T,):
            raise ValueError(f"Specified prior parameter --prior-params {param_path}: "
                             "prior_params['initial_abundance'].shape does not match.")
    return prior
