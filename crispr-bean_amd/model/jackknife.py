"""Replicate jackknife: which replicate carries a hit (``run_inference_jackknife``, ``bean run --jackknife-replicates``).

Next to the fit of the whole screen, one fit per replicate with that replicate left out - all with the SAME seed, so that
with common random numbers the differences between the fits come from the data and not from the random stream.

Masked, not removed.  ``leave_out`` is what the reference does with a replicate masked through its own options
(``--sample-mask-col``, ``--repguide-mask``): the replicate stays in every tensor, its rows of the two masks are zero.
Its counts then enter no likelihood term - no gradient, and the reported loss only loses their data-only constant - but
the guide side is unmasked: a masked (replicate, guide) pair still draws its ``pi`` and contributes the variational entropy
of ``q(pi)``.  A fit of the screen with the replicate absent would have no such site; the two are different models, and
this one is the reference's.  Size factors, ``a0`` and the other derived tensors are those of the whole screen.

Guide jackknife: is a hit carried by one guide (``run_inference_guide_jackknife``, ``bean run --jackknife-guides``).

The same, with guides left out instead of replicates (``leave_out_guides``: the guide's column of ``repguide_mask`` is
zero, nothing else).  In the sorting variant families without sample covariates the targets share no parameter and the
random streams are keyed by global index, so one fit that masks position j of EVERY target gives every target t exactly
the fit in which only guide (t, j) is masked: all G leave-one-guide-out fits are ``1 + Lmax`` members
(``guide_positions``, ``guide_member_masks``, ``guide_jackknife_summary``).

Sample jackknife: which single sorted sample carries or distorts a hit (``run_inference_sample_jackknife``, ``bean run
--jackknife-samples`` / ``--jackknife-conditions``).

A sample is one condition (bin) of one replicate.  ``leave_out_samples`` masks it the way the reference does through
``--sample-mask-col``: its entry of ``sample_mask`` is zero AND its counts are zero (the reference fits ``X * sample_mask``).
The counts matter: the (replicate, guide) site of a masked sample stays on, and the likelihood sums the counts of every
bin whatever the sample mask says, so the members of such a jackknife differ in their data, not in their masks alone
(``sample_member_masks``, ``sample_member_counts``, ``sample_jackknife_summary``).

Parametric bootstrap: how far would ``mu`` move if the experiment were repeated under the fitted model
(``run_inference_bootstrap``, ``bean run --bootstrap K``).

K screens drawn from the fitted model on the device (``HipSVI.simulate_members``) and refitted with the screen's seed:
``bootstrap_plan``, ``bootstrap_summary``.  The members differ in their counts alone; everything derived from the observed
screen is conditioned on.

Depth study: would sequencing deeper (or shallower) change the spread of ``mu`` (``run_inference_design``, ``bean run
--design-depths``).

The bootstrap's screens drawn at other read depths (``HipSVI.simulate_design``): every (replicate, guide) draws
``floor(f * n_obs + 0.5)`` reads, everything else as observed - the same cells, other read counts: ``design_plan``,
``design_summary``.

Power study: how large must a variant's effect be for this screen to have called it, and how often does a variant with no
effect cross the threshold (``run_inference_power``, ``bean run --power-effects``).

The bootstrap's screens drawn with an effect planted (``HipSVI.simulate_power``): the guides of every planted target sort
with ``mu_t = effect``, the value itself, everything else as fitted and observed: ``power_plan``, ``power_summary``.

Each of these, and the seed ensemble, is K fits of one screen: a ``MemberPlan``, fitted by ``model/run.py::_fit_plan``.

Pure torch: no GPU involved in this file.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch


@dataclass(frozen=True)
class MemberPlan:
    """K fits of one screen, in member order: everything ``model/run.py::_fit_plan`` needs to fit them as members of
    one engine or, where the batched kernels do not take the shape, one after the other."""
    seeds: Sequence[int]
    labels: Sequence[str]  # what a halt's message calls member k
    tags: Sequence[str]  # a halt dumps member k to tmp_result.<tags[k]>.pkl ...
    dump_extra: Sequence[dict]  # ... with these fields next to "param"
    screen: Callable[[int], object]  # member k's screen: ``data`` itself, or a ``leave_out*`` copy
    differ_in: Tuple[str, ...] = ()  # what the members' screens differ in: (), ("masks",) or ("masks", "counts")
    per_run: Optional[int] = None  # members next to member 0 that one engine run may hold; None: all in one
    label_halts: bool = False  # one after the other: append "(label)" to a halt's message
    chosen: tuple = ()  # what the constructor chose (left-out replicates, positions, groups ...), for the caller


def stack_masks(screens):
    """``(repguide (K, R, G) bool, sample_mask (K, R, B))`` of K screens, in their order."""
    return torch.stack([s.repguide_mask != 0 for s in screens]), torch.stack([s.sample_mask for s in screens])


def stack_counts(screens):
    """``(X (K, R, B, G), X_bcmatch (K, R, B, G) or None)`` of K screens, float32: their ``X_masked`` and, where the
    first has them, ``X_bcmatch_masked``."""
    x = torch.stack([s.X_masked.to(torch.float32) for s in screens])
    if getattr(screens[0], "X_bcmatch_masked", None) is None:
        return x, None
    return x, torch.stack([s.X_bcmatch_masked.to(torch.float32) for s in screens])


def seed_plan(data, seeds) -> MemberPlan:
    """A seed ensemble: member k is the screen itself with ``seeds[k]``.  No seed is a ``ValueError``."""
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError("run_inference_ensemble needs at least one seed")
    ks = range(len(seeds))
    return MemberPlan(seeds, [f"member {k}" for k in ks], [f"member{k}" for k in ks],
                      [{"member": k, "seed": seeds[k]} for k in ks], screen=lambda k: data)


PARTICLE_SEED_STRIDE = 1_000_003


def particle_seeds(seed: int, n_particles: int) -> List[int]:
    """The seeds of a multi-particle fit's draws (``HipSVI.run_particles``, ``run_inference(num_particles=P)``): particle
    p draws with ``seed + 1_000_003 * p``, so particle 0 is the fit's own seed.  ``n_particles < 1`` is a ``ValueError``."""
    if int(n_particles) < 1:
        raise ValueError(f"n_particles must be >= 1, got {int(n_particles)}")
    return [int(seed) + PARTICLE_SEED_STRIDE * p for p in range(int(n_particles))]


def _leave_one_out_plan(data, seed, items, label, tag, key, value, leave, **more) -> MemberPlan:
    """One seed for all: member 0 is the screen itself, member 1 + j is ``leave(data, items[j])``."""
    seed = int(seed)
    return MemberPlan(
        seeds=[seed] * (1 + len(items)),
        labels=["the full screen"] + [label(x) for x in items],
        tags=["full"] + [tag(x) for x in items],
        dump_extra=[{key: None, "seed": seed}] + [{key: value(x), "seed": seed} for x in items],
        screen=lambda k: data if k == 0 else leave(data, items[k - 1]), **more)


def leave_out(data, r: int):
    """A copy of the screen with replicate ``r`` masked: ``sample_mask[r, :] = 0`` and ``repguide_mask[r, :] = False``,
    nothing else touched (counts, ``X_masked``, size factors, ``a0`` are the whole screen's, shared with ``data``).
    This is the reference's fit with the replicate masked through its own options, not its fit with the replicate
    absent: the q(pi) entropy of the masked (replicate, guide) pairs stays in the loss.  ``data`` is not modified."""
    r = int(r)
    if not 0 <= r < int(data.n_reps):
        raise ValueError(f"replicate {r} of a screen with {int(data.n_reps)} replicates")
    out = copy.copy(data)
    out.sample_mask = data.sample_mask.clone()
    out.sample_mask[r, :] = 0
    out.repguide_mask = data.repguide_mask.clone()
    out.repguide_mask[r, :] = False
    return out


def candidate_replicates(data) -> List[int]:
    """The replicates a jackknife leaves out: those that are not already fully masked (a replicate whose rows of both
    masks are zero throughout: leaving it out would repeat the full fit).  Fewer than two is a ``ValueError``."""
    sm = data.sample_mask.detach().cpu() != 0
    rg = data.repguide_mask.detach().cpu() != 0
    cand = [r for r in range(int(data.n_reps)) if bool(sm[r].any()) or bool(rg[r].any())]
    if len(cand) < 2:
        raise ValueError(f"a replicate jackknife needs at least two replicates that are not fully masked, found {len(cand)}")
    return cand


def member_masks(data, left_out: Sequence[int]):
    """``stack_masks`` of the screen and of ``leave_out(data, r)`` for every r of ``left_out``."""
    return stack_masks([data] + [leave_out(data, r) for r in left_out])


def replicate_plan(data, seed) -> MemberPlan:
    """A replicate jackknife: the screen and, per replicate of ``candidate_replicates``, the screen without it."""
    left_out = candidate_replicates(data)
    return _leave_one_out_plan(data, seed, left_out, label=lambda r: f"replicate {r} left out",
                               tag=lambda r: f"without_replicate{r}", key="left_out", value=lambda r: r,
                               leave=leave_out, differ_in=("masks",), chosen=(left_out,))


def _param(result, name) -> torch.Tensor:
    store = result[0] if isinstance(result, (tuple, list)) else result
    return store[name].detach().cpu().to(torch.float64)


def _mu_loc(result) -> torch.Tensor:
    return _param(result, "mu_loc")


def jackknife_summary(full, loo, left_out: Sequence[int], replicate_names: Sequence) -> Dict[str, object]:
    """Delete-one summary of ``mu_loc`` (float64).  With ``m_j`` the ``mu_loc`` of ``loo[j]``, ``n = len(loo)`` and
    ``mbar = mean_j m_j``:

    * ``mu_jk_se = sqrt((n - 1) / n * sum_j (m_j - mbar)^2)`` - the jackknife standard error;
    * ``mu_jk_max_shift = max_j |m_j - mu_loc_full|`` and ``mu_jk_max_shift_rep``, the name of the replicate whose
      removal moves the target that far, a list with one name per target;
    * ``n_jk = n``.

    ``full`` / ``loo[j]`` are results of ``run_inference`` (or their stores / dicts); ``replicate_names[r]`` names
    replicate r, ``left_out[j]`` is the replicate ``loo[j]`` leaves out."""
    n = len(loo)
    if n < 2 or n != len(left_out):
        raise ValueError(f"jackknife_summary needs at least two leave-one-out fits and their replicates, got {n} / {len(left_out)}")
    m = torch.stack([_mu_loc(r) for r in loo])
    centre = _mu_loc(full)
    se = torch.sqrt((n - 1) / n * ((m - m.mean(0)) ** 2).sum(0))
    shift = (m - centre).abs()
    worst = shift.argmax(0)
    names = [str(replicate_names[int(left_out[int(j)])]) for j in worst.reshape(-1)]
    return {"mu_jk_se": se, "mu_jk_max_shift": shift.max(0).values, "mu_jk_max_shift_rep": names, "n_jk": n}


# ---------------------------------------------------------------- guides
MAX_GUIDE_POSITIONS = 63  # BEAN_HIP_MAX_MEMBERS - 1: the full screen is member 0


def leave_out_guides(data, guides):
    """A copy of the screen with the guides ``guides`` (indices, or one index) masked: ``repguide_mask[:, guides] =
    False`` and nothing else touched - masked, not removed, as ``leave_out``: the guides keep their ``pi`` draws and the
    entropy of ``q(pi)``, their counts enter no likelihood term.  ``data`` is not modified."""
    idx = torch.as_tensor(guides, dtype=torch.int64).reshape(-1).cpu()
    G = int(data.n_guides)
    bad = idx[(idx < 0) | (idx >= G)]
    if bad.numel():
        raise ValueError(f"guide {int(bad[0])} of a screen with {G} guides")
    out = copy.copy(data)
    out.repguide_mask = data.repguide_mask.clone()
    out.repguide_mask[:, idx.to(out.repguide_mask.device)] = False
    return out


def _guide_layout(data):
    offsets = data.target_offsets.detach().cpu()
    return offsets[:-1], offsets[1:] - offsets[:-1]


def guide_positions(data, max_positions: int = MAX_GUIDE_POSITIONS) -> Tuple[List[int], torch.Tensor]:
    """``(positions, included)`` of a guide jackknife.  ``positions`` are the j in ``[0, min(Lmax, max_positions))``,
    Lmax the longest target; ``included`` is ``(T, len(positions))`` bool, true where target t has a guide at
    ``target_offsets[t] + j`` that is not already masked in every replicate (leaving that one out would repeat the
    full fit).  Targets with more than ``max_positions`` guides are left out of the jackknife entirely (their row is
    false): a delete-one statistic over some of a target's guides would not be one.  No included pair at all, or
    ``max_positions`` outside ``[1, 63]``, is a ``ValueError``."""
    max_positions = int(max_positions)
    if not 1 <= max_positions <= MAX_GUIDE_POSITIONS:
        raise ValueError(f"a guide jackknife takes 1 to {MAX_GUIDE_POSITIONS} positions per target "
                         f"(one member each, next to the full screen), got {max_positions}")
    start, length = _guide_layout(data)
    n_pos = min(int(length.max()) if length.numel() else 0, max_positions)
    j = torch.arange(n_pos)
    present = (j[None, :] < length[:, None]) & (length <= max_positions)[:, None]
    alive = (data.repguide_mask.detach().cpu() != 0).any(0)
    g = (start[:, None] + j[None, :]).clamp(max=max(int(data.n_guides) - 1, 0))
    included = present & alive[g]
    if not bool(included.any()):
        raise ValueError(f"a guide jackknife needs at least one guide to leave out: no target of at most "
                         f"{max_positions} guides has a guide that is not already fully masked")
    return list(range(n_pos)), included


def guides_at_position(data, j: int) -> torch.Tensor:
    """The guide at position j of every target that has one."""
    start, length = _guide_layout(data)
    return (start + int(j))[length > int(j)]


def guide_member_masks(data, positions: Sequence[int]):
    """``stack_masks`` of the screen and, for every j of ``positions``, of the screen with the guide at position j of
    every target that has one masked."""
    return stack_masks([data] + [leave_out_guides(data, guides_at_position(data, j)) for j in positions])


def guide_plan(data, seed, max_positions: int = MAX_GUIDE_POSITIONS) -> MemberPlan:
    """A guide jackknife: the screen and, per position of ``guide_positions``, the screen without the guide at that
    position of every target.  One after the other, a halt's message gets the member's label."""
    positions, included = guide_positions(data, max_positions)
    return _leave_one_out_plan(data, seed, positions, label=lambda j: f"guides at position {j} of their targets left out",
                               tag=lambda j: f"without_guide_position{j}", key="left_out_position", value=lambda j: j,
                               leave=lambda d, j: leave_out_guides(d, guides_at_position(d, j)),
                               differ_in=("masks",), label_halts=True, chosen=(positions, included))


def guide_jackknife_summary(full, loo, positions: Sequence[int], included, data, guide_names: Sequence) -> Dict[str, object]:
    """Delete-one-guide summary of ``mu_loc`` (float64).  ``loo[i]`` is the fit that leaves position ``positions[i]``
    out everywhere; target t reads ITS ``mu_loc`` from it: ``m_tj``, for the included j of t, ``n_t`` their count,
    ``mbar_t`` their mean.

    * ``mu_gjk_se[t] = sqrt((n_t - 1) / n_t * sum_j (m_tj - mbar_t)^2)``;
    * ``mu_gjk_max_shift[t] = max_j |m_tj - mu_loc_full[t]|`` and ``mu_gjk_max_shift_guide``, the name of the guide
      whose removal moves the target that far, a list with one name per target;
    * ``n_gjk[t] = n_t`` (int64);
    * ``mu_shift_left_out[g] = m_tj - mu_loc_full[t]`` of guide g = (t, j), NaN for guides that were not left out.

    The first three are ``(T,)``; targets with ``n_t < 2`` get NaN, the empty name, and their ``n_t``."""
    included = torch.as_tensor(included).detach().cpu().bool()
    T, n_pos = included.shape
    if n_pos != len(positions) or n_pos != len(loo):
        raise ValueError(f"guide_jackknife_summary needs one fit per position, got {len(loo)} fits, {len(positions)} "
                         f"positions and {n_pos} columns of `included`")
    centre = _mu_loc(full).reshape(-1)
    if centre.numel() != T:
        raise ValueError(f"`included` has {T} targets, mu_loc {centre.numel()}")
    start, _ = _guide_layout(data)
    nan = float("nan")
    m = torch.stack([_mu_loc(r).reshape(-1) for r in loo], dim=1) if n_pos else torch.zeros(T, 0, dtype=torch.float64)
    n = included.sum(1)
    enough = n >= 2
    nf = n.clamp(min=1).to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    mbar = torch.where(included, m, zero).sum(1) / nf
    ss = torch.where(included, (m - mbar[:, None]) ** 2, zero).sum(1)
    shift = m - centre[:, None]
    size = torch.where(included, shift.abs(), torch.full((), -1.0, dtype=torch.float64))
    worst = size.argmax(1) if n_pos else torch.zeros(T, dtype=torch.int64)
    se = torch.where(enough, torch.sqrt((nf - 1) / nf * ss), torch.full((), nan, dtype=torch.float64))
    far = torch.where(enough, size.max(1).values if n_pos else torch.zeros(T, dtype=torch.float64),
                      torch.full((), nan, dtype=torch.float64))
    names = [str(guide_names[int(start[t]) + int(positions[int(worst[t])])]) if bool(enough[t]) else "" for t in range(T)]
    per_guide = torch.full((int(data.n_guides),), nan, dtype=torch.float64)
    t_idx, i_idx = torch.nonzero(included, as_tuple=True)
    per_guide[start[t_idx] + torch.as_tensor(list(positions), dtype=torch.int64)[i_idx]] = shift[t_idx, i_idx]
    return {"mu_gjk_se": se, "mu_gjk_max_shift": far, "mu_gjk_max_shift_guide": names, "n_gjk": n.to(torch.int64),
            "mu_shift_left_out": per_guide}


# ---------------------------------------------------------------- samples
def leave_out_samples(data, pairs):
    """A copy of the screen with the samples ``pairs`` - ``(replicate, condition)`` index pairs - masked: for every
    ``(r, b)``, ``sample_mask[r, b] = 0``, ``X_masked[r, b, :] = 0`` and, where the screen has it,
    ``X_bcmatch_masked[r, b, :] = 0``; nothing else is touched.  This is the screen the reference fits with those samples
    masked through ``--sample-mask-col`` (``X_masked = X * sample_mask``), except that size factors, ``a0`` and the other
    derived tensors stay the whole screen's - as ``leave_out`` rules for replicates, and for the same reason: the fits
    are to differ through the left-out data alone.  Works on every data class (sorting, survival, tiling); ``data`` is
    not modified.  An index out of range is a ``ValueError``."""
    R, B = int(data.n_reps), int(data.n_condits)
    clean = []
    for pair in pairs:
        try:
            r, b = pair
            r, b = int(r), int(b)
        except (TypeError, ValueError):
            raise ValueError(f"a sample is a (replicate, condition) pair, got {pair!r}") from None
        if not (0 <= r < R and 0 <= b < B):
            raise ValueError(f"sample ({r}, {b}) of a screen with {R} replicates x {B} conditions")
        clean.append((r, b))
    out = copy.copy(data)
    out.sample_mask = data.sample_mask.clone()
    out.X_masked = data.X_masked.clone()
    has_bc = getattr(data, "X_bcmatch_masked", None) is not None
    if has_bc:
        out.X_bcmatch_masked = data.X_bcmatch_masked.clone()
    for r, b in clean:
        out.sample_mask[r, b] = 0
        out.X_masked[r, b, :] = 0
        if has_bc:
            out.X_bcmatch_masked[r, b, :] = 0
    return out


def sample_groups(data, by: str = "sample") -> Tuple[List[List[Tuple[int, int]]], List[str]]:
    """``(groups, names)`` of a sample jackknife: ``groups[j]`` is the list of ``(r, b)`` pairs member 1 + j leaves out,
    ``names[j]`` its fallback name.

    * ``by="sample"``: one group per ``(r, b)`` with ``sample_mask[r, b] != 0`` whose replicate is not already fully
      masked in ``repguide_mask`` (leaving such a sample out would repeat the full fit); named ``r{r}_c{b}``.
    * ``by="condition"``: one group per condition b, holding its candidate ``(r, b)`` over all replicates (a condition
      without any is no group); named ``c{b}``.

    The candidates are the cells of ``sample_mask``, i.e. the conditions on the screen's condition axis.  The separate
    control / bulk tensors (``control_sample_mask``, ``X_control``, ``allele_counts_control``) are not candidates and are
    never touched: they feed ``pi_a0`` and the edit-rate site, not a bin of the sort.  Fewer than two groups is a
    ``ValueError``."""
    if by not in ("sample", "condition"):
        raise ValueError(f"sample_groups: by must be 'sample' or 'condition', got {by!r}")
    sm = data.sample_mask.detach().cpu() != 0
    alive = (data.repguide_mask.detach().cpu() != 0).any(1)
    R, B = int(data.n_reps), int(data.n_condits)
    cand = [(r, b) for r in range(R) for b in range(B) if bool(sm[r, b]) and bool(alive[r])]
    if by == "sample":
        groups = [[p] for p in cand]
        names = [f"r{r}_c{b}" for r, b in cand]
    else:
        groups = [[p for p in cand if p[1] == b] for b in range(B)]
        names = [f"c{b}" for b in range(B) if groups[b]]
        groups = [g for g in groups if g]
    if len(groups) < 2:
        raise ValueError(f"a sample jackknife needs at least two {by}s that are not already masked, found {len(groups)}")
    return groups, names


def sample_member_masks(data, groups):
    """``stack_masks`` of the screen and of ``leave_out_samples(data, g)`` for every g of ``groups``."""
    return stack_masks([data] + [leave_out_samples(data, g) for g in groups])


def sample_member_counts(data, groups):
    """``stack_counts`` of the screen and of ``leave_out_samples(data, g)`` for every g of ``groups``."""
    return stack_counts([data] + [leave_out_samples(data, g) for g in groups])


def sample_plan(data, by: str, seed: int, max_groups_per_run: int = MAX_GUIDE_POSITIONS) -> MemberPlan:
    """A sample jackknife: the screen and, per group of ``sample_groups(data, by)``, the screen without it - other masks
    AND other counts - in engine runs of at most ``max_groups_per_run`` groups next to the full screen (outside
    ``[1, 63]``: ``ValueError``).  One after the other, a halt's message gets the member's label."""
    per_run = int(max_groups_per_run)
    if not 1 <= per_run <= MAX_GUIDE_POSITIONS:
        raise ValueError(f"max_groups_per_run must be in [1, {MAX_GUIDE_POSITIONS}] (the full screen is member 0 of "
                         f"every run), got {per_run}")
    groups, names = sample_groups(data, by)
    return _leave_one_out_plan(data, seed, list(zip(names, groups)), label=lambda x: f"{by} {x[0]} left out",
                               tag=lambda x: f"without_{x[0]}", key="left_out", value=lambda x: [list(p) for p in x[1]],
                               leave=lambda d, x: leave_out_samples(d, x[1]), differ_in=("masks", "counts"),
                               per_run=per_run, label_halts=True, chosen=(groups, names))


def sample_jackknife_summary(full, loo, groups, names: Sequence) -> Dict[str, object]:
    """Leave-one-sample-out summary of ``mu_loc`` (float64).  With ``m_j`` the ``mu_loc`` of ``loo[j]``, ``c`` the full
    fit's ``mu_loc`` and ``s`` its ``mu_scale``:

    per target
      * ``mu_sjk_max_shift = max_j |m_j - c|`` and ``mu_sjk_max_shift_sample``, the name of the group whose removal moves
        the target that far (ties: the first such group), a list with one name per target;
      * ``n_sjk = len(loo)``;

    per group - ``influence``, a dict of lists in the order of ``groups`` (the influence table)
      * ``left_out`` (the name), ``n_samples`` (pairs in the group),
      * ``influence_median = median_t |m_j - c| / s`` and ``influence_max`` (the median of an even number of targets is
        the mean of the two middle ones),
      * ``n_targets_moved = #{t : |m_j - c| > s}``.

    There is NO jackknife standard error here, on purpose: the samples of different bins are not exchangeable units (a
    top bin and a bottom bin carry opposite information about ``mu``), so a delete-one variance over them would be a
    number that looks like a standard error and is none."""
    n = len(loo)
    if n < 2 or n != len(groups) or n != len(names):
        raise ValueError(f"sample_jackknife_summary needs at least two leave-one-out fits with their groups and names, "
                         f"got {n} / {len(groups)} / {len(names)}")
    m = torch.stack([_mu_loc(r).reshape(-1) for r in loo])
    centre = _mu_loc(full).reshape(-1)
    scale = _param(full, "mu_scale").reshape(-1)
    shift = (m - centre).abs()
    far, worst = shift.max(0)
    # (torch.max leaves the index among ties open: the first group that reaches the maximum)
    worst = (shift == far).to(torch.int64).argmax(0)
    rel = shift / scale
    influence = {
        "left_out": [str(x) for x in names],
        "n_samples": [len(g) for g in groups],
        "influence_median": [float(torch.quantile(rel[j], 0.5)) for j in range(n)],
        "influence_max": [float(rel[j].max()) for j in range(n)],
        "n_targets_moved": [int((shift[j] > scale).sum()) for j in range(n)],
    }
    return {"mu_sjk_max_shift": far, "mu_sjk_max_shift_sample": [str(names[int(j)]) for j in worst], "n_sjk": n,
            "influence": influence}


# ---------------------------------------------------------------- parametric bootstrap
def bootstrap_plan(data, seed, x, x_bcmatch=None) -> MemberPlan:
    """A parametric bootstrap: member 0 is the screen, member 1 + j a ``copy.copy(data)`` whose ``X_masked`` is plane j
    of ``x`` (K, R, B, G) and, where ``x_bcmatch`` is given, whose ``X_bcmatch_masked`` is plane j of it - the screens
    ``HipSVI.simulate_members`` drew from the fitted model.

    Conditioned on: everything else is the observed screen's, shared with ``data`` - both masks, the size factors,
    ``a0`` / ``a0_bcmatch``, ``pi_a0`` and the control allele counts it derives from, and every (replicate, guide)
    total (the simulator keeps them).  The bootstrap answers "how far does mu move when the sorted counts are redrawn at
    this depth, dispersion and prior", not what re-deriving those from each redrawn screen would add.

    Every member gets ``seed``: common random numbers, so the members differ through their data and not through the
    stream.  An engine run holds the screen and at most 63 bootstrap screens.  ``data`` is not modified."""
    seed = int(seed)
    K = int(x.shape[0])
    if x_bcmatch is not None and tuple(x_bcmatch.shape) != tuple(x.shape):
        raise ValueError(f"x_bcmatch has shape {tuple(x_bcmatch.shape)}, x {tuple(x.shape)}")

    def screen(data, j):
        out = copy.copy(data)
        out.X_masked = x[j]
        if x_bcmatch is not None:
            out.X_bcmatch_masked = x_bcmatch[j]
        return out

    return _leave_one_out_plan(data, seed, list(range(K)), label=lambda j: f"bootstrap screen {j}",
                               tag=lambda j: f"bootstrap{j}", key="bootstrap", value=lambda j: j, leave=screen,
                               differ_in=("masks", "counts"), per_run=MAX_GUIDE_POSITIONS, label_halts=True)


def bootstrap_summary(full, boots) -> Dict[str, object]:
    """Parametric-bootstrap summary of ``mu_loc`` (float64).  With ``m_j`` the ``mu_loc`` of ``boots[j]``:

    * ``mu_boot_se``: the standard deviation of ``m_j`` over j, unbiased (n - 1) - the frequentist spread the
      mean-field ``mu_sd`` can be held against;
    * ``mu_boot_bias = mean_j m_j - mu_loc_full``;
    * ``n_boot = len(boots)``.

    Fewer than two fits are a ``ValueError``."""
    n = len(boots)
    if n < 2:
        raise ValueError(f"bootstrap_summary needs at least two bootstrap fits, got {n}")
    m = torch.stack([_mu_loc(r) for r in boots])
    return {"mu_boot_se": m.std(0, unbiased=True), "mu_boot_bias": m.mean(0) - _mu_loc(full), "n_boot": n}


# ---------------------------------------------------------------- depth study
def depth_text(f) -> str:
    """A depth factor as labels, tags and column names show it: ``{f:g}``."""
    return f"{float(f):g}"


def design_plan(data, seed, depths, x, x_bcmatch=None) -> MemberPlan:
    """A depth study: member 0 is the screen, member ``1 + i * K + j`` a ``copy.copy(data)`` whose ``X_masked`` is plane
    ``(i, j)`` of ``x`` (D, K, R, B, G) - depth ``depths[i]``, draw j, the screens ``HipSVI.simulate_design`` drew from the
    fitted model - and, where ``x_bcmatch`` is given, whose ``X_bcmatch_masked`` is plane ``(i, j)`` of it.

    Conditioned on, as in ``bootstrap_plan``: both masks, the size factors, ``a0`` / ``a0_bcmatch``, ``pi_a0`` and the
    control allele counts are the observed screen's, shared with ``data`` - the same cells, other read counts.  Every
    member gets ``seed``; an engine run holds the screen and at most 63 of the screens.  ``data`` is not modified."""
    seed = int(seed)
    depths = [float(f) for f in depths]
    if x.dim() != 5 or int(x.shape[0]) != len(depths):
        raise ValueError(f"x has shape {tuple(x.shape)}: (D, K, R, B, G) with D = {len(depths)} depths is needed")
    if x_bcmatch is not None and tuple(x_bcmatch.shape) != tuple(x.shape):
        raise ValueError(f"x_bcmatch has shape {tuple(x_bcmatch.shape)}, x {tuple(x.shape)}")
    K = int(x.shape[1])

    def screen(data, ij):
        i, j = ij
        out = copy.copy(data)
        out.X_masked = x[i, j]
        if x_bcmatch is not None:
            out.X_bcmatch_masked = x_bcmatch[i, j]
        return out

    items = [(i, j) for i in range(len(depths)) for j in range(K)]
    plan = _leave_one_out_plan(data, seed, items, label=lambda ij: f"depth {depth_text(depths[ij[0]])} screen {ij[1]}",
                               tag=lambda ij: f"depth{depth_text(depths[ij[0]])}_{ij[1]}", key="depth",
                               value=lambda ij: depths[ij[0]], leave=screen, differ_in=("masks", "counts"),
                               per_run=MAX_GUIDE_POSITIONS, label_halts=True)
    extra = [{"depth": e["depth"], "screen": None if k == 0 else items[k - 1][1], "seed": seed}
             for k, e in enumerate(plan.dump_extra)]
    return replace(plan, dump_extra=extra)


def design_totals(n_obs, depth):
    """``floor(depth * n_obs + 0.5)`` in float64: the reads a pair of ``n_obs`` observed reads draws at ``depth``."""
    return torch.floor(torch.as_tensor(n_obs, dtype=torch.float64) * float(depth) + 0.5)


def design_summary(full, fits, depths, z_hit: float = 1.96, data=None) -> Dict[str, object]:
    """Depth-study summary (float64).  ``fits[i][j]`` is the refit of draw j at depth ``depths[i]``, ``m_ij`` / ``s_ij``
    its ``mu_loc`` / ``mu_scale``; ``depths`` holds the baseline depth 1.

    * ``mu_design_se`` (D, T): the standard deviation of ``m_ij`` over j, unbiased (K - 1);
    * ``mu_design_sd`` (D, T): the mean of ``s_ij`` over j;
    * ``se_ratio`` (D,): the median over targets of ``mu_design_se[i] / mu_design_se[depth 1]``; targets whose
      denominator is zero or not finite are left out, ``n_left_out`` counts them (all left out: NaN);
    * ``hits``: the targets (sorted indices) with ``|mu_loc_full| / mu_scale_full >= z_hit``; ``n_hits``;
    * ``recovery`` (D,): the share of (hit, j) with ``sign(m_ij) == sign(mu_loc_full)`` and ``|m_ij| / s_ij >= z_hit``;
      NaN where there is no hit;
    * ``n_screens`` = K, ``depths``, and ``median_total`` (D,): the median of ``floor(depth * n_obs + 0.5)`` over the
      (replicate, guide) pairs of ``data`` that ``repguide_mask`` keeps (NaN without ``data``).

    Fewer than two screens at a depth, depths and fits of different lengths, or no depth 1 are a ``ValueError``."""
    depths = [float(f) for f in depths]
    D = len(depths)
    if D < 1 or D != len(fits):
        raise ValueError(f"design_summary needs one list of fits per depth, got {len(fits)} for {D} depths")
    K = len(fits[0])
    if K < 2 or any(len(row) != K for row in fits):
        raise ValueError(f"design_summary needs at least two screens at every depth, the same number at each, got "
                         f"{[len(row) for row in fits]}")
    if 1.0 not in depths:
        raise ValueError(f"design_summary needs depth 1, the baseline of every ratio, among {depths}")
    base = depths.index(1.0)
    m = torch.stack([torch.stack([_mu_loc(r).reshape(-1) for r in row]) for row in fits])  # (D, K, T)
    s = torch.stack([torch.stack([_param(r, "mu_scale").reshape(-1) for r in row]) for row in fits])
    centre, scale = _mu_loc(full).reshape(-1), _param(full, "mu_scale").reshape(-1)
    se = m.std(1, unbiased=True)
    den = se[base]
    ok = torch.isfinite(den) & (den != 0)
    nan = float("nan")
    ratio = torch.stack([torch.quantile(se[i][ok] / den[ok], 0.5) if bool(ok.any()) else torch.tensor(nan, dtype=torch.float64)
                         for i in range(D)])
    hit = (centre.abs() / scale) >= float(z_hit)
    found = (torch.sign(m) == torch.sign(centre)) & ((m.abs() / s) >= float(z_hit))  # (D, K, T)
    n_hits = int(hit.sum())
    recovery = (found[:, :, hit].to(torch.float64).mean((1, 2)) if n_hits
                else torch.full((D,), nan, dtype=torch.float64))
    median_total = torch.full((D,), nan, dtype=torch.float64)
    if data is not None:
        n_obs = data.X_masked.detach().cpu().to(torch.float64).sum(1)  # (R, G)
        kept = n_obs[data.repguide_mask.detach().cpu() != 0]
        if kept.numel():
            median_total = torch.stack([torch.quantile(design_totals(kept, f), 0.5) for f in depths])
    return {"mu_design_se": se, "mu_design_sd": s.mean(1), "se_ratio": ratio, "n_left_out": int((~ok).sum()),
            "hits": torch.nonzero(hit).reshape(-1).tolist(), "n_hits": n_hits, "recovery": recovery, "n_screens": K,
            "median_total": median_total, "depths": depths}


# ---------------------------------------------------------------- power study
def effect_text(e) -> str:
    """A planted effect as labels, tags and column names show it: ``{e:g}``."""
    return f"{float(e):g}"


def power_plan(data, seed, effects, x, x_bcmatch=None) -> MemberPlan:
    """A power study: member 0 is the screen, member ``1 + i * K + j`` a ``copy.copy(data)`` whose ``X_masked`` is plane
    ``(i, j)`` of ``x`` (D, K, R, B, G) - planted effect ``effects[i]``, draw j, the screens ``HipSVI.simulate_power`` drew
    from the fitted model - and, where ``x_bcmatch`` is given, whose ``X_bcmatch_masked`` is plane ``(i, j)`` of it.

    Conditioned on, as in ``bootstrap_plan``: both masks, the size factors, ``a0`` / ``a0_bcmatch``, ``pi_a0`` and the
    control allele counts are the observed screen's, shared with ``data``.  Every member gets ``seed``; an engine run holds
    the screen and at most 63 of the screens.  ``data`` is not modified."""
    seed = int(seed)
    effects = [float(e) for e in effects]
    if x.dim() != 5 or int(x.shape[0]) != len(effects):
        raise ValueError(f"x has shape {tuple(x.shape)}: (D, K, R, B, G) with D = {len(effects)} effects is needed")
    if x_bcmatch is not None and tuple(x_bcmatch.shape) != tuple(x.shape):
        raise ValueError(f"x_bcmatch has shape {tuple(x_bcmatch.shape)}, x {tuple(x.shape)}")
    K = int(x.shape[1])

    def screen(data, ij):
        i, j = ij
        out = copy.copy(data)
        out.X_masked = x[i, j]
        if x_bcmatch is not None:
            out.X_bcmatch_masked = x_bcmatch[i, j]
        return out

    items = [(i, j) for i in range(len(effects)) for j in range(K)]
    plan = _leave_one_out_plan(data, seed, items, label=lambda ij: f"effect {effect_text(effects[ij[0]])} screen {ij[1]}",
                               tag=lambda ij: f"effect{effect_text(effects[ij[0]])}_{ij[1]}", key="effect",
                               value=lambda ij: effects[ij[0]], leave=screen, differ_in=("masks", "counts"),
                               per_run=MAX_GUIDE_POSITIONS, label_halts=True)
    extra = [{"effect": e["effect"], "screen": None if k == 0 else items[k - 1][1], "seed": seed}
             for k, e in enumerate(plan.dump_extra)]
    return replace(plan, dump_extra=extra)


def _first_crossing(anchors, power, level):
    """Per target, the smallest effect at which ``power`` (A, T) reaches ``level`` along ``anchors`` (A ascending values,
    the first of them 0): the smallest positive anchor where the power at 0 already reaches the level; else, at the first
    anchor k whose power reaches it, the point between anchors k - 1 and k where the straight line between their powers
    meets the level; ``+inf`` where no anchor reaches it."""
    A, T = power.shape
    out = torch.full((T,), float("inf"), dtype=torch.float64)
    if A < 2:
        return out
    open_ = torch.ones(T, dtype=torch.bool)
    at0 = power[0] >= level
    out[at0] = anchors[1]
    open_ &= ~at0
    for k in range(1, A):
        here = open_ & (power[k] >= level)
        w = (level - power[k - 1]) / (power[k] - power[k - 1])
        out[here] = (anchors[k - 1] * (1.0 - w) + anchors[k] * w)[here]
        open_ &= ~here
    return out


def power_summary(full, fits, effects, plant=None, z_hit: float = 1.96, level: float = 0.8) -> Dict[str, object]:
    """Power-study summary (float64).  ``fits[i][j]`` is the refit of draw j with ``effects[i]`` planted, ``m_ij`` /
    ``s_ij`` its ``mu_loc`` / ``mu_scale``; ``effects`` holds the null, effect 0; ``plant``: ``None`` (every target) or T
    booleans, the targets that were planted.

    * ``detected_ij[t]``: ``|m_ij| / s_ij >= z_hit`` and, for ``e_i != 0``, ``sign(m_ij) == sign(e_i)``;
    * ``power`` (D, T): the mean of ``detected`` over j - at effect 0 the false-positive rate; NaN on unplanted targets;
    * ``power_mean`` (D,): the mean over planted targets and j; ``power_median`` (D,): the median over planted targets of
      ``power``;
    * ``mu_power_mean`` / ``mu_power_se`` (D, T): the mean and the unbiased (K - 1) standard deviation of ``m_ij`` over j;
    * ``shrinkage`` (D,): the median over planted targets of ``mu_power_mean[i] / e_i``; NaN at effect 0;
    * ``mde`` (T,): the minimal detectable effect.  Over the anchors - effect 0, then the positive effects in ascending
      order - the first crossing of ``level`` by linear interpolation of ``power`` between neighbouring anchors; the
      smallest positive effect where the power at 0 already reaches the level; ``+inf`` where no anchor reaches it (and
      without a positive effect); NaN on unplanted targets;
    * ``mde_neg`` (T,): likewise over ``|e|`` of the negative effects, a positive number; absent without a negative effect;
    * ``n_planted``, ``n_screens`` = K, ``effects``, ``level``, ``z_hit``.

    Fewer than two screens per effect, rows of different lengths, a row count that is not D, no effect 0, and a ``plant``
    that is not one entry per target are each a ``ValueError``."""
    effects = [float(e) for e in effects]
    D = len(effects)
    if D < 1 or D != len(fits):
        raise ValueError(f"power_summary needs one list of fits per effect, got {len(fits)} for {D} effects")
    K = len(fits[0])
    if K < 2 or any(len(row) != K for row in fits):
        raise ValueError(f"power_summary needs at least two screens at every effect, the same number at each, got "
                         f"{[len(row) for row in fits]}")
    if 0.0 not in effects:
        raise ValueError(f"power_summary needs effect 0, the null every power is read against, among {effects}")
    z_hit, level = float(z_hit), float(level)
    m = torch.stack([torch.stack([_mu_loc(r).reshape(-1) for r in row]) for row in fits])  # (D, K, T)
    s = torch.stack([torch.stack([_param(r, "mu_scale").reshape(-1) for r in row]) for row in fits])
    T = int(m.shape[2])
    if plant is None:
        planted = torch.ones(T, dtype=torch.bool)
    else:
        planted = torch.as_tensor(plant).detach().cpu().reshape(-1) != 0
        if int(planted.numel()) != T:
            raise ValueError(f"plant has {int(planted.numel())} entries for {T} targets")
    e = torch.tensor(effects, dtype=torch.float64)
    nan = float("nan")
    detected = (m.abs() / s) >= z_hit
    directed = e != 0
    detected[directed] &= torch.sign(m[directed]) == torch.sign(e[directed]).reshape(-1, 1, 1)
    power = detected.to(torch.float64).mean(1)
    power[:, ~planted] = nan
    n_planted = int(planted.sum())
    none = torch.full((D,), nan, dtype=torch.float64)
    mean = m.mean(1)
    if n_planted:
        power_mean = power[:, planted].mean(1)
        power_median = torch.stack([torch.quantile(power[i][planted], 0.5) for i in range(D)])
        shrinkage = torch.stack([torch.quantile(mean[i][planted] / e[i], 0.5) if effects[i] != 0
                                 else torch.tensor(nan, dtype=torch.float64) for i in range(D)])
    else:
        power_mean, power_median, shrinkage = none, none.clone(), none.clone()
    out = {"power": power, "power_mean": power_mean, "power_median": power_median, "mu_power_mean": mean,
           "mu_power_se": m.std(1, unbiased=True), "shrinkage": shrinkage, "n_planted": n_planted, "n_screens": K,
           "effects": effects, "level": level, "z_hit": z_hit}
    null = effects.index(0.0)
    for key, sign in (("mde", 1.0), ("mde_neg", -1.0)):
        rows = sorted((sign * f, i) for i, f in enumerate(effects) if sign * f > 0)
        if key == "mde_neg" and not rows:
            continue
        anchors = torch.tensor([0.0] + [a for a, _ in rows], dtype=torch.float64)
        mde = _first_crossing(anchors, power[[null] + [i for _, i in rows]], level)
        mde[~planted] = nan
        out[key] = mde
    return out
