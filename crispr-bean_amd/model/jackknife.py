"""Replicate jackknife: which replicate carries a hit (``run_inference_jackknife``, ``bean run --jackknife-replicates``).

Next to the fit of the whole screen, one fit per replicate with that replicate left out - all with the SAME seed, so that
with common random numbers the differences between the fits come from the data and not from the random stream.

Masked, not removed.  ``leave_out`` is what the reference does with a replicate masked through its own options
(``--sample-mask-col``, ``--repguide-mask``): the replicate stays in every tensor, its rows of the two masks are zero.
Its counts then enter no likelihood term - no gradient, and the reported loss only loses their data-only constant - but
the guide side is unmasked: a masked (replicate, guide) pair still draws its ``pi`` and contributes the variational entropy
of ``q(pi)``.  A fit of the screen with the replicate absent would have no such site; the two are different models, and
this one is the reference's.  Size factors, ``a0`` and the other derived tensors are those of the whole screen.

Pure torch: no GPU involved in this file.
"""
from __future__ import annotations

import copy
from typing import Dict, List, Sequence

import torch


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
    """``(repguide (K, R, G) bool, sample_mask (K, R, B))`` of the K = 1 + len(left_out) fits: member 0 has the
    screen's own masks, member 1 + j those of ``leave_out(data, left_out[j])``."""
    screens = [data] + [leave_out(data, r) for r in left_out]
    return (torch.stack([s.repguide_mask != 0 for s in screens]), torch.stack([s.sample_mask for s in screens]))


def _mu_loc(result) -> torch.Tensor:
    store = result[0] if isinstance(result, (tuple, list)) else result
    return store["mu_loc"].detach().cpu().to(torch.float64)


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
