"""``bean run``: screen -> tensors -> (negative-control fit) -> main fit -> tables.

Follows ``bean/cli/run.py:66-311`` step for step (variant and tiling library designs);
every step delegates to the module that mirrors the reference's.  The fit itself
runs on the MI355X through ``run_inference`` (``libbean_hip``).
"""
from __future__ import annotations

import logging
import os
import pickle as pkl
from copy import deepcopy
from functools import partial

import numpy as np

from ..framework import read_h5ad
from ..model import jackknife as jk
from ..model import run as model_run
from ..model.readwrite import write_result_table
from ..model.run import (_check_prior_params, _get_guide_info, _get_guide_target_info, check_args,
                         identify_model_guide, identify_negctrl_model_guide, run_inference)
from ..model.tiling_info import guide_to_variant_df, variant_table
from ..preprocessing.screen_data import DATACLASS_DICT
from ..preprocessing.utils import prepare_bdata

logging.basicConfig(level=logging.INFO, format="%(levelname)-5s @ %(asctime)s:\n\t %(message)s \n",
                    datefmt="%a, %d %b %Y %H:%M:%S")
logger = logging.getLogger("bean_run")
info, warn = logger.info, logger.warning


def _init_distributed():
    """`torchrun --nproc-per-node N bin/bean run ...`: one process per GPU; every rank builds the
    same screen, `run_inference` shards the guides, rank 0 writes the tables.  Returns (rank, world).
    BEAN_DIST_BACKEND=gloo and BEAN_DIST_SINGLE_DEVICE=1 exist for rehearsals on a one-GPU box."""
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1
    if not dist.is_initialized():
        local = 0 if os.environ.get("BEAN_DIST_SINGLE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        backend = os.environ.get("BEAN_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    return dist.get_rank(), dist.get_world_size()


def _replicate_names(ndata):
    """Names of the screen's replicates in the order of the tensors' replicate axis (the samples are sorted by
    replicate, then condition)."""
    samples = ndata.screen.samples
    col = "_rc" if "_rc" in samples.columns else "replicate"
    names = list(dict.fromkeys(samples[col].astype(str))) if col in samples.columns else []
    return names if len(names) == int(ndata.n_reps) else [str(r) for r in range(int(ndata.n_reps))]


_SAME_SEED = "{flag} fits every member with the same seed and does not combine with --n-seeds > 1."
_TWO_RUNS = "{flag} and {other} are two runs: they do not combine in one."
_NEEDS_FITS = "{{flag}} needs the leave-one-{}out fits and does not combine with --load-existing."
_SAMPLE_RULES = (("jackknife_replicates", _TWO_RUNS), ("jackknife_guides", _TWO_RUNS), ("n_seeds", _SAME_SEED),
                 ("load_existing", _NEEDS_FITS.format("")), ("bootstrap", _TWO_RUNS), ("design_depths", _TWO_RUNS),
                 ("power_effects", _TWO_RUNS))
_BOOTSTRAP_FAMILY = ("{{flag}} simulates the counts of the sorting variant models (Normal, MixtureNormal) and is not "
                     "available for {}.")
_SURVIVAL_BOOTSTRAP_FAMILY = ("{{flag}} simulates the counts of the survival variant models (Normal, MixtureNormal) and "
                              "is not available for {}.")
# the flags that ask for a member set, in the order their refusals are reported:
# (attribute, mode, ((what it does not combine with, sentence), ...))
MEMBER_FLAGS = (
    ("jackknife_replicates", "replicates", (("n_seeds", _SAME_SEED),
                                            ("load_existing", _NEEDS_FITS.format("replicate-")),
                                            ("bootstrap", _TWO_RUNS), ("design_depths", _TWO_RUNS),
                                            ("power_effects", _TWO_RUNS))),
    ("jackknife_guides", "guides", (("n_seeds", _SAME_SEED), ("jackknife_replicates", _TWO_RUNS),
                                    ("load_existing", _NEEDS_FITS.format("guide-")),
                                    ("tiling", "{flag} needs targets that own their guides and does not combine with tiling."),
                                    ("bootstrap", _TWO_RUNS), ("design_depths", _TWO_RUNS),
                                    ("power_effects", _TWO_RUNS))),
    ("jackknife_samples", "sample", (("jackknife_conditions", _TWO_RUNS),) + _SAMPLE_RULES),
    ("jackknife_conditions", "condition", (("jackknife_samples", _TWO_RUNS),) + _SAMPLE_RULES),
    ("bootstrap", "bootstrap", (("bootstrap_one", "{flag} needs at least 2 screens."),
                                ("tiling", _BOOTSTRAP_FAMILY.format("tiling screens (MultiMixtureNormal)")),
                                ("survival", _BOOTSTRAP_FAMILY.format("survival screens")),
                                ("n_seeds", _SAME_SEED), ("jackknife_replicates", _TWO_RUNS),
                                ("jackknife_guides", _TWO_RUNS), ("jackknife_samples", _TWO_RUNS),
                                ("jackknife_conditions", _TWO_RUNS),
                                ("load_existing", "{flag} needs the refits of its simulated screens and does not combine "
                                                  "with --load-existing."),
                                ("design_depths", _TWO_RUNS), ("power_effects", _TWO_RUNS))),
    ("design_depths", "design", (("design_one", "{flag} needs at least 2 screens per depth (--design-screens)."),
                                 ("tiling", _BOOTSTRAP_FAMILY.format("tiling screens (MultiMixtureNormal)")),
                                 ("survival", _BOOTSTRAP_FAMILY.format("survival screens")),
                                 ("n_seeds", _SAME_SEED), ("jackknife_replicates", _TWO_RUNS),
                                 ("jackknife_guides", _TWO_RUNS), ("jackknife_samples", _TWO_RUNS),
                                 ("jackknife_conditions", _TWO_RUNS),
                                 ("load_existing", "{flag} needs the refits of its simulated screens and does not combine "
                                                   "with --load-existing."),
                                 ("bootstrap", _TWO_RUNS), ("power_effects", _TWO_RUNS))),
    ("power_effects", "power", (("power_one", "{flag} needs at least 2 screens per effect (--power-screens)."),
                                ("tiling", _BOOTSTRAP_FAMILY.format("tiling screens (MultiMixtureNormal)")),
                                ("survival", _BOOTSTRAP_FAMILY.format("survival screens")),
                                ("n_seeds", _SAME_SEED), ("jackknife_replicates", _TWO_RUNS),
                                ("jackknife_guides", _TWO_RUNS), ("jackknife_samples", _TWO_RUNS),
                                ("jackknife_conditions", _TWO_RUNS),
                                ("load_existing", "{flag} needs the refits of its simulated screens and does not combine "
                                                  "with --load-existing."),
                                ("bootstrap", _TWO_RUNS), ("design_depths", _TWO_RUNS))),
    ("survival_bootstrap", "survival_bootstrap",
     (("survival_bootstrap_one", "{flag} needs at least 2 screens."),
      ("tiling", _SURVIVAL_BOOTSTRAP_FAMILY.format("tiling screens (MultiMixtureNormal)")),
      ("sorting", _SURVIVAL_BOOTSTRAP_FAMILY.format("sorting screens (--bootstrap serves them)")),
      ("n_seeds", _SAME_SEED), ("jackknife_replicates", _TWO_RUNS), ("jackknife_guides", _TWO_RUNS),
      ("jackknife_samples", _TWO_RUNS), ("jackknife_conditions", _TWO_RUNS),
      ("load_existing", "{flag} needs the refits of its simulated screens and does not combine with --load-existing."),
      ("bootstrap", _TWO_RUNS), ("design_depths", _TWO_RUNS), ("power_effects", _TWO_RUNS))),
)
_IS_SET = {"n_seeds": lambda args: int(getattr(args, "n_seeds", 1) or 1) > 1,
           "bootstrap": lambda args: int(getattr(args, "bootstrap", 0) or 0) > 0,
           "bootstrap_one": lambda args: int(getattr(args, "bootstrap", 0) or 0) == 1,
           "design_one": lambda args: int(getattr(args, "design_screens", 8) or 0) < 2,
           "power_one": lambda args: int(getattr(args, "power_screens", 8) or 0) < 2,
           "survival_bootstrap": lambda args: int(getattr(args, "survival_bootstrap", 0) or 0) > 0,
           "survival_bootstrap_one": lambda args: int(getattr(args, "survival_bootstrap", 0) or 0) == 1,
           "sorting": lambda args: getattr(args, "selection", None) == "sorting",
           "survival": lambda args: getattr(args, "selection", None) == "survival",
           "tiling": lambda args: getattr(args, "library_design", None) == "tiling",
           "guides_max": lambda args: int(getattr(args, "jackknife_guides_max", 63)) > 63}


def _refuse(message):
    raise ValueError(message)


def member_mode(args, fail=_refuse, only=None, parser_rules=None):
    """The member set this run fits next to the screen: None, "seeds", "replicates", "guides", "sample", "condition",
    "bootstrap", "design" or "power".
    A combination that is refused goes to ``fail(sentence)`` (the parser's ``error``; here, raising ``ValueError``).
    ``only``: the flags whose rules are looked at (default: all); ``parser_rules``: further rules per flag, after its own."""
    is_set = lambda attr: _IS_SET.get(attr, lambda a: bool(getattr(a, attr, False)))(args)  # noqa: E731
    flag = lambda attr: "--" + attr.replace("_", "-")  # noqa: E731
    mode = "seeds" if is_set("n_seeds") else None
    for attr, flag_mode, rules in MEMBER_FLAGS:
        if not is_set(attr) or (only is not None and attr not in only):
            continue
        for other, sentence in rules + (parser_rules or {}).get(attr, ()):
            if is_set(other):
                fail(sentence.format(flag=flag(attr), other=flag(other)))
        mode = flag_mode
    return mode


_PARTICLES_ONE_FIT = ("--num-particles averages draws inside one fit and does not combine with {other}: particles inside "
                      "member sets are not batched.")
_PARTICLES_NEED_FIT = "--num-particles needs the fit itself and does not combine with --load-existing."
_PARTICLES_MAX = "--num-particles is at most {most}."


def particle_count(args, fail=_refuse) -> int:
    """``--num-particles``: the draws per step of the main model's fit.  More than one is refused - ``fail(sentence)``,
    as ``member_mode`` - next to a member set (``--n-seeds`` > 1, any ``--jackknife-*``), with ``--load-existing`` and
    above ``MAX_MEMBERS``."""
    from .._lib import MAX_MEMBERS

    n = int(getattr(args, "num_particles", 1) or 1)
    if n < 1:
        fail(f"--num-particles must be >= 1, got {n}.")
    if n == 1:
        return 1
    is_set = lambda attr: _IS_SET.get(attr, lambda a: bool(getattr(a, attr, False)))(args)  # noqa: E731
    for attr in ("n_seeds",) + tuple(attr for attr, _, _ in MEMBER_FLAGS):
        if is_set(attr):
            fail(_PARTICLES_ONE_FIT.format(other="--" + attr.replace("_", "-")))
    if is_set("load_existing"):
        fail(_PARTICLES_NEED_FIT)
    if n > MAX_MEMBERS:
        fail(_PARTICLES_MAX.format(most=MAX_MEMBERS))
    return n


_PREDICTIVE_FAMILY = ("--posterior-predictive simulates the counts of the sorting variant models (Normal, MixtureNormal) and "
                      "is not available for {what}.")


def predictive_draws(args, fail=_refuse) -> int:
    """``--posterior-predictive S``: the number of replicate screens to draw after the fit (0: none).  A family the count
    simulator does not take is refused - ``fail(sentence)``, as ``member_mode`` - with the family named."""
    n = int(getattr(args, "posterior_predictive", 0) or 0)
    if n < 0:
        fail(f"--posterior-predictive must be >= 0, got {n}.")
    if n == 0:
        return 0
    if getattr(args, "library_design", None) == "tiling":
        fail(_PREDICTIVE_FAMILY.format(what="tiling screens (MultiMixtureNormal)"))
    if getattr(args, "selection", None) == "survival":
        fail(_PREDICTIVE_FAMILY.format(what="survival screens"))
    return n


_SURVIVAL_PREDICTIVE_FAMILY = ("--survival-predictive simulates the counts of the survival variant models (Normal, "
                               "MixtureNormal) and is not available for {what}.")


def survival_predictive_draws(args, fail=_refuse) -> int:
    """``--survival-predictive S``: the number of replicate screens of a survival fit to draw after it (0: none).  A
    family the survival count simulator does not take is refused - ``fail(sentence)``, as ``member_mode`` - with the
    family named."""
    n = int(getattr(args, "survival_predictive", 0) or 0)
    if n < 0:
        fail(f"--survival-predictive must be >= 0, got {n}.")
    if n == 0:
        return 0
    if getattr(args, "library_design", None) == "tiling":
        fail(_SURVIVAL_PREDICTIVE_FAMILY.format(what="tiling screens (MultiMixtureNormal)"))
    if getattr(args, "selection", None) != "survival":
        fail(_SURVIVAL_PREDICTIVE_FAMILY.format(what="sorting screens (--posterior-predictive serves them)"))
    return n


_IMPORTANCE_FAMILY = ("--importance-check weights draws of the sorting variant models (Normal, MixtureNormal) per target and "
                      "is not available for {what}.")
IMPORTANCE_MIN_DRAWS = 25  # model/importance.py::MIN_DRAWS: fewer draws have no tail to fit


def importance_draws(args, fail=_refuse) -> int:
    """``--importance-check S``: the number of draws from the fitted guide to weight after the fit (0: none).  Fewer than
    25 and a family the per-target weights do not take are refused - ``fail(sentence)``, as ``member_mode`` - with the
    family named."""
    n = int(getattr(args, "importance_check", 0) or 0)
    if n < 0:
        fail(f"--importance-check must be >= 0, got {n}.")
    if n == 0:
        return 0
    if n < IMPORTANCE_MIN_DRAWS:
        fail(f"--importance-check needs at least {IMPORTANCE_MIN_DRAWS} draws to fit the tail of the weights, got {n}.")
    if getattr(args, "library_design", None) == "tiling":
        fail(_IMPORTANCE_FAMILY.format(what="tiling screens (MultiMixtureNormal)"))
    if getattr(args, "selection", None) == "survival":
        fail(_IMPORTANCE_FAMILY.format(what="survival screens"))
    return n


IMPORTANCE_NODES = (16, 32, 64)  # _lib.MARGINAL_NODES


def importance_nodes(args, fail=_refuse):
    """``--importance-integrate-pi [--importance-nodes Q]``: the quadrature nodes of the marginal check (``pi`` integrated
    out of the model), or None without the flag.  It rides on ``--importance-check`` - refused without it, and for every
    family that flag is refused for (``importance_draws`` names it)."""
    nodes = int(getattr(args, "importance_nodes", 32) or 32)
    if nodes not in IMPORTANCE_NODES:
        fail(f"--importance-nodes must be one of 16, 32, 64, got {nodes}.")
    if not getattr(args, "importance_integrate_pi", False):
        return None
    if not int(getattr(args, "importance_check", 0) or 0):
        fail("--importance-integrate-pi integrates pi out of the weights of --importance-check S and needs that flag.")
    return nodes


def importance_tail_rule(args, fail=_refuse) -> bool:
    """``--importance-tail-rule``: the Gauss-Jacobi rule for the pairs the marginal check's quadrature does not resolve.
    Refused without ``--importance-integrate-pi``; every other refusal is that flag's own (``importance_nodes``)."""
    if not getattr(args, "importance_tail_rule", False):
        return False
    if not getattr(args, "importance_integrate_pi", False):
        fail("--importance-tail-rule sets the rule --importance-integrate-pi uses for the pairs it does not resolve and "
             "needs that flag.")
    return True


_GRID_FAMILY = ("--grid-posterior evaluates the posterior of (mu, sd) per target of the sorting variant models (Normal, "
                "MixtureNormal) and is not available for {what}.")
_GRID_ACC = ("--grid-posterior is not available with --scale-by-acc: the guide noise is a further latent per guide, so the "
             "posterior of a target is not a function of (mu, sd) alone.")


def grid_nodes(args, fail=_refuse):
    """``--grid-posterior [--grid-nodes Q]``: the quadrature nodes of the grid posterior, or None without the flag.
    Refused - ``fail(sentence)``, as ``member_mode`` - for every family ``--importance-check`` is refused for, with the
    family named, and with ``--scale-by-acc``."""
    nodes = int(getattr(args, "grid_nodes", 32) or 32)
    if nodes not in IMPORTANCE_NODES:
        fail(f"--grid-nodes must be one of 16, 32, 64, got {nodes}.")
    if not getattr(args, "grid_posterior", False):
        return None
    if getattr(args, "library_design", None) == "tiling":
        fail(_GRID_FAMILY.format(what="tiling screens (MultiMixtureNormal)"))
    if getattr(args, "selection", None) == "survival":
        fail(_GRID_FAMILY.format(what="survival screens"))
    if getattr(args, "scale_by_acc", False):
        fail(_GRID_ACC)
    return nodes


def grid_tail_rule(args, fail=_refuse) -> bool:
    """``--grid-tail-rule``: the Gauss-Jacobi rule for the pairs the grid posterior's quadrature does not resolve.
    Refused without ``--grid-posterior``; every other refusal is that flag's own (``grid_nodes``)."""
    if not getattr(args, "grid_tail_rule", False):
        return False
    if not getattr(args, "grid_posterior", False):
        fail("--grid-tail-rule sets the rule --grid-posterior uses for the pairs it does not resolve and needs that flag.")
    return True


def check_guide_jackknife_switches(args) -> bool:
    """Whether --jackknife-guides is set; the combinations it is refused with raise (the parser refuses them first)."""
    return member_mode(args, only=("jackknife_guides",)) == "guides"


def check_sample_jackknife_switches(args):
    """``"sample"`` / ``"condition"`` if --jackknife-samples / --jackknife-conditions is set, else None; the
    combinations they are refused with raise (the parser refuses them first)."""
    mode = member_mode(args, only=("jackknife_samples", "jackknife_conditions"))
    return mode if mode in ("sample", "condition") else None


def _sample_group_names(ndata, groups, fallback, by, condition_column):
    """Names of a sample jackknife's groups: the sample table row the tensor builder put at (r, b) - the samples are
    sorted by replicate, then condition - or the condition's label; ``fallback`` (``r{r}_c{b}`` / ``c{b}``) where the
    screen's sample table does not have that layout."""
    samples = getattr(getattr(ndata, "screen", None), "samples", None)
    R, B = int(ndata.n_reps), int(ndata.n_condits)
    if samples is None or len(samples) != R * B:
        return list(fallback)
    if by == "sample":
        names = [str(samples.index[g[0][0] * B + g[0][1]]) for g in groups]
    elif condition_column in samples.columns:
        names = [str(samples[condition_column].iloc[g[0][1]]) for g in groups]
    else:
        return list(fallback)
    return names if len(set(names)) == len(names) else list(fallback)


def _entries(heads, fits):
    return [{**head, "params": out["params"], "loss": out["loss"]} for head, (_, out) in zip(heads, fits)]


def _seed_members(fit, ndata, args, guide_names, n_rows):
    from ..model.ensemble import combine_ensemble

    members = fit(model_run.run_inference_ensemble, seeds=[model_run.SEED + k for k in range(int(args.n_seeds))])
    store, spread = combine_ensemble(members)  # the tables come from the combination
    combined = (store, {"params": {k: v.detach().cpu() for k, v in store.items()}, "loss": members[0][1]["loss"]})
    return combined, _entries([{}] * len(members), members), {"seed_sd": spread["mu_seed_sd"], "n_seeds": len(members)}


def _replicate_members(fit, ndata, args, guide_names, n_rows):
    full, loo, left_out = fit(model_run.run_inference_jackknife)
    names = _replicate_names(ndata)
    return (full, _entries([{"left_out": names[r]} for r in left_out], loo),
            {"jackknife": jk.jackknife_summary(full, loo, left_out, names)})


def _guide_members(fit, ndata, args, guide_names, n_rows):
    full, loo, positions, included = fit(model_run.run_inference_guide_jackknife,
                                         max_positions=int(getattr(args, "jackknife_guides_max", 63)))
    return (full, {"included": included, "positions": _entries([{"position": j} for j in positions], loo)},
            {"guide_jackknife": jk.guide_jackknife_summary(full, loo, positions, included, ndata, guide_names)})


def _sample_members(fit, ndata, args, guide_names, n_rows):
    by = member_mode(args)
    full, loo, groups, fallback = fit(model_run.run_inference_sample_jackknife, by=by)
    names = _sample_group_names(ndata, groups, fallback, by, args.condition_col)
    return (full, _entries([{"left_out": name, "pairs": [list(p) for p in g]} for name, g in zip(names, groups)], loo),
            {"sample_jackknife": jk.sample_jackknife_summary(full, loo, groups, names)})


def _bootstrap_members(fit, ndata, args, guide_names, n_rows):
    full, boots = fit(model_run.run_inference_bootstrap, n_boot=int(args.bootstrap),
                      boot_seed=int(getattr(args, "bootstrap_seed", model_run.SEED)))
    return (full, _entries([{"screen": j} for j in range(len(boots))], boots),
            {"bootstrap": jk.bootstrap_summary(full, boots)})


def _survival_bootstrap_members(fit, ndata, args, guide_names, n_rows):
    full, boots = fit(model_run.run_survival_bootstrap, n_boot=int(args.survival_bootstrap),
                      boot_seed=int(getattr(args, "bootstrap_seed", model_run.SEED)))
    return (full, _entries([{"screen": j} for j in range(len(boots))], boots),
            {"bootstrap": _rows_of(jk.bootstrap_summary(full, boots), n_rows)})


def _rows_of(summary, n_rows):
    """A per-target summary for a target table of ``n_rows`` rows.  The table of a screen that lists a target under two
    groups has more rows than the fit has targets; ``write_result_table`` leaves the fitted columns (``mu`` ...) of the
    surplus rows empty, and so are the summary's per-target entries.  ``n_boot`` is the run's number of screens, one
    number for the whole table."""
    out = dict(summary)
    for k, v in summary.items():
        if k != "n_boot":
            v = np.asarray(v.detach().cpu() if hasattr(v, "detach") else v, dtype=np.float64).reshape(-1)
            out[k] = np.concatenate([v, np.full(max(n_rows - len(v), 0), np.nan)])
    return out


def _design_members(fit, ndata, args, guide_names, n_rows):
    depths = model_run.design_depths(args.design_depths)
    full, fits = fit(model_run.run_inference_design, depths=depths, n_screens=int(getattr(args, "design_screens", 8)),
                     design_seed=int(getattr(args, "design_seed", model_run.SEED)))
    heads = [{"depth": f, "screen": j} for f in depths for j in range(len(fits[0]))]
    return (full, _entries(heads, [r for row in fits for r in row]),
            {"design": jk.design_summary(full, fits, depths, data=ndata)})


def _power_members(fit, ndata, args, guide_names, n_rows):
    effects = model_run.power_effects(args.power_effects)
    full, fits = fit(model_run.run_inference_power, effects=effects, n_screens=int(getattr(args, "power_screens", 8)),
                     power_seed=int(getattr(args, "power_seed", model_run.SEED)))
    heads = [{"effect": e, "screen": j} for e in effects for j in range(len(fits[0]))]
    return (full, _entries(heads, [r for row in fits for r in row]),
            {"power": jk.power_summary(full, fits, effects, level=float(getattr(args, "power_level", 0.8)))})


# mode -> (what fits its members and returns (the fit the tables come from, the members' entry of the --save-raw
#          pickle, write_result_table's keywords for their summary), the key of that entry)
MEMBER_RUNS = {"seeds": (_seed_members, "ensemble"), "replicates": (_replicate_members, "jackknife"),
               "guides": (_guide_members, "guide_jackknife"), "sample": (_sample_members, "sample_jackknife"),
               "condition": (_sample_members, "sample_jackknife"), "bootstrap": (_bootstrap_members, "bootstrap"),
               "design": (_design_members, "design"), "power": (_power_members, "power"),
               "survival_bootstrap": (_survival_bootstrap_members, "bootstrap")}


def main(args, return_data=False):
    rank, world = (0, 1) if return_data else _init_distributed()
    if rank != 0:  # one banner / one log / one set of tables
        logger.setLevel(logging.ERROR)
    print(r"""
    _ _
  /  \ '\                       
  |   \  \      _ _ _  _ _ ___  
   \   \  |    | '_| || | ' \   
    `.__|/     |_|  \_,_|_||_|  [crispr-bean_amd / MI355X]
    """)
    print("bean-run: Run model to identify targeted variants and their impact.")
    bdata = read_h5ad(args.bdata_path)
    args, bdata = check_args(args, bdata)
    prefix = args.outdir + "/bean_run_result." + os.path.basename(args.bdata_path).rsplit(".h5ad", 1)[0]
    os.makedirs(prefix, exist_ok=True)
    if rank == 0:  # rank 0 owns the log file and every table; the other ranks only fit their shards
        handler = logging.FileHandler(f"{prefix}/bean_run.log")
        handler.setLevel(logging.INFO)
        logger.addHandler(handler)
    model_label, model, guide = identify_model_guide(args)
    info("Done loading data. Preprocessing...")
    bdata = prepare_bdata(bdata, args, warn, prefix, write_files=(rank == 0))
    is_neg = lambda scr: np.where(scr.guides[args.negctrl_col].map(lambda v: str(v).lower())  # noqa: E731
                                  == args.negctrl_col_value.lower())[0]
    negctrl_idx = is_neg(bdata) if args.negctrl_col in bdata.guides.columns else np.zeros(0, dtype=int)
    ndata = DATACLASS_DICT[args.selection][model_label](
        bdata,
        repguide_mask=args.repguide_mask,
        sample_mask_column=args.sample_mask_col,
        accessibility_col=args.acc_col,
        accessibility_bw_path=args.acc_bw_path,
        condition_column=args.condition_col,
        time_column=args.time_col,
        control_condition=args.control_condition,
        lower_quantile_column=args.sorting_bin_lower_quantile_col,
        upper_quantile_column=args.sorting_bin_upper_quantile_col,
        target_col=args.target_col,
        shrink_alpha=args.shrink_alpha,
        popt=args.popt,
        use_bcmatch=(not args.ignore_bcmatch),
        negctrl_guide_idx=negctrl_idx,
        allele_df_key=args.allele_df_key,
        control_guide_tag=args.control_guide_tag,
    )
    if args.save_raw and rank == 0:
        pkl.dump(bdata, open(f"{prefix}/ndata.pkl", "wb"))
    if return_data:
        return ndata
    adj_negctrl_idx = None
    control = args.control_condition.split(",")[0]
    if args.library_design == "variant":
        if not args.uniform_edit and "edit_rate" not in ndata.screen.guides.columns:
            ndata.screen.get_guide_edit_rate(unsorted_condition_label=control, condition_col=args.condition_col)
        target_info_df = _get_guide_target_info(ndata.screen, args, cols_include=[args.negctrl_col])
        if args.adjust_confidence_by_negative_control:
            adj_negctrl_idx = np.where(target_info_df[args.negctrl_col].map(lambda v: str(v).lower())
                                       == args.negctrl_col_value.lower())[0]
    else:
        # tiling: one row per edit (bean/cli/run.py:155-206)
        if "edit_rate_norm" not in ndata.screen.guides.columns and "edits" in ndata.screen.layers:
            ndata.screen.get_guide_edit_rate(unsorted_condition_label=control, condition_col=args.condition_col)
        splice = None
        if getattr(args, "splice_site_path", None) is not None:
            import pandas as pd
            splice = pd.read_csv(args.splice_site_path).pos
        target_info_df = variant_table(ndata, ndata.screen.guides.index.values,
                                       bdata.guides["target_group"].values, control_tag=args.control_guide_tag,
                                       splice_sites=splice)
        if args.adjust_confidence_by_negative_control:
            adj_negctrl_idx = np.where((target_info_df.ref == target_info_df.alt)
                                       & (target_info_df.coding == "coding"))[0]
            info(f"Using {len(adj_negctrl_idx)} synonymous variants to adjust confidence.")
    guide_info_df = _get_guide_info(ndata.screen, args, guide_lfc_pseudocount=args.guide_lfc_pseudocount)
    if args.library_design == "tiling":
        import pandas as pd
        guide_info_df = pd.concat([guide_info_df, guide_to_variant_df(target_info_df).reindex(guide_info_df.index)],
                                  axis=1)
    if args.prior_params is not None:
        model = partial(model, prior_params=_check_prior_params(args.prior_params, ndata))

    info(f"Running inference for {model_label}...")
    mode = member_mode(args)
    n_particles = particle_count(args)
    n_predictive = predictive_draws(args)
    if n_predictive:
        # refused before the fit, not after it: what only the screen shows (sample covariates, several ranks)
        from ..engine import PredictiveUnsupported

        why = model_run._predictive_refusal(model_run._resolve(model), ndata, world)
        if why is not None:
            raise PredictiveUnsupported(_PREDICTIVE_FAMILY.format(what=why))
    n_survival_predictive = survival_predictive_draws(args)
    if n_survival_predictive:
        from ..engine import PredictiveUnsupported

        why = model_run._survival_predictive_refusal(model_run._resolve(model), ndata, world)
        if why is not None:
            raise PredictiveUnsupported(_SURVIVAL_PREDICTIVE_FAMILY.format(what=why))
    n_importance = importance_draws(args)
    n_nodes = importance_nodes(args)
    is_tail = importance_tail_rule(args)
    if n_importance:
        from ..engine import PredictiveUnsupported

        why = model_run._predictive_refusal(model_run._resolve(model), ndata, world)
        if why is not None:
            raise PredictiveUnsupported(_IMPORTANCE_FAMILY.format(what=why))
    n_grid = grid_nodes(args)
    if n_grid:
        from ..engine import PredictiveUnsupported

        why = model_run._predictive_refusal(model_run._resolve(model), ndata, world)
        if why is not None:
            raise PredictiveUnsupported(_GRID_FAMILY.format(what=why))
    table_columns = {}
    save_dict = dict()
    param_history_dict_negctrl = None
    if args.load_existing:
        # re-write the tables from a `--save-raw` pickle instead of fitting.  (The reference's branch,
        # bean/cli/run.py:229-231, indexes the loaded dict as if it were the parameter store and
        # fails; here the stored parameters are used.)
        from ..model.run import ParamStore

        with open(f"{prefix}/{model_label}.result{args.result_suffix}.pkl", "rb") as handle:
            loaded = pkl.load(handle)
        param_history_dict = ParamStore(loaded["params"])
        if "negctrl" in loaded:
            param_history_dict_negctrl = ParamStore(loaded["negctrl"]["params"])
        save_dict = loaded
    elif args.fit_negctrl:
        negctrl_model, negctrl_guide = identify_negctrl_model_guide(args, "X_bcmatch" in bdata.layers)
        idx = is_neg(ndata.screen)
        info(f"Using {len(idx)} negative control elements to adjust phenotypic effect sizes...")
        ndata_negctrl = ndata[idx]
        param_history_dict_negctrl, save_dict["negctrl"] = deepcopy(
            run_inference(negctrl_model, negctrl_guide, ndata_negctrl, num_steps=args.n_iter))
        if args.selection == "survival":
            model = partial(model, mu_negctrl=(param_history_dict_negctrl["mu_loc"].detach().mean(),
                                               param_history_dict_negctrl["mu_scale"].detach().mean()))
    if not args.load_existing:
        save_dict["data"] = ndata
        if mode is not None:
            # a member set: member 0 is the fit a run without the flag does, the set's summary adds columns to its tables
            fit_members, key = MEMBER_RUNS[mode]
            fit = lambda fit_of, **own: fit_of(model, guide, ndata, num_steps=args.n_iter, **own)  # noqa: E731
            shown, saved, table_columns = fit_members(fit, ndata, args, list(guide_info_df.index), len(target_info_df))
            param_history_dict, save_dict_model = deepcopy(shown)
            save_dict.update(save_dict_model)
            save_dict[key] = saved
        else:
            particles = dict(num_particles=n_particles) if n_particles > 1 else {}
            param_history_dict, save_dict_model = deepcopy(
                run_inference(model, guide, ndata, num_steps=args.n_iter, **particles))
            save_dict.update(save_dict_model)
    if rank != 0:
        return prefix
    outfile = f"{prefix}/bean_element[sgRNA]_result.{model_label}{args.result_suffix}.csv"
    info(f"Done running inference. Writing result at {outfile}...")
    if args.save_raw:
        with open(f"{prefix}/{model_label}.result{args.result_suffix}.pkl", "wb") as handle:
            pkl.dump(save_dict, handle)
    if n_importance:
        info(f"Importance-sampling check: {n_importance} draws from the fitted guide, weighted per target...")
        summary = model_run.run_importance_check(model, guide, ndata, param_history_dict, n_draws=n_importance,
                                                 seed=int(getattr(args, "importance_seed", model_run.SEED)),
                                                 **({"integrate_pi": n_nodes} if n_nodes else {}),
                                                 **({"tail_rule": True} if is_tail else {}))
        table_columns = {**table_columns, "importance": {k: v.detach().cpu() for k, v in summary.items()}}
        k = table_columns["importance"]["psis_k"]
        info(f"Importance-sampling check: psis_k > 0.7 on {int((k > 0.7).sum())} of {k.numel()} targets "
             f"({100.0 * float((k > 0.7).double().mean()) if k.numel() else 0.0:.1f} %); median psis_k "
             f"{float(k.median()) if k.numel() else float('nan'):.3f}.")
        if n_nodes:
            km = table_columns["importance"]["psis_k_marg"]
            left_out = table_columns["importance"]["n_pairs_unresolved"] > 0
            share = lambda m: 100.0 * float(m.double().mean()) if m.numel() else 0.0  # noqa: E731
            info(f"Importance-sampling check, pi integrated out ({n_nodes} nodes): psis_k_marg > 0.7 on "
                 f"{int((km > 0.7).sum())} of {km.numel()} targets ({share(km > 0.7):.1f} %); {int(left_out.sum())} of "
                 f"{km.numel()} targets ({share(left_out):.1f} %) left out as unresolved.")
        if is_tail:
            imp = table_columns["importance"]
            had = imp["n_pairs_tail"] > 0
            got = had & ~imp["psis_k_marg"].isnan()
            barred = had & ~(imp["is_tail_err"] <= 1e-3 * imp["n_pairs_tail"])
            pct = lambda m, of: 100.0 * float(m.sum()) / max(int(of), 1)  # noqa: E731
            info(f"Importance-sampling check, tail rule: {int(had.sum())} of {had.numel()} targets "
                 f"({pct(had, had.numel()):.1f} %) had tail pairs; {int(got.sum())} of those ({pct(got, had.sum()):.1f} %) "
                 f"now have numbers; {int(barred.sum())} of {had.numel()} targets ({pct(barred, had.numel()):.1f} %) refused "
                 "by the tail bar (is_tail_err > 1e-3 n_pairs_tail).")
    if n_grid:
        import torch

        info(f"Grid posterior: the log joint of (mu, sd) per target on its own grid, pi integrated out ({n_grid} nodes)...")
        tail = grid_tail_rule(args)
        summary = model_run.run_grid_posterior(model, guide, ndata, param_history_dict, nodes=n_grid,
                                               **({"tail_rule": True} if tail else {}))
        grid = {k: v.detach().cpu() for k, v in summary.items()}
        table_columns = {**table_columns, "grid": grid}
        out_of = ~grid["grid_ok"] | (grid["n_pairs_unresolved"] > 0)
        if tail:
            had = grid["n_pairs_tail"] > 0
            out_of = ~grid["grid_ok"]
            pct = lambda m, of: 100.0 * float(m.sum()) / max(int(of), 1)  # noqa: E731
            got, barred = had & grid["grid_ok"], had & ~grid["grid_tail_ok"]
            info(f"Grid posterior, tail rule: {int(had.sum())} of {had.numel()} targets ({pct(had, had.numel()):.1f} %) had "
                 f"tail pairs; {int(got.sum())} of those ({pct(got, had.sum()):.1f} %) now have numbers; {int(barred.sum())} "
                 f"of {had.numel()} targets ({pct(barred, had.numel()):.1f} %) refused by the tail bar "
                 "(grid_tail_err > 1e-3 n_pairs_tail).")
        fitted_sd = torch.as_tensor(param_history_dict["mu_scale"]).detach().cpu().double().reshape(-1)
        ratio = (fitted_sd / grid["mu_sd_grid"])[~out_of]
        info(f"Grid posterior: {int(out_of.sum())} of {out_of.numel()} targets "
             f"({100.0 * float(out_of.double().mean()) if out_of.numel() else 0.0:.1f} %) not grid_ok or unresolved; median "
             f"mu_sd / mu_sd_grid over the others {float(ratio.median()) if ratio.numel() else float('nan'):.3f}.")
    write_result_table(
        target_info_df,
        guide_info_df,
        param_history_dict,
        negctrl_params=param_history_dict_negctrl,
        model_label=model_label,
        prefix=f"{prefix}/",
        suffix=args.result_suffix,
        guide_acc=(ndata.guide_accessibility.cpu().numpy() if ndata.guide_accessibility is not None else None),
        adjust_confidence_by_negative_control=args.adjust_confidence_by_negative_control,
        adjust_confidence_negatives=adj_negctrl_idx,
        sd_is_fitted=(args.selection == "sorting"),
        sample_covariates=getattr(ndata, "sample_covariates", None),
        is_survival_screen=(args.selection == "survival"),
        **table_columns,
    )
    if n_predictive:
        from ..model.predictive import write_predictive_tables

        info(f"Posterior predictive check: {n_predictive} replicate screens...")
        summary = model_run.run_posterior_predictive(model, guide, ndata, param_history_dict, n_draws=n_predictive,
                                                     seed=int(getattr(args, "predictive_seed", model_run.SEED)))
        paths = write_predictive_tables(summary, guide_info_df, ndata, f"{prefix}/", model_label, args.result_suffix)
        info(f"Wrote {paths[0]} and {paths[1]}.")
    if n_survival_predictive:
        from ..model.predictive import write_predictive_tables

        info(f"Survival predictive check: {n_survival_predictive} replicate screens...")
        summary = model_run.run_survival_predictive(model, guide, ndata, param_history_dict,
                                                    n_draws=n_survival_predictive,
                                                    seed=int(getattr(args, "predictive_seed", model_run.SEED)))
        paths = write_predictive_tables(summary, guide_info_df, ndata, f"{prefix}/", model_label, args.result_suffix)
        info(f"Wrote {paths[0]} and {paths[1]}.")
    info("Done!")
    return prefix
