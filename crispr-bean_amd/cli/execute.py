"""``bean`` command dispatcher (``bean/cli/execute.py:30-84``): the ``run`` sub-command, its companion
``build-prior`` and the mask-producing part of ``qc`` are in scope of this implementation."""
from __future__ import annotations

import argparse
import sys

from ..model.parser import parse_args as attach_run_args


def _positive_int(text: str) -> int:
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError(f"must be >= 1, got {value}")
    return value


def _non_negative_int(text: str) -> int:
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError(f"must be >= 0, got {value}")
    return value


def parse_depths(text):
    """``--design-depths``: a comma-separated list of positive floats, in the order given (``argparse`` type: a bad
    entry, a factor that is not > 0 and a factor given twice are refused with their sentence)."""
    import math

    entries = [e.strip() for e in str(text).split(",")]
    out = []
    for entry in entries:
        try:
            f = float(entry)
        except (TypeError, ValueError):
            raise argparse.ArgumentTypeError(f"{entry!r} is not a number: a comma-separated list of depth factors such as "
                                             "0.25,0.5,2,4 is expected") from None
        if not (math.isfinite(f) and f > 0):
            raise argparse.ArgumentTypeError(f"a depth factor must be a finite number > 0, got {entry}")
        if f in out:
            raise argparse.ArgumentTypeError(f"depth factor {f:g} is given more than once")
        out.append(f)
    return out


def parse_effects(text):
    """``--power-effects``: a comma-separated list of finite floats, negatives allowed, in the order given (``argparse``
    type: a bad entry, an effect that is not finite and an effect given twice are refused with their sentence)."""
    import math

    entries = [e.strip() for e in str(text).split(",")]
    out = []
    for entry in entries:
        try:
            f = float(entry)
        except (TypeError, ValueError):
            raise argparse.ArgumentTypeError(f"{entry!r} is not a number: a comma-separated list of effects such as "
                                             "0.1,0.2,0.4 is expected") from None
        if not math.isfinite(f):
            raise argparse.ArgumentTypeError(f"a planted effect must be a finite number, got {entry}")
        if f in out:
            raise argparse.ArgumentTypeError(f"effect {f:g} is given more than once")
        out.append(f)
    return out


def _open_unit_interval(text: str) -> float:
    value = float(text)
    if not 0.0 < value < 1.0:
        raise argparse.ArgumentTypeError(f"must be in (0, 1), got {text}")
    return value


def get_parser():
    parser = argparse.ArgumentParser(prog="bean")
    sub = parser.add_subparsers(dest="subcommand", help="bean subcommands")
    run = sub.add_parser("run", help="Quantify variant effect sizes from screen data (MI355X)")
    attach_run_args(run)
    # this project's own switches (the reference's flag table, model/parser.py, stays the reference's)
    own = run.add_argument_group("crispr-bean_amd")
    own.add_argument("--n-seeds", dest="n_seeds", type=_positive_int, default=1,
                     help="Fit this many seeds (101, 102, ...) of the main model at once and report their moment-matched "
                          "average, with the between-seed spread of mu in the columns mu_seed_sd / n_seeds (default 1: one fit).")
    own.add_argument("--jackknife-replicates", dest="jackknife_replicates", action="store_true",
                     help="Next to the fit of the screen, fit it once per replicate with that replicate masked (same seed) "
                          "and report, per target, the jackknife standard error of mu and the replicate whose removal "
                          "moves it most: columns mu_jk_se / mu_jk_max_shift / mu_jk_max_shift_rep / n_jk.  The two numeric "
                          "columns are on the scale of the column mu (the raw posterior mean), not of mu_scaled / mu_adj "
                          "that --fit-negctrl adds.  Not combined with --n-seeds > 1 or --load-existing.")
    own.add_argument("--jackknife-guides", dest="jackknife_guides", action="store_true",
                     help="Next to the fit of the screen, fit it once per guide position with the guide at that position "
                          "of every target masked (same seed; in the sorting variant models one such fit holds every "
                          "target's leave-one-guide-out fit) and report, per target, the jackknife standard error of mu "
                          "over its guides and the guide whose removal moves it most: columns mu_gjk_se / "
                          "mu_gjk_max_shift / mu_gjk_max_shift_guide / n_gjk, and mu_shift_left_out in the sgRNA table.  "
                          "The numeric columns are on the scale of the column mu (the raw posterior mean); --fit-negctrl "
                          "does not rescale them.  Variant screens only; not combined with --n-seeds > 1, "
                          "--jackknife-replicates or --load-existing.")
    own.add_argument("--jackknife-guides-max", dest="jackknife_guides_max", type=_positive_int, default=63,
                     help="Targets with more guides than this take no part in --jackknife-guides (default and "
                          "largest value 63: one member per guide position next to the full screen).")
    own.add_argument("--jackknife-samples", dest="jackknife_samples", action="store_true",
                     help="Next to the fit of the screen, fit it once per sorted sample (one condition of one replicate) "
                          "with that sample masked as --sample-mask-col masks it (same seed) and report, per target, how "
                          "far the removal of one sample moves mu and which sample does: columns mu_sjk_max_shift / "
                          "mu_sjk_max_shift_sample / n_sjk, on the scale of the column mu; and, per sample, its influence "
                          "over all targets in bean_sample_influence.<model>.csv.  No standard error is reported: samples "
                          "of different bins are not exchangeable.  Not combined with --jackknife-conditions, "
                          "--jackknife-replicates, --jackknife-guides, --n-seeds > 1 or --load-existing.")
    own.add_argument("--jackknife-conditions", dest="jackknife_conditions", action="store_true",
                     help="As --jackknife-samples, leaving out one condition (that bin of every replicate) per fit.")
    own.add_argument("--num-particles", dest="num_particles", type=_positive_int, default=1,
                     help="Draw every latent site this many times in each step of the main model's fit and update with the "
                          "mean of the gradients (Pyro's Trace_ELBO(num_particles=P); default 1, the reference's single "
                          "draw): one fit and the usual tables, with less gradient noise.  The --fit-negctrl fit of the "
                          "negative controls stays at one particle.  At most 64; not combined with --n-seeds > 1, any "
                          "--jackknife-* flag or --load-existing.")
    own.add_argument("--posterior-predictive", dest="posterior_predictive", type=_non_negative_int, default=0, metavar="S",
                     help="After the fit, draw S replicate screens from the fitted guide and the likelihood on the GPU "
                          "and compare them with the observed counts (a posterior predictive check): per guide, "
                          "ppc_p_score / ppc_z_score (does the model reproduce the guide's sorting score?) and "
                          "ppc_p_spread (do its replicates disagree more than the model predicts?) in "
                          "bean_predictive_guides.<model>.csv; per sample, the share of cells with p <= 0.05 and their "
                          "mean z in bean_predictive_samples.<model>.csv.  The other tables do not change.  With a member "
                          "set (--n-seeds, --jackknife-*) the check is of the fit the tables come from.  Sorting variant "
                          "screens only; the --fit-negctrl control fit is not checked.  Default 0: off.")
    own.add_argument("--predictive-seed", dest="predictive_seed", type=int, default=101,
                     help="Seed of the draws of --posterior-predictive and --survival-predictive (default 101).")
    own.add_argument("--survival-predictive", dest="survival_predictive", type=_non_negative_int, default=0, metavar="S",
                     help="The posterior predictive check of a survival variant screen: after the fit, draw S replicate "
                          "screens over the timepoints from the fitted guide and the likelihood on the GPU and compare them "
                          "with the observed counts.  Writes the tables of --posterior-predictive, "
                          "bean_predictive_guides.<model>.csv and bean_predictive_samples.<model>.csv, with the guide's "
                          "score read as its read-weighted mean time: ppc_z_score > 0 is a guide that grows faster than "
                          "the fitted model says.  The other tables do not change.  Survival variant screens (Normal, "
                          "MixtureNormal) only; the --fit-negctrl control fit is not checked.  Default 0: off.")
    own.add_argument("--importance-check", dest="importance_check", type=_non_negative_int, default=0, metavar="S",
                     help="After the fit, draw S times from the fitted mean-field guide on the GPU, weight every draw per "
                          "target by p(x, z) / q(z) and report, per target, the Pareto tail index of the weights and the "
                          "importance-corrected posterior: columns psis_k (below 0.5 the Gaussian can be trusted for "
                          "this target, above 0.7 it cannot be repaired at this S), mu_is / mu_sd_is (on the scale of the "
                          "column mu), is_ess and n_is in the element table.  No refit; the other tables do not change.  "
                          "Combines with the member flags and --load-existing: the check is of the fit the tables come "
                          "from.  At least 25 draws; sorting variant screens only; the --fit-negctrl control fit is not "
                          "checked.  Default 0: off.")
    own.add_argument("--importance-seed", dest="importance_seed", type=int, default=101,
                     help="Seed of the draws of --importance-check (default 101).")
    own.add_argument("--importance-integrate-pi", dest="importance_integrate_pi", action="store_true",
                     help="With --importance-check S: also weight the same draws by the weight of (mu, sd) alone, the "
                          "editing rates pi integrated out of the model by quadrature on the GPU - the joint weight of a "
                          "MixtureNormal target covers its 2 x replicates x guides pi coordinates, for which the guide is "
                          "a poor proposal whatever the quality of the Gaussian of mu.  Columns psis_k_marg, mu_is_marg, "
                          "mu_sd_is_marg, is_ess_marg and n_pairs_unresolved behind those of --importance-check; a target "
                          "with a (replicate, guide) pair the quadrature rule does not resolve (an essentially unedited "
                          "guide: prior concentration plus control reads of an allele below 2) has n_pairs_unresolved > 0 "
                          "and empty marginal columns.  With the Normal model, which has no pi, the marginal columns equal "
                          "the joint ones.")
    own.add_argument("--importance-nodes", dest="importance_nodes", type=int, default=32, metavar="Q",
                     help="Quadrature nodes per integral of --importance-integrate-pi: 16, 32 or 64 (default 32).")
    own.add_argument("--importance-tail-rule", dest="importance_tail_rule", action="store_true",
                     help="With --importance-integrate-pi: integrate the (replicate, guide) pairs its quadrature rule does "
                          "not resolve - an essentially unedited guide is one - by the 64-node Gauss-Jacobi rule of "
                          "--grid-tail-rule, per draw, and check it against the 48-node rule.  A target with such pairs "
                          "then gets its marginal columns where the two rules agree within 1e-3 nat per pair over the "
                          "draws that carry its weight (raw weight at least 1e-6 of the largest), and stays empty "
                          "otherwise.  Adds the columns n_pairs_tail and is_tail_err behind the marginal columns; "
                          "n_pairs_unresolved stays what it is.  Works with --scale-by-acc.  Refused without "
                          "--importance-integrate-pi.")
    own.add_argument("--grid-posterior", dest="grid_posterior", action="store_true",
                     help="After the fit, evaluate every target's posterior of (mu, sd) itself on the GPU - its log joint on "
                          "a grid of (mu, log sd) placed by zoom passes from the fitted values, the editing rates pi "
                          "integrated out by quadrature, no Gaussian and no guide involved - and report, per target: "
                          "columns mu_grid / mu_sd_grid (posterior mean and sd of mu without the mean-field assumption, "
                          "on the scale of the column mu), sd_grid, p_mu_pos_grid (P(mu > 0 | x)), log_evidence_grid, "
                          "log_bf10_grid (log Bayes factor against mu = 0), grid_ok and n_pairs_unresolved behind the "
                          "importance columns of the element table.  A target whose grid did not settle (grid_ok 0) or "
                          "with a (replicate, guide) pair the quadrature rule does not resolve has empty columns.  The "
                          "zoom follows one peak: a second mode of mu outside the final box is not detected.  No refit; "
                          "the other tables do not change.  Sorting variant screens only; not with --scale-by-acc.")
    own.add_argument("--grid-nodes", dest="grid_nodes", type=int, default=32, metavar="Q",
                     help="Quadrature nodes per integral of --grid-posterior: 16, 32 or 64 (default 32).")
    own.add_argument("--grid-tail-rule", dest="grid_tail_rule", action="store_true",
                     help="With --grid-posterior: integrate the (replicate, guide) pairs its quadrature rule does not "
                          "resolve - an essentially unedited guide is one - by a 64-node Gauss-Jacobi rule that carries "
                          "the pair's endpoint singularity in its weight, and check it against the 48-node rule.  A "
                          "target with such pairs then gets numbers where the two rules agree within 1e-3 nat per pair "
                          "over the nodes that hold its posterior, and stays empty otherwise (prior-data conflict in the "
                          "editing rate is the case the rule does not cover).  Adds the columns n_pairs_tail and "
                          "grid_tail_err behind the grid columns; n_pairs_unresolved stays what it is.  Refused without "
                          "--grid-posterior.")
    own.add_argument("--bootstrap", dest="bootstrap", type=_non_negative_int, default=0, metavar="K",
                     help="Parametric bootstrap: after the fit of the screen, draw K screens from the fitted model on the "
                          "GPU (mu, sd and the guide noise at their fitted locations; fresh pi, Dirichlet and count draws; "
                          "masks, size factors, a0, pi_a0 and every guide's total as observed), refit each with the same "
                          "seed and report, per target, the spread and the mean shift of mu over the refits: columns "
                          "mu_boot_se / mu_boot_bias / n_boot, on the scale of the column mu - a frequentist spread to "
                          "hold mu_sd against.  K >= 2; sorting variant screens only; not combined with --n-seeds > 1, any "
                          "--jackknife-* flag, --num-particles > 1 or --load-existing.  Default 0: off.")
    own.add_argument("--bootstrap-seed", dest="bootstrap_seed", type=int, default=101,
                     help="Seed of the simulated screens of --bootstrap and --survival-bootstrap (default 101).")
    own.add_argument("--survival-bootstrap", dest="survival_bootstrap", type=_non_negative_int, default=0, metavar="K",
                     help="Parametric bootstrap of a survival variant screen: after the fit of the screen, draw K screens "
                          "over the timepoints from the fitted model in one launch on the GPU (mu and the guide noise "
                          "at their fitted locations, the Normal model's initial abundance at the mean of its Dirichlet; "
                          "per screen a fresh baseline of the MixtureNormal model, fresh pi, Dirichlet and count draws; "
                          "masks, size factors, a0, pi_a0, the observed initial counts, the control fit's mu_negctrl and "
                          "every guide's total as observed), refit each with the same seed, one after the other, and "
                          "report the columns of --bootstrap: mu_boot_se / mu_boot_bias / n_boot.  K >= 2; survival "
                          "variant screens only (--bootstrap serves sorting screens); not combined with --bootstrap, "
                          "--design-depths, --power-effects, --n-seeds > 1, any --jackknife-* flag, --num-particles > 1 "
                          "or --load-existing; combines with --survival-predictive.  Default 0: off.")
    own.add_argument("--design-depths", dest="design_depths", type=parse_depths, default=None, metavar="F,F,...",
                     help="Depth study: after the fit of the screen, draw --design-screens screens from the fitted model "
                          "on the GPU at each of these read depths - a comma-separated list of factors > 0 such as "
                          "0.25,0.5,2,4; at factor f every (replicate, guide) draws round(f x its observed reads), "
                          "everything else (masks, size factors, a0, pi_a0) as observed: the same cells, other read "
                          "counts - refit each with the same seed and report how the spread of mu over the refits "
                          "changes with the depth: one row per depth in bean_design.<model>.csv (depth, n_screens, "
                          "median_total, median_mu_design_se, se_ratio against depth 1, recovery of the screen's hits, "
                          "n_hits) and the columns mu_design_se_x<f> in the element table, on the scale of the column "
                          "mu.  Depth 1 is added where absent.  Sorting variant screens only; not combined with "
                          "--bootstrap, --n-seeds > 1, any --jackknife-* flag, --num-particles > 1 or --load-existing.")
    own.add_argument("--design-screens", dest="design_screens", type=_positive_int, default=8, metavar="K",
                     help="Screens drawn and refitted per depth of --design-depths (default 8, at least 2).")
    own.add_argument("--design-seed", dest="design_seed", type=int, default=101,
                     help="Seed of the simulated screens of --design-depths (default 101).")
    own.add_argument("--power-effects", dest="power_effects", type=parse_effects, default=None, metavar="E,E,...",
                     help="Power study: after the fit of the screen, draw --power-screens screens from the fitted model on "
                          "the GPU with each of these effects planted - a comma-separated list such as 0.1,0.2,0.4, "
                          "negatives allowed (--power-effects=-0.5,0.5); with effect e every target's mu is e, the value "
                          "itself, everything else (sd, editing rates, masks, size factors, a0, pi_a0, totals) as fitted "
                          "and observed - refit each with the same seed and report how often a target is called (|z| >= "
                          "1.96 with the effect's sign): one row per effect in bean_power.<model>.csv (effect, n_screens, "
                          "n_planted, power_mean, power_median, shrinkage, median_mu_power_se) and the columns "
                          "power_x<e> and mde<100 level> (mde<100 level>_neg with negative effects) in the element "
                          "table.  Effect 0, whose rate is the false-positive rate, is added where absent.  Sorting "
                          "variant screens only; not combined with --bootstrap, --design-depths, --n-seeds > 1, any "
                          "--jackknife-* flag, --num-particles > 1 or --load-existing.")
    own.add_argument("--power-screens", dest="power_screens", type=_positive_int, default=8, metavar="K",
                     help="Screens drawn and refitted per effect of --power-effects (default 8, at least 2).")
    own.add_argument("--power-seed", dest="power_seed", type=int, default=101,
                     help="Seed of the simulated screens of --power-effects (default 101).")
    own.add_argument("--power-level", dest="power_level", type=_open_unit_interval, default=0.8, metavar="P",
                     help="The power the minimal detectable effect of --power-effects is read at, in (0, 1) (default 0.8: "
                          "the column mde80).")
    from .build_prior import attach_args as attach_prior_args

    attach_prior_args(sub.add_parser("build-prior", help="obtain prior_params.pkl for batched runs"))
    from .qc import attach_args as attach_qc_args

    attach_qc_args(sub.add_parser("qc", help="QC of the screen: mask low-quality samples and outlier guides"))
    return parser


def check_run_switches(parser, args):
    """Combinations of this project's own `bean run` switches that are refused (exit status 2, one sentence)."""
    from .run import (grid_nodes, grid_tail_rule, importance_draws, importance_nodes, importance_tail_rule, member_mode,
                      particle_count, predictive_draws, survival_predictive_draws)

    member_mode(args, parser.error,
                parser_rules={"jackknife_guides": (("guides_max", "--jackknife-guides-max is at most 63."),)})
    particle_count(args, parser.error)
    predictive_draws(args, parser.error)
    survival_predictive_draws(args, parser.error)
    importance_draws(args, parser.error)
    importance_nodes(args, parser.error)
    importance_tail_rule(args, parser.error)
    grid_nodes(args, parser.error)
    grid_tail_rule(args, parser.error)


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    if args.subcommand == "build-prior":
        from .build_prior import main as build_prior_main

        build_prior_main(args)
        return 0
    if args.subcommand == "qc":
        from .qc import main as qc_main

        qc_main(args)
        return 0
    if args.subcommand != "run":
        parser.print_help()
        return 2
    check_run_switches(parser, args)
    from .run import main as run_main

    try:
        run_main(args)
    finally:
        # `torchrun ... bean run`: leave the process group cleanly (RCCL communicators, store)
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
