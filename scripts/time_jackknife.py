"""Replicate jackknife of one small screen: the R + 1 masked fits as members of one engine (this build) against the same
R + 1 fits in a row (a build of the parent commit).

    python scripts/time_jackknife.py --parent-lib /path/to/parent/libbean_hip.so [--reps 5] [--steps 2000]
                                     [--out profiles/jackknife_small_screens.json]

Two worker processes, one per library (the parent's is loaded through BEAN_HIP_LIB, which is read when the package is
imported), take turns: for every repetition and every shape the batched fit-set and the sequential fit-set run one after
the other, so drift of the box hits both.  A fit-set is the fit of the screen and of its R leave-one-replicate-out copies
(model/jackknife.py: the replicate's rows of the two masks zeroed), `steps` SVI steps each with the same seed, stepped in
windows of 100 as run_inference_jackknife steps them, between two device synchronisations; engines are built outside the
timed region on both sides (the sequential side has one engine per masked copy: the masks are bound data).  Written:
median / min / max wall time per fit-set and the waves per SIMD of the two launches of a step.
"""
import member_timing as mt

SHAPES = [  # (label, guides, replicates, family, engine keywords): members = replicates + 1
    ("readme 3455x6 MixtureNormal", 3455, 6, "MixtureNormal", {}),
    ("readme 3455x6 MixtureNormal+Acc", 3455, 6, "MixtureNormal", {"scale_by_accessibility": True}),
    ("5000x3 MixtureNormal", 5000, 3, "MixtureNormal", {}),
    ("5000x3 MixtureNormal+Acc", 5000, 3, "MixtureNormal", {"scale_by_accessibility": True}),
]
WHAT = ("replicate jackknife, R + 1 masked fits as members of one engine (this build) vs the same fits in a row "
        "(parent build), wall time per fit-set")


def build(engine, data, fam, kw, steps, mode, k):
    from bean_amd.model.jackknife import candidate_replicates, leave_out, member_masks

    left_out = candidate_replicates(data)
    if mode == "batched":
        return [engine.HipSVI(fam, data, num_steps=steps, n_members=1 + len(left_out),
                              member_masks=member_masks(data, left_out), **kw)]
    return [engine.HipSVI(fam, d, num_steps=steps, **kw) for d in [data] + [leave_out(data, r) for r in left_out]]


def seeds_of(data, k):
    return [mt.SEED] * (data.n_reps + 1)


def rows_of_shape(a, new, old, i, shape):
    return [mt.jackknife_row(a, i, shape, [("batched", new, {"mode": "batched"}), ("sequential", old, {"mode": "sequential"})])]


if __name__ == "__main__":
    mt.main(__file__, "jackknife_small_screens.json", lambda: mt.serve(SHAPES, build, seeds_of), rows_of_shape, SHAPES,
            lambda a, rows: mt.jackknife_summary(a, rows, WHAT))
