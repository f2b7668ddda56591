"""Sample jackknife of one small screen: the 1 + R B fits (the screen, and one per sorted sample with that sample masked
and its counts zeroed) as members of one engine with their own counts (this build) against the same fits in a row (a
build of the parent commit), and against a mask-only ensemble of the same K on this build.

    python scripts/time_sample_jackknife.py --parent-lib /path/to/parent/libbean_hip.so [--reps 5] [--steps 2000]
                                            [--out profiles/sample_jackknife_small_screens.json]

Two worker processes, one per library (the parent's is loaded through BEAN_HIP_LIB, which is read when the package is
imported), take turns: for every repetition and every shape the three fit-sets run one after the other, so drift of the
box hits all of them.  A fit-set is the fit of the screen and of its R B leave-one-sample-out copies
(model/jackknife.py::leave_out_samples), `steps` SVI steps each with the same seed, stepped in windows of 100 as
run_inference_sample_jackknife steps them, between two device synchronisations; engines are built outside the timed
region on every side (the sequential side has one engine per copy: masks and counts are bound data).  "masks only" is
the same K members with the same sample masks but the SHARED counts (what a replicate jackknife of that K steps): not
the leave-one-sample-out fits, but the same launches without the members' private reads of X.  Written: median / min /
max wall time per fit-set, ms per step, the bytes of the member counts, the waves per SIMD of the two launches of a step.
"""
import member_timing as mt

SHAPES = [  # (label, guides, replicates, family, engine keywords): members = replicates x conditions + 1
    ("readme 3455x6 MixtureNormal", 3455, 6, "MixtureNormal", {}),
    ("readme 3455x6 MixtureNormal+Acc", 3455, 6, "MixtureNormal", {"scale_by_accessibility": True}),
    ("5000x3 MixtureNormal", 5000, 3, "MixtureNormal", {}),
    ("5000x3 MixtureNormal+Acc", 5000, 3, "MixtureNormal", {"scale_by_accessibility": True}),
]
WHAT = ("sample jackknife, 1 + R B leave-one-sample-out fits as members of one engine with their own counts "
        "(this build) vs the same fits in a row (parent build) vs a mask-only ensemble of the same K (this "
        "build), wall time per fit-set")


def build(engine, data, fam, kw, steps, mode, k):
    from bean_amd.model.jackknife import leave_out_samples, sample_groups, sample_member_counts, sample_member_masks

    groups, _ = sample_groups(data, "sample")
    if mode == "sequential":
        return [engine.HipSVI(fam, d, num_steps=steps, **kw) for d in [data] + [leave_out_samples(data, g) for g in groups]]
    counts = {"member_counts": sample_member_counts(data, groups)} if mode == "batched" else {}
    return [engine.HipSVI(fam, data, num_steps=steps, n_members=1 + len(groups),
                          member_masks=sample_member_masks(data, groups), **counts, **kw)]


def seeds_of(data, k):
    return [mt.SEED] * (data.n_reps * data.n_condits + 1)


def rows_of_shape(a, new, old, i, shape):
    label, guides, reps, fam, kw = shape
    n_counts = 2 if fam == "MixtureNormal" or kw.get("use_bcmatch", True) else 1

    def more(times, k, conds):  # the mask-only ensemble of the same K, and what the members' own counts cost
        e, mo = times["batched"], times["masks_only"]
        extra = {"masks_only_same_k_wall_s": mo, "batched_ms_per_step": e["median"] * 1e3 / a.steps,
                 "masks_only_ms_per_step": mo["median"] * 1e3 / a.steps,
                 "private_counts_over_masks_only": e["median"] / mo["median"],
                 "member_counts_bytes": n_counts * 4 * k * reps * conds * guides}
        return {"conditions": conds}, extra, f"  masks only {mt.ms(mo)}  counts {extra['member_counts_bytes'] / 2**20:.1f} MiB"

    sides = [("batched", new, {"mode": "batched"}), ("masks_only", new, {"mode": "masks_only"}),
             ("sequential", old, {"mode": "sequential"})]
    return [mt.jackknife_row(a, i, shape, sides, more)]


if __name__ == "__main__":
    mt.main(__file__, "sample_jackknife_small_screens.json",
            lambda: mt.serve(SHAPES, build, seeds_of, batched=("batched", "masks_only")), rows_of_shape, SHAPES,
            lambda a, rows: mt.jackknife_summary(a, rows, WHAT))
