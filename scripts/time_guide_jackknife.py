"""Guide jackknife of one small screen: the 1 + Lmax masked fits as members of one engine (this build) against the same
1 + Lmax fits in a row (a build of the parent commit).

    python scripts/time_guide_jackknife.py --parent-lib /path/to/parent/libbean_hip.so [--reps 5] [--steps 2000]
                                           [--out profiles/guide_jackknife_small_screens.json]

Two worker processes, one per library (the parent's is loaded through BEAN_HIP_LIB, which is read when the package is
imported), take turns: for every repetition and every shape the batched fit-set and the sequential fit-set run one after
the other, so drift of the box hits both.  A fit-set is the fit of the screen and, for each of the Lmax = 5 guide
positions, of its copy with the guide at that position of every target masked (model/jackknife.py: those columns of
repguide_mask zeroed; in these families that one fit holds every target's leave-one-guide-out fit), `steps` SVI steps each
with the same seed, stepped in windows of 100 as run_inference_guide_jackknife steps them, between two device
synchronisations; engines are built outside the timed region on both sides (the sequential side has one engine per masked
copy: the masks are bound data).  Written: median / min / max wall time per fit-set and the waves per SIMD of the two
launches of a step.
"""
import member_timing as mt

SHAPES = [  # (label, guides, replicates, family, engine keywords): 5 guides per target, members = 5 + 1
    ("readme 3455x6 MixtureNormal", 3455, 6, "MixtureNormal", {}),
    ("readme 3455x6 MixtureNormal+Acc", 3455, 6, "MixtureNormal", {"scale_by_accessibility": True}),
    ("5000x3 MixtureNormal", 5000, 3, "MixtureNormal", {}),
    ("5000x3 MixtureNormal+Acc", 5000, 3, "MixtureNormal", {"scale_by_accessibility": True}),
]
LMAX = 5  # guides per target of make_sorting_variant_screen
WHAT = ("guide jackknife, 1 + Lmax masked fits as members of one engine (this build) vs the same fits in a row "
        "(parent build), wall time per fit-set")


def build(engine, data, fam, kw, steps, mode, k):
    from bean_amd.model.jackknife import guides_at_position, guide_member_masks, guide_positions, leave_out_guides

    positions, _ = guide_positions(data)
    assert len(positions) == LMAX
    if mode == "batched":
        return [engine.HipSVI(fam, data, num_steps=steps, n_members=1 + LMAX,
                              member_masks=guide_member_masks(data, positions), **kw)]
    return [engine.HipSVI(fam, d, num_steps=steps, **kw)
            for d in [data] + [leave_out_guides(data, guides_at_position(data, j)) for j in positions]]


def seeds_of(data, k):
    return [mt.SEED] * (1 + LMAX)


def rows_of_shape(a, new, old, i, shape):
    return [mt.jackknife_row(a, i, shape, [("batched", new, {"mode": "batched"}), ("sequential", old, {"mode": "sequential"})])]


if __name__ == "__main__":
    mt.main(__file__, "guide_jackknife_small_screens.json", lambda: mt.serve(SHAPES, build, seeds_of), rows_of_shape, SHAPES,
            lambda a, rows: mt.jackknife_summary(a, rows, WHAT))
