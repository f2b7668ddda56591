"""K seeds of one small screen: one ensemble (this build) against K single fits in a row (a build of the parent commit).

    python scripts/time_ensemble.py --parent-lib /path/to/parent/libbean_hip.so [--reps 5] [--steps 2000]
                                    [--out profiles/ensemble_small_screens.json]

Two worker processes, one per library (the parent's is loaded through BEAN_HIP_LIB, which is read when the package is
imported), take turns: for every repetition and every (shape, K) the ensemble fit-set and the sequential fit-set run one
after the other, so drift of the box hits both.  A fit-set is K fits of `steps` SVI steps, stepped in windows of 100 as
run_inference steps them, between two device synchronisations (the fences of bench.py's Leg.timed); engines are built
outside the timed region on both sides.  Written: median / min / max wall time per fit-set and per step, and the waves
per SIMD of the two launches of a step.
"""
import member_timing as mt

SHAPES = [  # (label, guides, replicates, family, engine keywords)
    ("readme 3455x6 MixtureNormal", 3455, 6, "MixtureNormal", {}),
    ("readme 3455x6 MixtureNormal+Acc", 3455, 6, "MixtureNormal", {"scale_by_accessibility": True}),
    ("5000x3 MixtureNormal", 5000, 3, "MixtureNormal", {}),
    ("12500x3 MixtureNormal", 12500, 3, "MixtureNormal", {}),
]
KS = (1, 2, 4, 8, 16)


def build(engine, data, fam, kw, steps, mode, k):
    """K seeds: one engine of K members, or the one single-fit engine the fits of every K run on in a row."""
    return [engine.HipSVI(fam, data, num_steps=steps, n_members=k if mode == "ensemble" else 1, **kw)]


def worker():
    mt.serve(SHAPES, build, seeds_of=lambda data, k: [101 + j for j in range(k)], batched=("ensemble",),
             engines_key=lambda mode, k: (mode, k if mode == "ensemble" else 1))


def rows_of_shape(a, new, old, i, shape):
    label, guides, reps, fam, kw = shape
    sides = [(f"{m} {k}", w, {"mode": m, "k": k}) for k in KS for m, w in (("ensemble", new), ("sequential", old))]
    # (untimed first: the ensemble of every K, and the parent build's one single-fit engine)
    times, meta = mt.measure(a, i, sides, warm=sides[0::2] + sides[1:2])
    rows = []
    for k in KS:
        e, s = times[f"ensemble {k}"], times[f"sequential {k}"]
        rows.append({
            "shape": label, "guides": guides, "replicates": reps, "family": fam, "engine_kw": kw, "members": k,
            "steps": a.steps, "ensemble_wall_s": e, "sequential_parent_wall_s": s,
            "ensemble_ms_per_step": e["median"] / a.steps * 1e3,
            "sequential_ms_per_step_of_the_set": s["median"] / a.steps * 1e3, **mt.gain(e, s),
            "waves_per_simd": mt.waves_per_simd(guides, reps, meta["targets"], k, meta["cus"]),
        })
        print(f"{label:34s} K={k:2d}  ensemble {mt.ms(e)}  {k} parent fits {mt.ms(s)}  x{rows[-1]['speedup_median']:.2f}", flush=True)
    return rows


def summary(a, rows):
    cond = next(r for r in rows if r["shape"].startswith("readme") and r["family"] == "MixtureNormal"
                and not r["engine_kw"] and r["members"] == 8)
    out = {"what": "K-member seed ensemble (this build) vs K single fits in a row (parent build), wall time per fit-set",
           "steps_per_fit": a.steps, "window": mt.WINDOW, "repetitions": a.reps, "rows": rows,
           "condition_readme_k8_met": bool(cond["faster_by_more_than_the_spread"])}
    return out, f"README shape, K = 8: condition {'met' if out['condition_readme_k8_met'] else 'NOT met'}"


if __name__ == "__main__":
    mt.main(__file__, "ensemble_small_screens.json", worker, rows_of_shape, SHAPES, summary)
