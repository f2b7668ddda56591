"""What the tail rule of the marginal importance check costs, and what it buys after a 300-step fit (DESIGN.md section
25):

    python scripts/time_importance_tail.py [--reps 5] [--draws 1024] [--out profiles/importance_tail.json]

Section 23's protocol: one process, wall time, `--reps` (at least five) repetitions, median [min, max]; per shape (3 455
x 6 and 50 000 x 5, MixtureNormal, both likelihoods, a 300-step fit), S = 1 024 draws at Q = 32:

  tail    HipSVI.log_weights(0, S, integrate_pi=32, tail_rule=True);
  plain   HipSVI.log_weights(0, S, integrate_pi=32) of the same build, alternating with it - there is nothing on the
          parent commit to compare with, so there is no threshold.

Recorded next to them: the number of tail pairs and their share of the pairs under the repguide mask, the targets that
have one, of those the ones that get numbers, those the tail bar refuses, and the largest is_tail_err.
"""
import argparse
import json
import os
import sys
import time

import member_timing as mt

SHAPES = (("README shape", 3455, 6), ("metric shape", 50_000, 5))
FAMILY = "MixtureNormal"
Q = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "importance_tail.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import _lib, engine
    from bean_amd.model.importance import TAIL_BOUND, marginal_summary
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    S = a.draws

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    rows = []
    for name, guides, reps in SHAPES:
        host = make_sorting_variant_screen(guides, reps, seed=7)
        eng = engine.HipSVI(FAMILY, host.to(dev), num_steps=300)
        eng.run(300, seed=mt.SEED)
        torch.cuda.synchronize(dev)
        calls = {"tail": lambda: eng.log_weights(0, S, seed=mt.SEED, integrate_pi=Q, tail_rule=True),
                 "plain": lambda: eng.log_weights(0, S, seed=mt.SEED, integrate_pi=Q)}
        res, plain = calls["tail"](), calls["plain"]()  # first calls apart
        torch.cuda.synchronize(dev)
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():  # the sides alternate
                times[k].append(timed(fn)[0])
        summary = marginal_summary(res["logw"], res["mu"], res["n_unresolved"], tail_err=res["tail_err"])
        n_tail = summary["n_pairs_tail"]
        had = n_tail > 0
        got = had & ~summary["psis_k_marg"].isnan()
        barred = had & ~(summary["is_tail_err"] <= TAIL_BOUND * n_tail)
        untouched = bool(torch.equal(res["logw"][:, ~had], plain["logw"][:, ~had]) and torch.equal(res["mu"], plain["mu"]))
        pairs = float(host.repguide_mask.sum())
        chunk = max(1, min(S, _lib.MAX_LOGW_DRAWS, eng.LOGW_PAIR_BYTES // (8 * reps * guides)))
        eng.close()
        t, p = mt.stats(times["tail"]), mt.stats(times["plain"])
        row = {"shape": name, "guides": guides, "replicates": reps, "family": FAMILY, "targets": int(host.n_targets),
               "draws": S, "nodes": Q, "library_calls": -(-S // chunk),
               "log_weights_marginal_tail_wall_s": t, "log_weights_marginal_wall_s": p,
               "tail_pairs": int(n_tail.sum()), "share_of_pairs_tail": float(n_tail.sum()) / pairs,
               "targets_with_tail_pairs": int(had.sum()), "of_those_with_numbers": int(got.sum()),
               "refused_by_the_tail_bar": int(barred.sum()), "largest_is_tail_err": float(summary["is_tail_err"].max()),
               "targets_without_tail_pairs_keep_their_bits": untouched}
        print(f"{name}: integrate_pi={Q}, tail_rule=True {mt.ms(t)}; integrate_pi={Q} {mt.ms(p)}; {row['tail_pairs']} tail "
              f"pairs ({100 * row['share_of_pairs_tail']:.3f} % of the pairs) in {row['targets_with_tail_pairs']} targets, "
              f"{row['of_those_with_numbers']} of them with numbers, {row['refused_by_the_tail_bar']} refused by the tail "
              f"bar; largest is_tail_err {row['largest_is_tail_err']:.2e}; bits kept elsewhere: {untouched}", flush=True)
        rows.append(row)

    out = {"what": "HipSVI.log_weights(integrate_pi=32, tail_rule=True) (bean_hip_log_weights_marginal_tail) next to "
                   "integrate_pi=32 alone of the same build; one process, wall time, the calls alternating; no parent "
                   "figure exists, so no threshold",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "rows": rows}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
