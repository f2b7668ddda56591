"""What the tail rule of the grid posterior costs, and what it buys after a 300-step fit:

    python scripts/time_grid_tail.py [--reps 5] [--out profiles/grid_tail.json]

Section 22's protocol: one process, wall time, `--reps` (at least five) repetitions, median [min, max]; per shape (3 455
x 6 and 50 000 x 5, MixtureNormal, both likelihoods, a 300-step fit):

  tail    model/grid_posterior.py::grid_posterior(engine, tail_rule=True) with its defaults;
  plain   grid_posterior(engine) of the same build, alternating with it - there is nothing on the parent commit to
          compare with, so there is no threshold.

Recorded next to them: the share of (replicate, guide) pairs under the repguide mask that are tail pairs, the share of
targets that have one, of those the share that gets numbers, and the share the tail bar refuses.
"""
import argparse
import json
import os
import sys
import time

import member_timing as mt

SHAPES = (("README shape", 3455, 6), ("metric shape", 50_000, 5))
FAMILY = "MixtureNormal"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "grid_tail.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model.grid_posterior import grid_posterior
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

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
        res = grid_posterior(eng, tail_rule=True)  # first calls apart
        plain = grid_posterior(eng)
        torch.cuda.synchronize(dev)
        calls = {"tail": lambda: grid_posterior(eng, tail_rule=True), "plain": lambda: grid_posterior(eng)}
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():  # the sides alternate
                times[k].append(timed(fn)[0])
        n_tail = res["n_pairs_tail"]
        had = n_tail > 0
        pairs = float(host.repguide_mask.sum())
        same = ~had
        untouched = all(torch.equal(torch.isnan(res[k][same]), torch.isnan(plain[k][same]))
                        and torch.equal(torch.nan_to_num(res[k][same]), torch.nan_to_num(plain[k][same]))
                        for k in ("mu_grid", "mu_sd_grid", "log_evidence_grid"))
        eng.close()
        t, p = mt.stats(times["tail"]), mt.stats(times["plain"])
        row = {"shape": name, "guides": guides, "replicates": reps, "family": FAMILY, "targets": int(host.n_targets),
               "grid_posterior_tail_rule_wall_s": t, "grid_posterior_wall_s": p,
               "tail_pairs": int(n_tail.sum()), "share_of_pairs_tail": float(n_tail.sum()) / pairs,
               "share_of_targets_with_tail_pairs": float(had.double().mean()),
               "targets_with_tail_pairs": int(had.sum()),
               "of_those_with_numbers": int((had & res["grid_ok"]).sum()),
               "refused_by_the_tail_bar": int((had & ~res["grid_tail_ok"]).sum()),
               "largest_grid_tail_err": float(res["grid_tail_err"].max()),
               "share_of_targets_grid_ok_tail_rule": float(res["grid_ok"].double().mean()),
               "share_of_targets_grid_ok_plain": float(plain["grid_ok"].double().mean()),
               "targets_without_tail_pairs_keep_their_bits": untouched}
        print(f"{name}: grid_posterior(tail_rule=True) {mt.ms(t)}; grid_posterior {mt.ms(p)}; {row['tail_pairs']} tail pairs "
              f"({100 * row['share_of_pairs_tail']:.3f} % of the pairs) in {row['targets_with_tail_pairs']} targets, "
              f"{row['of_those_with_numbers']} of them with numbers, {row['refused_by_the_tail_bar']} refused by the tail "
              f"bar; largest grid_tail_err {row['largest_grid_tail_err']:.2e}; bits kept elsewhere: {untouched}", flush=True)
        rows.append(row)

    out = {"what": "grid_posterior(tail_rule=True) (bean_hip_marginal_grid_tail) next to grid_posterior of the same build; "
                   "one process, wall time, the calls alternating; no parent figure exists, so no threshold",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "rows": rows}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
