"""What a survival bootstrap costs, against the loop of single calls the parent commit offers.

    python scripts/time_survival_bootstrap.py [--reps 5] [--steps 2000] [--k 32] [--whole all|small|none]
                                              [--out profiles/survival_bootstrap.json]

One process, this build (the protocol of time_bootstrap.py; stats / gain / ms of member_timing.py).  For each shape -
3 455 guides x 6 replicates x 6 timepoints, and the screen `bench.py --config survival` builds (100 000 x 3 x 6) -
MixtureNormal, both likelihoods, K = 32:

(a) the draws.  An engine is built, fitted for 300 steps, the plug-in noise injected (model/run.py::
    survival_bootstrap_engine's zeros) and both sides run once untimed.  Then, `reps` times, the two sides one after the
    other, each between two device synchronisations: one HipSVI.simulate_survival_members(0, K) call, and K
    HipSVI.simulate_survival(d) calls, d = 0 ... K - 1 - the parent's path to the same K screens (the planes are compared
    with torch.equal in the warm-up).
(b) the whole bootstrap (`--whole`: at both shapes, the small one, or not at all).  run_survival_bootstrap(n_boot = K,
    `steps` steps), against the same work through the parent's entry points: run_inference on the screen, an engine with
    the fitted parameters and K simulate_survival calls, run_inference on each of the K screens - 1 + K fits in a row.
    Both sides run once untimed at 200 steps, then alternate `reps` times; wall time around the Python calls, engines built
    inside on both sides.  The refits of the warm-up are compared bit for bit.  Survival fits go one after the other on
    both sides, so the two differ in the draws alone.

No ratio is promised: the figures are what they are, and `faster_by_more_than_the_spread` says whether the difference of
the medians exceeds the larger min-max spread of the two sides.
"""
import argparse
import copy
import json
import os
import sys
import time
from functools import partial

import member_timing as mt

SHAPES = (("3 455 x 6 x 6", 3455, 6, 7), ("bench.py --config survival", 100_000, 3, 20240506))
FAMILY = "MixtureNormal"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--whole", choices=("all", "small", "none"), default="all")
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "survival_bootstrap.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model import run as model_run
    from bean_amd.model import survival_model as sm
    from bean_amd.preprocessing.synthetic import make_survival_variant_screen

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    K = a.k
    model, guide = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    def in_a_row(data, steps):
        """The parent's path: 1 + K run_inference calls and K simulate_survival calls."""
        full = model_run.run_inference(model, guide, data, num_steps=steps, seed=mt.SEED, verbose=False)
        eng = model_run.survival_bootstrap_engine(model, guide, data, full[0])
        try:
            sims = [eng.simulate_survival(d, seed=mt.SEED) for d in range(K)]
            torch.cuda.synchronize(dev)
        finally:
            eng.close()
        boots = []
        for sim in sims:
            screen = copy.copy(data)
            screen.X_masked = sim["X"].to(data.X_masked.device, data.X_masked.dtype)
            screen.X_bcmatch_masked = sim["X_bcmatch"].to(data.X_bcmatch_masked.device, data.X_bcmatch_masked.dtype)
            boots.append(model_run.run_inference(model, guide, screen, num_steps=steps, seed=mt.SEED, verbose=False))
        return full, boots

    def batched(data, steps):
        return model_run.run_survival_bootstrap(model, guide, data, n_boot=K, seed=mt.SEED, boot_seed=mt.SEED,
                                                num_steps=steps, verbose=False)

    rows = []
    for i, (name, guides, reps, seed) in enumerate(SHAPES):
        host = make_survival_variant_screen(guides, reps, seed=seed)
        # ---- (a) the draws
        eng = engine.HipSVI(FAMILY, host.to(dev), num_steps=300)
        eng.run(300, seed=mt.SEED)
        eng.set_noise({"eps_mu": torch.zeros(eng.T, dtype=torch.float64, device=dev)})
        many = eng.simulate_survival_members(0, K, seed=mt.SEED)
        singles = [eng.simulate_survival(d, seed=mt.SEED) for d in range(K)]
        torch.cuda.synchronize(dev)
        same = all(torch.equal(many[key][d], singles[d][key]) for key in many for d in range(K))
        assert same, "the planes of simulate_survival_members are not the single draws"
        del many, singles
        t_one, t_loop = [], []
        for _ in range(a.reps):
            t_one.append(timed(lambda: eng.simulate_survival_members(0, K, seed=mt.SEED))[0])
            t_loop.append(timed(lambda: [eng.simulate_survival(d, seed=mt.SEED) for d in range(K)])[0])
        n_tot = float(eng._keep["X"].double().sum() + eng._keep["X_BC"].double().sum())
        tiles = (guides + 63) // 64
        waves = (tiles + 7) // 8 * 8 * reps
        eng.close()
        e, q = mt.stats(t_one), mt.stats(t_loop)
        row = {"shape": name, "guides": guides, "replicates": reps, "conditions": int(host.n_condits), "family": FAMILY,
               "k": K, "likelihoods": 2, "categorical_draws_per_screen": n_tot,
               "simulate_survival_members_wall_s": e, "simulate_survival_loop_wall_s": q, "draws": mt.gain(e, q),
               "planes_bit_identical_in_warm_up": bool(same),
               "waves_per_simd": {"k_simulate_survival": waves / (4 * cus),
                                  "k_simulate_survival_members": waves * K / (4 * cus)}}
        print(f"{name} (a): simulate_survival_members(K={K}) {mt.ms(e)}  {K} x simulate_survival {mt.ms(q)}  "
              f"x{row['draws']['speedup_median']:.2f}", flush=True)
        # ---- (b) the whole bootstrap
        if a.whole == "all" or (a.whole == "small" and i == 0):
            got, want = batched(host, 200), in_a_row(host, 200)
            identical = all(torch.equal(x[1]["params"][p], y[1]["params"][p])
                            for x, y in zip([got[0]] + list(got[1]), [want[0]] + list(want[1])) for p in y[1]["params"])
            assert identical, "run_survival_bootstrap does not return the fits in a row"
            t_boot, t_row = [], []
            for _ in range(a.reps):
                t_boot.append(timed(lambda: batched(host, a.steps))[0])
                t_row.append(timed(lambda: in_a_row(host, a.steps))[0])
            e, q = mt.stats(t_boot), mt.stats(t_row)
            row.update({"steps": a.steps, "bootstrap_wall_s": e, "fits_in_a_row_wall_s": q, "bootstrap": mt.gain(e, q),
                        "refits_bit_identical_in_warm_up": bool(identical)})
            print(f"{name} (b): run_survival_bootstrap {mt.ms(e)}  {1 + K} run_inference + {K} simulate_survival "
                  f"{mt.ms(q)}  x{row['bootstrap']['speedup_median']:.2f}", flush=True)
        else:
            row["bootstrap"] = "not timed at this shape (--whole " + a.whole + ")"
        rows.append(row)
        with open(a.out + ".partial", "w") as fh:  # (what is measured so far, should the run be cut short)
            json.dump(rows, fh, indent=1)
    out = {"what": "survival bootstrap: K screens in one simulate_survival_members call against K simulate_survival calls, "
                   "and run_survival_bootstrap against 1 + K run_inference calls and K simulate_survival calls; one "
                   "process, wall time",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "whole": a.whole, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    os.remove(a.out + ".partial")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
