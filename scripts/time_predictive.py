"""What a posterior predictive check costs: S replicate screens drawn on the device and summarised.

    python scripts/time_predictive.py [--reps 5] [--draws 200] [--out profiles/predictive_check.json]

One process, this build (the protocol of time_particles.py).  For each shape - the README shape, 3 455 guides x 6
replicates, and the metric shape, 50 000 x 5 - a MixtureNormal engine is built and fitted for 300 steps, and 5 draws run
untimed.  Then, `reps` times, between two device synchronisations: `draws` calls of HipSVI.simulate alone, and the whole
check (model/predictive.py::posterior_predictive: the same draws plus the torch summary).  Recorded next to them, as
context from other hardware doing the same job: the time preprocessing/synthetic.py::_dirmult_counts (numpy, one host
thread) takes to draw the same number of replicate screens - both likelihoods, the concentrations and totals the device
used - once per shape.  There is no target and no parent figure: the parent commit has no such path.
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
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "predictive_check.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import numpy as np
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model.predictive import posterior_predictive
    from bean_amd.preprocessing.synthetic import _dirmult_counts, make_sorting_variant_screen

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows = []
    for name, guides, reps in SHAPES:
        data = make_sorting_variant_screen(guides, reps, seed=7).to(dev)
        eng = engine.HipSVI(FAMILY, data, num_steps=300)
        assert eng.predictive_supported
        eng.run(300, seed=mt.SEED)
        for d in range(5):
            eng.simulate(d, seed=mt.SEED)
        posterior_predictive(eng, 2, seed=mt.SEED)
        torch.cuda.synchronize(dev)
        n_tot = float(eng._keep["X"].double().sum() + eng._keep["X_BC"].double().sum())
        t_sim, t_all = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for d in range(a.draws):
                eng.simulate(d, seed=mt.SEED)
            torch.cuda.synchronize(dev)
            t_sim.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            summary = posterior_predictive(eng, a.draws, seed=mt.SEED)
            torch.cuda.synchronize(dev)
            t_all.append(time.perf_counter() - t0)
            assert summary["n_draws"] == a.draws
        # the host generator on the same job: the concentrations and totals of one device draw, `draws` screens each
        sim = eng.simulate(0, seed=mt.SEED, alphas=True)
        alpha = sim["alpha"].permute(0, 1, 3, 2).cpu().numpy()              # (2, R, G, B)
        totals = [eng._keep[k].double().sum(1).cpu().numpy().astype(np.int64) for k in ("X", "X_BC")]
        rng = np.random.default_rng(0)
        t0 = time.perf_counter()
        for d in range(a.draws):
            for lik in range(2):
                _dirmult_counts(rng, totals[lik], alpha[lik])
            if d % 20 == 19:
                print(f"  numpy: {d + 1} of {a.draws} screens, {time.perf_counter() - t0:.1f} s", flush=True)
        t_np = time.perf_counter() - t0
        s, w = mt.stats(t_sim), mt.stats(t_all)
        rows.append({
            "shape": name, "guides": guides, "replicates": reps, "conditions": int(data.n_condits), "family": FAMILY,
            "draws": a.draws, "likelihoods": 2, "categorical_draws_per_screen": n_tot,
            "simulate_wall_s": s, "check_wall_s": w,
            "simulate_ms_per_draw": s["median"] / a.draws * 1e3,
            "categorical_draws_per_s": n_tot * a.draws / s["median"],
            "numpy_dirmult_counts_wall_s": {"value": t_np, "n": 1},
            "numpy_over_device_simulate": t_np / s["median"],
        })
        print(f"{name}: simulate x{a.draws} {mt.ms(s)}  whole check {mt.ms(w)}  numpy _dirmult_counts {t_np:.1f} s "
              f"(x{t_np / s['median']:.0f})", flush=True)
        eng.close()
    out = {"what": "posterior predictive check: S replicate screens (bean_hip_simulate) and their summary, one process, "
                   "wall time; numpy's _dirmult_counts on this host for the same screens as context",
           "repetitions": a.reps, "compute_units": cus, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
