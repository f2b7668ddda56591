"""What a posterior predictive check of a survival screen costs: S replicate screens drawn on the device and summarised.

    python scripts/time_survival_predictive.py [--reps 5] [--draws 200] [--out profiles/survival_predictive.json]

One process, this build (the protocol of time_predictive.py).  For each shape - 3 455 guides x 6 replicates x 6 timepoints
at the generator's default depth, and the screen `bench.py --config survival` builds (100 000 guides x 3 replicates x 6
timepoints) - a MixtureNormal engine is built and fitted for 300 steps, and 5 draws run untimed.  Then, `reps` times,
between two device synchronisations: `draws` calls of HipSVI.simulate_survival alone, and the whole check
(model/predictive.py::survival_predictive: the same draws plus the torch summary).  Recorded next to them, as context from
other hardware doing the same job: the time preprocessing/synthetic.py::_dirmult_counts (numpy, one host thread) takes to
draw replicate screens - both likelihoods, the concentrations and totals the device used - timed on `--host-screens`
screens per shape and scaled to `draws`.  There is no target and no parent figure: the parent commit has no such path.
The cost model is the sorting simulator's - a wave lasts ceil(n_max / 4) trips, n_max the largest total of its 64 pairs:
`trips_per_draw` is that sum over the waves and both likelihoods, `ns_per_wave_trip` the measured time over it.
"""
import argparse
import json
import os
import sys
import time

import member_timing as mt

SHAPES = (("3 455 x 6 x 6", 3455, 6, 7), ("bench.py --config survival", 100_000, 3, 20240506))
FAMILY = "MixtureNormal"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--host-screens", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "survival_predictive.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import numpy as np
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model.predictive import survival_predictive
    from bean_amd.preprocessing.synthetic import _dirmult_counts, make_survival_variant_screen

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rows = []
    for name, guides, reps, seed in SHAPES:
        data = make_survival_variant_screen(guides, reps, seed=seed).to(dev)
        eng = engine.HipSVI(FAMILY, data, num_steps=300)
        assert eng.survival_predictive_supported
        eng.run(300, seed=mt.SEED)
        for d in range(5):
            eng.simulate_survival(d, seed=mt.SEED)
        survival_predictive(eng, 2, seed=mt.SEED)
        torch.cuda.synchronize(dev)
        totals = [eng._keep[k].double().sum(1) for k in ("X", "X_BC")]    # (R, G) each
        n_tot = float(totals[0].sum() + totals[1].sum())
        G = int(data.n_guides)
        pad = (-G) % 64
        trips = 0.0
        for n in totals:  # the largest total of every 64-guide tile of every replicate
            tiles = torch.nn.functional.pad(n, (0, pad)).reshape(n.shape[0], -1, 64).max(-1).values
            trips += float(torch.ceil(tiles / 4).sum())
        t_sim, t_all = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for d in range(a.draws):
                eng.simulate_survival(d, seed=mt.SEED)
            torch.cuda.synchronize(dev)
            t_sim.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            summary = survival_predictive(eng, a.draws, seed=mt.SEED)
            torch.cuda.synchronize(dev)
            t_all.append(time.perf_counter() - t0)
            assert summary["n_draws"] == a.draws
        # the host generator on the same job: the concentrations and totals of one device draw
        sim = eng.simulate_survival(0, seed=mt.SEED, alphas=True)
        alpha = sim["alpha"].permute(0, 1, 3, 2).cpu().numpy()              # (2, R, G, B)
        host_n = [t.cpu().numpy().astype(np.int64) for t in totals]
        rng = np.random.default_rng(0)
        t0 = time.perf_counter()
        for d in range(a.host_screens):
            for lik in range(2):
                _dirmult_counts(rng, host_n[lik], alpha[lik])
        t_np = (time.perf_counter() - t0) / a.host_screens * a.draws
        s, w = mt.stats(t_sim), mt.stats(t_all)
        rows.append({
            "shape": name, "guides": guides, "replicates": reps, "conditions": int(data.n_condits), "family": FAMILY,
            "draws": a.draws, "likelihoods": 2, "categorical_draws_per_screen": n_tot,
            "wave_trips_per_draw": trips,
            "simulate_wall_s": s, "check_wall_s": w,
            "simulate_ms_per_draw": s["median"] / a.draws * 1e3,
            "ns_per_wave_trip": s["median"] / a.draws / trips * 1e9,
            "categorical_draws_per_s": n_tot * a.draws / s["median"],
            "numpy_dirmult_counts_wall_s": {"value": t_np, "screens_timed": a.host_screens, "scaled_to_draws": a.draws},
            "numpy_over_device_simulate": t_np / s["median"],
        })
        print(f"{name}: simulate_survival x{a.draws} {mt.ms(s)}  whole check {mt.ms(w)}  numpy _dirmult_counts "
              f"{t_np:.1f} s (x{t_np / s['median']:.0f}), {trips:.0f} wave trips per draw", flush=True)
        eng.close()
    out = {"what": "survival posterior predictive check: S replicate screens (bean_hip_simulate_survival) and their "
                   "summary, one process, wall time; numpy's _dirmult_counts on this host for the same screens as context",
           "repetitions": a.reps, "compute_units": cus, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
