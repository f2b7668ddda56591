"""What a depth study costs, and what it reports on the generated screens.

    python scripts/time_design.py [--reps 5] [--steps 2000] [--k 8] [--parent-lib PATH] [--out profiles/design_study.json]

One MI355X, this build in this process (stats / gain / ms of member_timing.py), warmed, `reps` repetitions, median
[min, max].  For each shape - the README shape, 3 455 guides x 6 replicates, and the metric shape, 50 000 x 5 -
MixtureNormal, both likelihoods, depths (0.25, 1, 4), K = 8:

(a) the one call.  An engine is built, fitted for 300 steps, the plug-in noise injected (model/run.py::bootstrap_engine's
    zeros); HipSVI.simulate_design(0, K, depths) between two device synchronisations.  Next to it the depth-1-only call
    simulate_design(0, K, [1]) and - with --parent-lib, a libbean_hip.so built from the parent commit, loaded by a second
    process through BEAN_HIP_LIB - the parent build's simulate_members(0, K) on an engine prepared the same way; the two
    alternate.  They run the same body: `within_the_spread` says whether the medians differ by no more than the larger
    min-max spread of the two sides.  A figure, not a test.
(b) the whole study.  run_inference_design(depths, n_screens = K, `steps` steps): wall time around the Python call,
    engines built inside (as a user pays for them), once untimed at 200 steps first; and, of the last repetition,
    se_ratio / recovery / median_total per depth (model/jackknife.py::design_summary).
"""
import argparse
import json
import os
import sys
import time
from functools import partial

import member_timing as mt

SHAPES = (("README shape", 3455, 6), ("metric shape", 50_000, 5))
FAMILY = "MixtureNormal"
DEPTHS = (0.25, 1.0, 4.0)


def _prepared(engine, torch, dev, guides, reps):
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    host = make_sorting_variant_screen(guides, reps, seed=7)
    eng = engine.HipSVI(FAMILY, host.to(dev), num_steps=300)
    eng.run(300, seed=mt.SEED)
    zeros = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    eng.set_noise({"eps_mu": zeros(eng.T), "eps_sd": zeros(eng.T)})
    return host, eng


def worker():
    """The parent build's side of (a): simulate_members(0, k) of the shape asked for, timed between two synchronisations."""
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine

    dev = torch.device("cuda:0")
    built = {}
    for line in sys.stdin:
        req = json.loads(line)
        if req["op"] == "quit":
            break
        i = req["shape"]
        if i not in built:
            for e in built.values():
                e.close()
            built.clear()
            built[i] = _prepared(engine, torch, dev, *SHAPES[i][1:])[1]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        built[i].simulate_members(0, req["k"], seed=mt.SEED)
        torch.cuda.synchronize(dev)
        sys.stdout.write(json.dumps({"wall_s": time.perf_counter() - t0}) + "\n")
        sys.stdout.flush()
    for e in built.values():
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "design_study.json"))
    a = ap.parse_args()
    if a.worker:
        return worker()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    if a.parent_lib and not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libbean_hip.so built from the parent commit")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model import jackknife as jk
    from bean_amd.model import model as m
    from bean_amd.model import run as model_run

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    K = a.k
    model, guide = partial(m.MixtureNormalModel), partial(m.MixtureNormalGuide)
    parent = mt.Worker(__file__, a.parent_lib) if a.parent_lib else None

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    rows = []
    try:
        for i, (name, guides, reps) in enumerate(SHAPES):
            # ---- (a) the one call
            host, eng = _prepared(engine, torch, dev, guides, reps)
            grid = eng.simulate_design(0, K, DEPTHS, seed=mt.SEED)
            one = eng.simulate_design(0, K, [1.0], seed=mt.SEED)
            members = eng.simulate_members(0, K, seed=mt.SEED)
            torch.cuda.synchronize(dev)
            assert all(torch.equal(grid[key][1], members[key]) and torch.equal(one[key][0], members[key]) for key in members)
            del grid, one, members
            if parent:
                parent.ask(op="time", shape=i, k=K)
            t_grid, t_one, t_parent = [], [], []
            for _ in range(a.reps):
                t_grid.append(timed(lambda: eng.simulate_design(0, K, DEPTHS, seed=mt.SEED))[0])
                t_one.append(timed(lambda: eng.simulate_design(0, K, [1.0], seed=mt.SEED))[0])
                if parent:
                    t_parent.append(parent.ask(op="time", shape=i, k=K)["wall_s"])
            n_obs = eng._keep["X"].double().sum(1)
            eng.close()
            g, o = mt.stats(t_grid), mt.stats(t_one)
            row = {"shape": name, "guides": guides, "replicates": reps, "conditions": int(host.n_condits), "family": FAMILY,
                   "k": K, "depths": list(DEPTHS), "likelihoods": 2, "median_observed_total": float(n_obs.median()),
                   "largest_observed_total": float(n_obs.max()), "simulate_design_wall_s": g,
                   "simulate_design_depth_1_only_wall_s": o}
            text = ""
            if parent:
                p = mt.stats(t_parent)
                spread = max(o["max"] - o["min"], p["max"] - p["min"])
                row.update({"parent_simulate_members_wall_s": p, "larger_min_max_spread_s": spread,
                            "depth_1_minus_parent_median_s": o["median"] - p["median"],
                            "within_the_spread": abs(o["median"] - p["median"]) <= spread})
                text = f"  parent simulate_members {mt.ms(p)}"
            print(f"{name} (a): simulate_design(D=3, K={K}) {mt.ms(g)}  depth 1 only {mt.ms(o)}{text}", flush=True)
            # ---- (b) the whole study
            study = lambda steps: model_run.run_inference_design(model, guide, host, DEPTHS, n_screens=K, seed=mt.SEED,  # noqa: E731
                                                                 design_seed=mt.SEED, num_steps=steps, verbose=False)
            study(200)
            t_study, last = [], None
            for _ in range(a.reps):
                dt, last = timed(lambda: study(a.steps))
                t_study.append(dt)
            s = jk.design_summary(last[0], last[1], DEPTHS, data=host)
            row.update({"steps": a.steps, "fits": 1 + len(DEPTHS) * K, "run_inference_design_wall_s": mt.stats(t_study),
                        "se_ratio": s["se_ratio"].tolist(), "recovery": s["recovery"].tolist(), "n_hits": s["n_hits"],
                        "median_total": s["median_total"].tolist(), "n_left_out": s["n_left_out"],
                        "median_mu_design_se": [float(torch.quantile(v, 0.5)) for v in s["mu_design_se"]],
                        "median_mu_design_sd": [float(torch.quantile(v, 0.5)) for v in s["mu_design_sd"]]})
            print(f"{name} (b): run_inference_design {mt.ms(row['run_inference_design_wall_s'])}  se_ratio "
                  f"{[round(v, 3) for v in row['se_ratio']]}  recovery {[round(v, 3) for v in row['recovery']]}  "
                  f"hits {row['n_hits']}", flush=True)
            rows.append(row)
    finally:
        if parent:
            parent.close()
    out = {"what": "depth study: D x K screens in one simulate_design call, the depth-1-only call next to the parent build's "
                   "simulate_members, and run_inference_design with its summary; wall time",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "parent_lib_given": bool(a.parent_lib), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
