"""What a power study costs, and what it reports on the generated screens.

    python scripts/time_power.py [--reps 5] [--steps 2000] [--k 8] [--parent-lib PATH] [--out profiles/power_study.json]

One MI355X, this build in this process (stats / ms of member_timing.py), warmed, `reps` repetitions, median [min, max].
For each shape - the README shape, 3 455 guides x 6 replicates, and the metric shape, 50 000 x 5 - MixtureNormal, both
likelihoods, effects (0, 0.25, 1), K = 8.  An engine is built, fitted for 300 steps and the plug-in noise injected
(model/run.py::bootstrap_engine's zeros); every call is timed between two device synchronisations:

(i)   the one call: HipSVI.simulate_power(0, K, effects), every target planted.
(ii)  what the flag costs a lane that plants nothing: simulate_power(0, K, [0]) with an all-zero mask, next to - with
      --parent-lib, a libbean_hip.so built from the parent commit, loaded by a second process through BEAN_HIP_LIB - the
      parent build's simulate_members(0, K) on an engine prepared the same way; the two alternate.  `within_the_spread`
      says whether the medians differ by no more than the larger min-max spread of the two sides.  A figure, not a test.
(iii) the parent build's route to the screens of (i): per effect, write mu_loc = effect on the device, then
      simulate_members(0, K) - D parameter writes, D PREP launches, D launches of K members - in the second process,
      alternating with (i).  Its planes are compared with (i)'s through a checksum.
(iv)  the whole study: run_inference_power(effects, n_screens = K, `steps` steps): wall time around the Python call,
      engines built inside (as a user pays for them), once untimed at 200 steps first; and, of the last repetition,
      power_mean / power_median / shrinkage per effect and the share of targets with a finite mde80.
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
EFFECTS = (0.0, 0.25, 1.0)


def _prepared(engine, torch, dev, guides, reps):
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    host = make_sorting_variant_screen(guides, reps, seed=7)
    eng = engine.HipSVI(FAMILY, host.to(dev), num_steps=300)
    eng.run(300, seed=mt.SEED)
    zeros = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    eng.set_noise({"eps_mu": zeros(eng.T), "eps_sd": zeros(eng.T)})
    return host, eng


def _checksum(torch, planes):
    """One number per plane set that any changed count changes: the counts against fixed pseudo-random weights."""
    total = 0.0
    for key in sorted(planes):
        x = planes[key].double().reshape(-1)
        w = (torch.arange(x.numel(), device=x.device, dtype=torch.float64) * 0.6180339887498949) % 1.0
        total += float((x * w).sum())
    return total


def worker():
    """The parent build's side: simulate_members(0, k) of the shape asked for ("members"), or the route to the planted
    screens - per effect mu_loc written, then simulate_members ("route") - timed between two synchronisations."""
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
        eng = built[i]
        if req["op"] == "members":
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng.simulate_members(0, req["k"], seed=mt.SEED)
            torch.cuda.synchronize(dev)
            reply = {"wall_s": time.perf_counter() - t0}
        else:
            fitted = eng.unconstrained["mu_loc"].clone()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            planes = []
            for e in req["effects"]:
                eng.unconstrained["mu_loc"].fill_(e)
                planes.append(eng.simulate_members(0, req["k"], seed=mt.SEED))
            torch.cuda.synchronize(dev)
            reply = {"wall_s": time.perf_counter() - t0,
                     "checksum": _checksum(torch, {k: torch.stack([p[k] for p in planes]) for k in planes[0]})}
            eng.unconstrained["mu_loc"].copy_(fitted)
        sys.stdout.write(json.dumps(reply) + "\n")
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
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "power_study.json"))
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
            host, eng = _prepared(engine, torch, dev, guides, reps)
            nothing = torch.zeros(eng.T, dtype=torch.uint8, device=dev)
            grid = eng.simulate_power(0, K, EFFECTS, seed=mt.SEED)
            unplanted = eng.simulate_power(0, K, [0.0], plant=nothing, seed=mt.SEED)
            members = eng.simulate_members(0, K, seed=mt.SEED)
            torch.cuda.synchronize(dev)
            assert all(torch.equal(unplanted[key][0], members[key]) for key in members)
            checksum = _checksum(torch, grid)
            del grid, unplanted, members
            same_screens = None
            if parent:
                parent.ask(op="members", shape=i, k=K)
                same_screens = parent.ask(op="route", shape=i, k=K, effects=list(EFFECTS))["checksum"] == checksum
            t_grid, t_none, t_parent, t_route = [], [], [], []
            for _ in range(a.reps):
                t_grid.append(timed(lambda: eng.simulate_power(0, K, EFFECTS, seed=mt.SEED))[0])
                if parent:
                    t_route.append(parent.ask(op="route", shape=i, k=K, effects=list(EFFECTS))["wall_s"])
                t_none.append(timed(lambda: eng.simulate_power(0, K, [0.0], plant=nothing, seed=mt.SEED))[0])
                if parent:
                    t_parent.append(parent.ask(op="members", shape=i, k=K)["wall_s"])
            n_obs = eng._keep["X"].double().sum(1)
            eng.close()
            g, o = mt.stats(t_grid), mt.stats(t_none)
            row = {"shape": name, "guides": guides, "replicates": reps, "conditions": int(host.n_condits), "family": FAMILY,
                   "k": K, "effects": list(EFFECTS), "likelihoods": 2, "targets": int(host.n_targets),
                   "median_observed_total": float(n_obs.median()), "simulate_power_wall_s": g,
                   "simulate_power_nothing_planted_one_effect_wall_s": o}
            text = ""
            if parent:
                p, r = mt.stats(t_parent), mt.stats(t_route)
                spread = max(o["max"] - o["min"], p["max"] - p["min"])
                row.update({"parent_simulate_members_wall_s": p, "larger_min_max_spread_s": spread,
                            "nothing_planted_minus_parent_median_s": o["median"] - p["median"],
                            "within_the_spread": abs(o["median"] - p["median"]) <= spread,
                            "parent_route_wall_s": r, "parent_route_draws_the_same_screens": same_screens,
                            "route_over_one_call_median": r["median"] / g["median"]})
                text = f"  parent simulate_members {mt.ms(p)}  parent route {mt.ms(r)} (same screens: {same_screens})"
            print(f"{name} (i)-(iii): simulate_power(D=3, K={K}) {mt.ms(g)}  nothing planted, D=1 {mt.ms(o)}{text}", flush=True)
            # ---- (iv) the whole study
            study = lambda steps: model_run.run_inference_power(model, guide, host, EFFECTS, n_screens=K, seed=mt.SEED,  # noqa: E731
                                                                power_seed=mt.SEED, num_steps=steps, verbose=False)
            study(200)
            t_study, last = [], None
            for _ in range(a.reps):
                dt, last = timed(lambda: study(a.steps))
                t_study.append(dt)
            s = jk.power_summary(last[0], last[1], EFFECTS)
            row.update({"steps": a.steps, "fits": 1 + len(EFFECTS) * K, "run_inference_power_wall_s": mt.stats(t_study),
                        "power_mean": s["power_mean"].tolist(), "power_median": s["power_median"].tolist(),
                        "shrinkage": s["shrinkage"].tolist(), "level": s["level"],
                        "share_of_targets_with_finite_mde": float(torch.isfinite(s["mde"]).double().mean()),
                        "median_finite_mde": float(torch.quantile(s["mde"][torch.isfinite(s["mde"])], 0.5))
                        if bool(torch.isfinite(s["mde"]).any()) else None,
                        "median_mu_power_se": [float(torch.quantile(v, 0.5)) for v in s["mu_power_se"]]})
            print(f"{name} (iv): run_inference_power {mt.ms(row['run_inference_power_wall_s'])}  power_mean "
                  f"{[round(v, 3) for v in row['power_mean']]}  shrinkage {[round(v, 3) for v in row['shrinkage']]}  "
                  f"finite mde80 on {row['share_of_targets_with_finite_mde']:.3f} of the targets", flush=True)
            rows.append(row)
    finally:
        if parent:
            parent.close()
    out = {"what": "power study: D x K screens in one simulate_power call, the nothing-planted call next to the parent "
                   "build's simulate_members, the parent build's route to the same screens, and run_inference_power with "
                   "its summary; wall time",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "parent_lib_given": bool(a.parent_lib), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
