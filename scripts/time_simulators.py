"""The six count simulators alone, for comparing two builds of the library.

    [BEAN_HIP_LIB=<other build>] python scripts/time_simulators.py OUT.json

The simulator calls that time_predictive.py, time_bootstrap.py, time_design.py, time_power.py,
time_survival_predictive.py and time_survival_bootstrap.py time, at their shapes and arguments, without their refits, torch
summaries and host comparisons (which run no simulator code): MixtureNormal, both likelihoods, an engine fitted for 300
steps, every call once untimed, then 7 repetitions with the calls of a shape taking turns, each between two device
synchronisations.  One process per build - BEAN_HIP_LIB names the library, as for those scripts; run the parent's build
twice for its own spread.  Writes {call: median, min, max} per shape.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bean_amd  # noqa: E402,F401
from bean_amd import engine  # noqa: E402
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen, make_survival_variant_screen  # noqa: E402

SEED, REPS = 101, 7
dev = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


rows = {}


def measure(shape, calls):
    for name, fn in calls:
        fn()
    ts = {name: [] for name, _ in calls}
    for _ in range(REPS):
        for name, fn in calls:
            ts[name].append(timed(fn))
    for name, xs in ts.items():
        rows[f"{shape} | {name}"] = stats(xs)
        s = rows[f"{shape} | {name}"]
        print(f"{shape:28s} {name:44s} {s['median']*1e3:9.2f} ms [{s['min']*1e3:.2f}, {s['max']*1e3:.2f}]", flush=True)


for shape, guides, reps in (("3455x6 sorting", 3455, 6), ("50000x5 sorting", 50_000, 5)):
    data = make_sorting_variant_screen(guides, reps, seed=7).to(dev)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(300, seed=SEED)
    eng.set_noise({"eps_mu": torch.zeros(eng.T, dtype=torch.float64, device=dev),
                   "eps_sd": torch.zeros(eng.T, dtype=torch.float64, device=dev)})
    nothing = torch.zeros(int(eng.T), dtype=torch.uint8)
    measure(shape, [
        ("simulate x 20 (k_simulate_wave2)", lambda: [eng.simulate(d, seed=SEED) for d in range(20)]),
        ("simulate_members(0, 32)", lambda: eng.simulate_members(0, 32, seed=SEED)),
        ("simulate_design(0, 8, (0.25, 1, 4))", lambda: eng.simulate_design(0, 8, (0.25, 1.0, 4.0), seed=SEED)),
        ("simulate_power(0, 8, (0, 0.25, 1))", lambda: eng.simulate_power(0, 8, (0.0, 0.25, 1.0), seed=SEED)),
        ("simulate_power(0, 8, (0,), nothing planted)", lambda: eng.simulate_power(0, 8, (0.0,), plant=nothing, seed=SEED)),
    ])
    eng.close()

for shape, guides, reps, seed in (("3455x6x6 survival", 3455, 6, 7), ("100000x3x6 survival", 100_000, 3, 20240506)):
    data = make_survival_variant_screen(guides, reps, seed=seed).to(dev)
    eng = engine.HipSVI("MixtureNormal", data, num_steps=300)
    eng.run(300, seed=SEED)
    eng.set_noise({"eps_mu": torch.zeros(eng.T, dtype=torch.float64, device=dev)})
    measure(shape, [
        ("simulate_survival x 20", lambda: [eng.simulate_survival(d, seed=SEED) for d in range(20)]),
        ("simulate_survival_members(0, 32)", lambda: eng.simulate_survival_members(0, 32, seed=SEED)),
    ])
    eng.close()

with open(sys.argv[1], "w") as fh:
    json.dump({"library": os.environ.get("BEAN_HIP_LIB", "tree"), "repetitions": REPS, "rows": rows}, fh, indent=1)
