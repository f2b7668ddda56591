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
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = 100
SHAPES = [  # (label, guides, replicates, family, engine keywords)
    ("readme 3455x6 MixtureNormal", 3455, 6, "MixtureNormal", {}),
    ("readme 3455x6 MixtureNormal+Acc", 3455, 6, "MixtureNormal", {"scale_by_accessibility": True}),
    ("5000x3 MixtureNormal", 5000, 3, "MixtureNormal", {}),
    ("12500x3 MixtureNormal", 12500, 3, "MixtureNormal", {}),
]
KS = (1, 2, 4, 8, 16)


def worker():
    sys.path.insert(0, ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    dev = torch.device("cuda:0")
    screens, engines = {}, {}

    def screen(i):
        if i not in screens:
            _, g, r, _, kw = SHAPES[i]
            screens[i] = make_sorting_variant_screen(g, r, seed=7, with_accessibility=bool(kw.get("scale_by_accessibility"))).to(dev)
        return screens[i]

    def eng_of(i, k, steps):
        if (i, k) not in engines:
            for key in [key for key in engines if key[0] != i]:  # one shape's engines at a time
                engines.pop(key).close()
            _, _, _, fam, kw = SHAPES[i]
            engines[(i, k)] = engine.HipSVI(fam, screen(i), num_steps=steps, n_members=k, **kw)
        return engines[(i, k)]

    for line in sys.stdin:
        req = json.loads(line)
        if req["op"] == "quit":
            break
        i, k, steps, mode = req["shape"], req["k"], req["steps"], req["mode"]
        seeds = [101 + j for j in range(k)]
        e = eng_of(i, k if mode == "ensemble" else 1, req["capacity"])
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if mode == "ensemble":
            for first in range(0, steps, WINDOW):
                e.run_ensemble(min(WINDOW, steps - first), seeds, first_step=first)
        else:
            for s in seeds:  # K fits in a row on one engine: every fit begins like a fresh one (its first window prepares)
                for first in range(0, steps, WINDOW):
                    e.run(min(WINDOW, steps - first), seed=s, first_step=first, resume=True)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        info = {"wall_s": dt, "kernel": e.dominant_kernel, "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                "targets": int(e.T), "finite": bool(torch.isfinite(e.loss_hist).all())}
        sys.stdout.write(json.dumps(info) + "\n")
        sys.stdout.flush()
    for e in engines.values():
        e.close()


class Worker:
    def __init__(self, lib=None):
        env = dict(os.environ)
        if lib:
            env["BEAN_HIP_LIB"] = os.path.abspath(lib)
        else:
            env.pop("BEAN_HIP_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=env)

    def ask(self, **req):
        self.p.stdin.write(json.dumps(req) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"worker died (exit status {self.p.poll()})")
        return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def waves_per_simd(guides, reps, targets, k, cus):
    simds = 4 * cus
    tiles = (guides + 63) // 64
    guide_waves = (tiles + 7) // 8 * 8 * reps * k
    param_blocks = (targets * 16 + 255) // 256 + (guides + 255) // 256
    return {"k_guide_wave2": guide_waves / simds, "k_param": 4 * param_blocks * k / simds}


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_small_screens.json"))
    a = ap.parse_args()
    if a.worker:
        return worker()
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libbean_hip.so built from the parent commit (the sequential baseline)")
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    new, old = Worker(), Worker(a.parent_lib)
    rows = []
    try:
        for i, (label, guides, reps, fam, kw) in enumerate(SHAPES):
            times = {(k, m): [] for k in KS for m in ("ensemble", "sequential")}
            meta = None
            for k in KS:  # untimed: builds engines, captures graphs
                meta = new.ask(op="time", shape=i, k=k, steps=200, capacity=a.steps, mode="ensemble")
            old.ask(op="time", shape=i, k=1, steps=200, capacity=a.steps, mode="sequential")
            for rep in range(a.reps):
                for k in KS:
                    r1 = new.ask(op="time", shape=i, k=k, steps=a.steps, capacity=a.steps, mode="ensemble")
                    r2 = old.ask(op="time", shape=i, k=k, steps=a.steps, capacity=a.steps, mode="sequential")
                    assert r1["finite"] and r2["finite"], (label, k)
                    times[(k, "ensemble")].append(r1["wall_s"])
                    times[(k, "sequential")].append(r2["wall_s"])
            for k in KS:
                e, s = stats(times[(k, "ensemble")]), stats(times[(k, "sequential")])
                spread = max(e["max"] - e["min"], s["max"] - s["min"])
                row = {
                    "shape": label, "guides": guides, "replicates": reps, "family": fam, "engine_kw": kw, "members": k,
                    "steps": a.steps, "ensemble_wall_s": e, "sequential_parent_wall_s": s,
                    "ensemble_ms_per_step": e["median"] / a.steps * 1e3,
                    "sequential_ms_per_step_of_the_set": s["median"] / a.steps * 1e3,
                    "speedup_median": s["median"] / e["median"],
                    "gain_s": s["median"] - e["median"], "larger_min_max_spread_s": spread,
                    "faster_by_more_than_the_spread": (s["median"] - e["median"]) > spread,
                    "waves_per_simd": waves_per_simd(guides, reps, meta["targets"], k, meta["cus"]),
                }
                rows.append(row)
                print(f"{label:34s} K={k:2d}  ensemble {e['median']*1e3:8.1f} ms [{e['min']*1e3:.1f}, {e['max']*1e3:.1f}]  "
                      f"{k} parent fits {s['median']*1e3:8.1f} ms [{s['min']*1e3:.1f}, {s['max']*1e3:.1f}]  "
                      f"x{row['speedup_median']:.2f}", flush=True)
    finally:
        new.close()
        old.close()
    cond = next(r for r in rows if r["shape"].startswith("readme") and r["family"] == "MixtureNormal"
                and not r["engine_kw"] and r["members"] == 8)
    out = {"what": "K-member seed ensemble (this build) vs K single fits in a row (parent build), wall time per fit-set",
           "steps_per_fit": a.steps, "window": WINDOW, "repetitions": a.reps, "rows": rows,
           "condition_readme_k8_met": bool(cond["faster_by_more_than_the_spread"])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"README shape, K = 8: condition {'met' if out['condition_readme_k8_met'] else 'NOT met'}; wrote {a.out}")


if __name__ == "__main__":
    main()
