"""Sample jackknife of one small screen: the 1 + R B fits (the screen, and one per sorted sample with that sample masked
and its counts zeroed) as members of one engine with their own counts (this build) against the same fits in a row (a
build of the parent commit), and against a mask-only ensemble of the same K on this build.

    python scripts/time_sample_jackknife.py --parent-lib /path/to/parent/libbean_hip.so [--reps 5] [--steps 2000]
                                            [--out profiles/sample_jackknife_small_screens.json]

Two worker processes, one per library (the parent's is loaded through BEAN_HIP_LIB, which is read when the package is
imported), take turns: for every repetition and every shape the three fit-sets run one after the other, so drift of the
box hits all of them.  A fit-set is the fit of the screen and of its R B leave-one-sample-out copies
(model/jackknife.py::leave_out_samples), `steps` SVI steps each with the same seed, stepped in windows of 100 as
run_inference_sample_jackknife steps them, between two device synchronisations; engines are built outside the timed
region on every side (the sequential side has one engine per copy: masks and counts are bound data).  "masks only" is
the same K members with the same sample masks but the SHARED counts (what a replicate jackknife of that K steps): not
the leave-one-sample-out fits, but the same launches without the members' private reads of X.  Written: median / min /
max wall time per fit-set, ms per step, the bytes of the member counts, the waves per SIMD of the two launches of a step.
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
SHAPES = [  # (label, guides, replicates, family, engine keywords): members = replicates x conditions + 1
    ("readme 3455x6 MixtureNormal", 3455, 6, "MixtureNormal", {}),
    ("readme 3455x6 MixtureNormal+Acc", 3455, 6, "MixtureNormal", {"scale_by_accessibility": True}),
    ("5000x3 MixtureNormal", 5000, 3, "MixtureNormal", {}),
    ("5000x3 MixtureNormal+Acc", 5000, 3, "MixtureNormal", {"scale_by_accessibility": True}),
]
SEED = 101


def worker():
    sys.path.insert(0, ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model.jackknife import leave_out_samples, sample_groups, sample_member_counts, sample_member_masks
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    dev = torch.device("cuda:0")
    screens, engines = {}, {}

    def screen(i):
        if i not in screens:
            _, g, r, _, kw = SHAPES[i]
            screens[i] = make_sorting_variant_screen(g, r, seed=7, with_accessibility=bool(kw.get("scale_by_accessibility"))).to(dev)
        return screens[i]

    def engines_of(i, mode, steps):
        if (i, mode) not in engines:
            for key in [key for key in engines if key[0] != i]:  # one shape's engines at a time
                for e in engines.pop(key):
                    e.close()
            _, _, _, fam, kw = SHAPES[i]
            data = screen(i)
            groups, _ = sample_groups(data, "sample")
            if mode == "batched":
                engines[(i, mode)] = [engine.HipSVI(fam, data, num_steps=steps, n_members=1 + len(groups),
                                                    member_masks=sample_member_masks(data, groups),
                                                    member_counts=sample_member_counts(data, groups), **kw)]
            elif mode == "masks_only":
                engines[(i, mode)] = [engine.HipSVI(fam, data, num_steps=steps, n_members=1 + len(groups),
                                                    member_masks=sample_member_masks(data, groups), **kw)]
            else:
                engines[(i, mode)] = [engine.HipSVI(fam, d, num_steps=steps, **kw)
                                      for d in [data] + [leave_out_samples(data, g) for g in groups]]
        return engines[(i, mode)]

    for line in sys.stdin:
        req = json.loads(line)
        if req["op"] == "quit":
            break
        i, steps, mode = req["shape"], req["steps"], req["mode"]
        es = engines_of(i, mode, req["capacity"])
        data = screen(i)
        k = data.n_reps * data.n_condits + 1
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if mode in ("batched", "masks_only"):
            for first in range(0, steps, WINDOW):
                es[0].run_ensemble(min(WINDOW, steps - first), [SEED] * k, first_step=first)
        else:
            for e in es:  # the fits in a row: every fit begins like a fresh one (its first window prepares)
                for first in range(0, steps, WINDOW):
                    e.run(min(WINDOW, steps - first), seed=SEED, first_step=first, resume=True)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        e = es[0]
        info = {"wall_s": dt, "kernel": e.dominant_kernel, "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                "targets": int(e.T), "members": k, "conditions": int(data.n_condits), "finite": all(bool(torch.isfinite(x.loss_hist).all()) for x in es)}
        sys.stdout.write(json.dumps(info) + "\n")
        sys.stdout.flush()
    for es in engines.values():
        for e in es:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_jackknife_small_screens.json"))
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
            times = {"batched": [], "sequential": [], "masks_only": []}
            # untimed: builds engines, captures graphs
            meta = new.ask(op="time", shape=i, steps=200, capacity=a.steps, mode="batched")
            new.ask(op="time", shape=i, steps=200, capacity=a.steps, mode="masks_only")
            old.ask(op="time", shape=i, steps=200, capacity=a.steps, mode="sequential")
            k, conds = meta["members"], meta["conditions"]
            for rep in range(a.reps):
                r1 = new.ask(op="time", shape=i, steps=a.steps, capacity=a.steps, mode="batched")
                r3 = new.ask(op="time", shape=i, steps=a.steps, capacity=a.steps, mode="masks_only")
                r2 = old.ask(op="time", shape=i, steps=a.steps, capacity=a.steps, mode="sequential")
                assert r1["finite"] and r2["finite"] and r3["finite"], label
                times["batched"].append(r1["wall_s"])
                times["sequential"].append(r2["wall_s"])
                times["masks_only"].append(r3["wall_s"])
            e, q, mo = stats(times["batched"]), stats(times["sequential"]), stats(times["masks_only"])
            n_counts = 2 if fam == "MixtureNormal" or kw.get("use_bcmatch", True) else 1
            spread = max(e["max"] - e["min"], q["max"] - q["min"])
            row = {
                "shape": label, "guides": guides, "replicates": reps, "family": fam, "engine_kw": kw, "members": k,
                "conditions": conds, "steps": a.steps, "batched_wall_s": e, "sequential_parent_wall_s": q,
                "masks_only_same_k_wall_s": mo, "batched_ms_per_step": e["median"] * 1e3 / a.steps,
                "masks_only_ms_per_step": mo["median"] * 1e3 / a.steps,
                "private_counts_over_masks_only": e["median"] / mo["median"],
                "member_counts_bytes": n_counts * 4 * k * reps * conds * guides,
                "speedup_median": q["median"] / e["median"],
                "gain_s": q["median"] - e["median"], "larger_min_max_spread_s": spread,
                "faster_by_more_than_the_spread": (q["median"] - e["median"]) > spread,
                "waves_per_simd": waves_per_simd(guides, reps, meta["targets"], k, meta["cus"]),
            }
            rows.append(row)
            print(f"{label:34s} K={k:2d}  batched {e['median']*1e3:8.1f} ms [{e['min']*1e3:.1f}, {e['max']*1e3:.1f}]  "
                  f"{k} parent fits {q['median']*1e3:8.1f} ms [{q['min']*1e3:.1f}, {q['max']*1e3:.1f}]  "
                  f"x{row['speedup_median']:.2f}  masks only {mo['median']*1e3:8.1f} ms [{mo['min']*1e3:.1f}, {mo['max']*1e3:.1f}]  "
                  f"counts {row['member_counts_bytes'] / 2**20:.1f} MiB", flush=True)
    finally:
        new.close()
        old.close()
    met = all(r["faster_by_more_than_the_spread"] for r in rows)
    out = {"what": "sample jackknife, 1 + R B leave-one-sample-out fits as members of one engine with their own counts "
                   "(this build) vs the same fits in a row (parent build) vs a mask-only ensemble of the same K (this "
                   "build), wall time per fit-set",
           "steps_per_fit": a.steps, "window": WINDOW, "repetitions": a.reps, "seed": SEED, "rows": rows,
           "condition_met_at_every_shape": bool(met)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"faster than the parent's fits in a row by more than the spread at every shape: {'yes' if met else 'NO'}; wrote {a.out}")


if __name__ == "__main__":
    main()
