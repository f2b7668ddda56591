"""What the four member timing scripts (time_ensemble.py, time_jackknife.py, time_guide_jackknife.py,
time_sample_jackknife.py) share: K fits of one small screen as members of one engine (this build) against the same fits in
a row (a build of the parent commit).

Two worker processes, one per library (the parent's is loaded through BEAN_HIP_LIB, which is read when the package is
imported), take turns: for every repetition the fit-sets of a shape run one after the other, so drift of the box hits all
of them.  A fit-set is `steps` SVI steps per fit, stepped in windows of 100 as run_inference steps them, between two device
synchronisations (the fences of bench.py's Leg.timed); engines are built outside the timed region on every side.

A script keeps what is its own: SHAPES, `seeds_of(data, k)`, `build(engine, data, family, kw, steps, mode, k) -> engines` -
one engine with a member per seed for a batched mode, else the engines the seeds are fitted on in a row (seed j on engine j
modulo their number) -, `engines_key(mode, k)`, what a request's engines depend on (they are built once per shape and key,
in the untimed warm-up), and its rows.
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
SEED = 101


def serve(shapes, build, seeds_of, batched=("batched",), engines_key=lambda mode, k: (mode, k)):
    """The worker's request loop: screens and engines are cached (one shape's engines at a time, one set per
    ``engines_key``), a request is timed between two synchronisations and answered with one JSON line."""
    sys.path.insert(0, ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    dev = torch.device("cuda:0")
    screens, built = {}, {}
    for line in sys.stdin:
        req = json.loads(line)
        if req["op"] == "quit":
            break
        i, steps, mode, k = req["shape"], req["steps"], req["mode"], req.get("k")
        _, g, r, fam, kw = shapes[i]
        if i not in screens:
            screens[i] = make_sorting_variant_screen(g, r, seed=7, with_accessibility=bool(kw.get("scale_by_accessibility"))).to(dev)
        data = screens[i]
        if (i, engines_key(mode, k)) not in built:
            for key in [key for key in built if key[0] != i]:  # one shape's engines at a time
                for e in built.pop(key):
                    e.close()
            built[(i, engines_key(mode, k))] = build(engine, data, fam, kw, req["capacity"], mode, k)
        es, seeds = built[(i, engines_key(mode, k))], seeds_of(data, k)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if mode in batched:
            for first in range(0, steps, WINDOW):
                es[0].run_ensemble(min(WINDOW, steps - first), seeds, first_step=first)
        else:
            for j, s in enumerate(seeds):  # the fits in a row: every fit begins like a fresh one (its first window prepares)
                for first in range(0, steps, WINDOW):
                    es[j % len(es)].run(min(WINDOW, steps - first), seed=s, first_step=first, resume=True)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        info = {"wall_s": dt, "kernel": es[0].dominant_kernel, "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
                "targets": int(es[0].T), "members": len(seeds), "conditions": int(data.n_condits),
                "finite": all(bool(torch.isfinite(x.loss_hist).all()) for x in es)}
        sys.stdout.write(json.dumps(info) + "\n")
        sys.stdout.flush()
    for es in built.values():
        for e in es:
            e.close()


class Worker:
    def __init__(self, script, lib=None):
        env = dict(os.environ)
        if lib:
            env["BEAN_HIP_LIB"] = os.path.abspath(lib)
        else:
            env.pop("BEAN_HIP_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(script), "--worker"], stdin=subprocess.PIPE,
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


def measure(a, shape, sides, warm=None):
    """The alternating driver for one shape.  ``sides`` is a list of ``(name, worker, request)``; every side in ``warm``
    (default: all) runs 200 untimed steps first (builds engines, captures graphs), then for each of ``a.reps`` repetitions
    the sides run ``a.steps`` steps in their order.  Returns ``({name: stats of the wall times}, first warm-up's reply)``."""
    meta = None
    for _, worker, req in (sides if warm is None else warm):
        reply = worker.ask(op="time", shape=shape, steps=200, capacity=a.steps, **req)
        meta = meta or reply
    times = {name: [] for name, _, _ in sides}
    for _ in range(a.reps):
        for name, worker, req in sides:
            reply = worker.ask(op="time", shape=shape, steps=a.steps, capacity=a.steps, **req)
            assert reply["finite"], (shape, name)
            times[name].append(reply["wall_s"])
    return {name: stats(xs) for name, xs in times.items()}, meta


def gain(e, q):
    """The row fields that compare a batched fit-set ``e`` with the sequential one ``q`` (both ``stats``)."""
    spread = max(e["max"] - e["min"], q["max"] - q["min"])
    return {"speedup_median": q["median"] / e["median"], "gain_s": q["median"] - e["median"],
            "larger_min_max_spread_s": spread, "faster_by_more_than_the_spread": (q["median"] - e["median"]) > spread}


def ms(x):
    return f"{x['median']*1e3:8.1f} ms [{x['min']*1e3:.1f}, {x['max']*1e3:.1f}]"


def jackknife_row(a, i, shape, sides, more=None):
    """One shape of a jackknife script: its sides measured, "batched" against "sequential".  ``more(times, members,
    conditions)`` may add ``(fields after "members", fields after the wall times, text for the printed line)``."""
    label, guides, reps, fam, kw = shape
    times, meta = measure(a, i, sides)
    e, q, k = times["batched"], times["sequential"], meta["members"]
    early, late, text = more(times, k, meta["conditions"]) if more else ({}, {}, "")
    row = {"shape": label, "guides": guides, "replicates": reps, "family": fam, "engine_kw": kw, "members": k, **early,
           "steps": a.steps, "batched_wall_s": e, "sequential_parent_wall_s": q, **late, **gain(e, q),
           "waves_per_simd": waves_per_simd(guides, reps, meta["targets"], k, meta["cus"])}
    print(f"{label:34s} K={k:2d}  batched {ms(e)}  {k} parent fits {ms(q)}  x{row['speedup_median']:.2f}{text}", flush=True)
    return row


def jackknife_summary(a, rows, what):
    met = all(r["faster_by_more_than_the_spread"] for r in rows)
    out = {"what": what, "steps_per_fit": a.steps, "window": WINDOW, "repetitions": a.reps, "seed": SEED, "rows": rows,
           "condition_met_at_every_shape": bool(met)}
    return out, f"faster than the parent's fits in a row by more than the spread at every shape: {'yes' if met else 'NO'}"


def main(script, default_out, worker, rows_of_shape, shapes, summary):
    """Parse the command line; as ``--worker`` serve, else start the two workers, collect ``rows_of_shape(a, new, old, i,
    shape)`` over ``shapes`` and write ``{**summary(a, rows)[0], ...}`` to ``--out``, printing ``summary(a, rows)[1]``."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", default_out))
    a = ap.parse_args()
    if a.worker:
        return worker()
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libbean_hip.so built from the parent commit (the sequential baseline)")
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    new, old = Worker(script), Worker(script, a.parent_lib)
    rows = []
    try:
        for i, shape in enumerate(shapes):
            rows += rows_of_shape(a, new, old, i, shape)
    finally:
        new.close()
        old.close()
    out, message = summary(a, rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"{message}; wrote {a.out}")
