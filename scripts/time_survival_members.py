"""K survival fits of one screen as members of one engine (this build) against K single fits in a row (a build of the
parent commit), and the whole survival bootstrap with batched against sequential refits.

    python scripts/time_survival_members.py --parent-lib /path/to/parent/libbean_hip.so [--reps 5] [--steps 2000]
                                            [--whole all|small|none] [--out profiles/survival_members.json]

The protocol of time_ensemble.py (member_timing.py): two worker processes, one per library (the parent's is loaded through
BEAN_HIP_LIB), take turns - for every repetition and every (shape, K) the member fit-set and the sequential fit-set run
one after the other, so drift of the box hits both.  A fit-set is K fits of `steps` SVI steps in windows of 100, between
two device synchronisations; engines are built and warmed (200 untimed steps) outside the timed region on both sides.
Before a shape is timed, fresh engines of this build fit 200 steps as 4 members and as single fits, and every parameter,
both Adam moments and the loss history of the first and the last member are compared with torch.equal.

The whole bootstrap (`--whole`): run_survival_bootstrap(n_boot = 32, `steps` steps) with batch_refits=True against
batch_refits=False - the parent's path through the same Python: 1 + 32 run_inference calls' worth of fits, the single-fit
kernels being the same code objects in both builds - in the worker of this build, alternating, engines built inside on
both sides; the refits of a 200-step warm-up are compared bit for bit.

No ratio is promised: `faster_by_more_than_the_spread` says whether the difference of the medians exceeds the larger
min-max spread of the two sides, `slower_by_more_than_the_spread` the same the other way round.
"""
import json
import os
import sys
import time
from functools import partial

import member_timing as mt

SHAPES = [  # (label, guides, replicates, screen seed, family, engine keywords)
    ("3 455 x 6 x 6 MixtureNormal", 3455, 6, 7, "MixtureNormal", {}),
    ("3 455 x 6 x 6 MixtureNormal+Acc", 3455, 6, 7, "MixtureNormal", {"scale_by_accessibility": True}),
    ("bench.py --config survival (100 000 x 3 x 6) MixtureNormal", 100_000, 3, 20240506, "MixtureNormal", {}),
]
KS = (1, 2, 4, 8, 16, 32)
N_BOOT = 32
CHECK_K, CHECK_STEPS = 4, 200


def seeds_of(k):
    return [mt.SEED + j for j in range(k)]


def worker():
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model import run as model_run
    from bean_amd.model import survival_model as sm
    from bean_amd.preprocessing.synthetic import make_survival_variant_screen

    dev = torch.device("cuda:0")
    hosts, screens, built = {}, {}, {}

    def state(eng, member=None):
        pick = (lambda t: t) if member is None else (lambda t: t[member])
        out = [pick(v) for d in (eng.unconstrained, eng._m, eng._v) for _, v in sorted(d.items())]
        return out + [pick(eng.loss_hist)[: eng.steps_done]]

    for line in sys.stdin:
        req = json.loads(line)
        if req["op"] == "quit":
            break
        i = req["shape"]
        _, g, r, seed, fam, kw = SHAPES[i]
        if i not in screens:
            hosts[i] = make_survival_variant_screen(g, r, seed=seed, with_accessibility=bool(kw.get("scale_by_accessibility")))
            screens[i] = hosts[i].to(dev)
        data = screens[i]
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        if req["op"] == "check":  # member bits against the single fits', on fresh engines
            seeds = seeds_of(CHECK_K)
            ens = engine.HipSVI(fam, data, num_steps=CHECK_STEPS, n_members=CHECK_K, **kw)
            ens.run_ensemble(CHECK_STEPS, seeds)
            same = True
            for k in (0, CHECK_K - 1):
                one = engine.HipSVI(fam, data, num_steps=CHECK_STEPS, **kw)
                one.run(CHECK_STEPS, seed=seeds[k])
                torch.cuda.synchronize(dev)
                same = same and all(torch.equal(a, b) for a, b in zip(state(ens, k), state(one)))
                one.close()
            ens.close()
            reply = {"same": bool(same)}
        elif req["op"] == "bootstrap":
            model, guide = partial(sm.MixtureNormalModel), partial(sm.MixtureNormalGuide)  # (rows without engine keywords)
            boot = lambda batched, steps: model_run.run_survival_bootstrap(  # noqa: E731
                model, guide, hosts[i], n_boot=N_BOOT, seed=mt.SEED, boot_seed=mt.SEED, num_steps=steps, verbose=False,
                batch_refits=batched)
            if req.get("compare"):
                got, want = boot(True, CHECK_STEPS), boot(False, CHECK_STEPS)
                same = all(torch.equal(x[1]["params"][p], y[1]["params"][p]) and x[1]["loss"] == y[1]["loss"]
                           for x, y in zip([got[0]] + list(got[1]), [want[0]] + list(want[1])) for p in y[1]["params"])
                reply = {"same": bool(same)}
            else:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                boot(req["batched"], req["steps"])
                torch.cuda.synchronize(dev)
                reply = {"wall_s": time.perf_counter() - t0, "finite": True}
        else:
            steps, mode, k = req["steps"], req["mode"], req["k"]
            key = (i, mode, k if mode == "members" else 1)
            if key not in built:
                for old in [old for old in built if old[0] != i]:  # one shape's engines at a time
                    built.pop(old).close()
                built[key] = engine.HipSVI(fam, data, num_steps=req["capacity"], n_members=key[2], **kw)
            eng, seeds = built[key], seeds_of(k)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if mode == "members":
                for first in range(0, steps, mt.WINDOW):
                    eng.run_ensemble(min(mt.WINDOW, steps - first), seeds, first_step=first)
            else:  # the fits in a row: every fit begins like a fresh one (its first window prepares)
                for s in seeds:
                    for first in range(0, steps, mt.WINDOW):
                        eng.run(min(mt.WINDOW, steps - first), seed=s, first_step=first, resume=True)
            torch.cuda.synchronize(dev)
            reply = {"wall_s": time.perf_counter() - t0, "kernel": eng.dominant_kernel, "cus": cus, "targets": int(eng.T),
                     "conditions": int(data.n_condits), "finite": bool(torch.isfinite(eng.loss_hist).all())}
        sys.stdout.write(json.dumps(reply) + "\n")
        sys.stdout.flush()
    for e in built.values():
        e.close()


def waves_per_simd(guides, reps, targets, k, cus):
    """Of the two launches of a step: single-wave workgroups of the guide kernel (the grid padded to 8 tiles), and the four
    waves of every 256-thread block of k_param - target blocks at 4 lanes per target, alpha_pi blocks and q0 blocks."""
    simds = 4 * cus
    tiles = (guides + 63) // 64
    gblocks = (guides + 255) // 256
    return {"k_guide_survival_wave": (tiles + 7) // 8 * 8 * reps * k / simds,
            "k_param": 4 * ((targets * 4 + 255) // 256 + 2 * gblocks) * k / simds}


def loss(e, q):
    spread = max(e["max"] - e["min"], q["max"] - q["min"])
    return {"slower_by_more_than_the_spread": (e["median"] - q["median"]) > spread}


def rows_of_shape(a, new, old, i, shape):
    label, guides, reps, _, fam, kw = shape
    same = new.ask(op="check", shape=i)["same"]
    assert same, f"{label}: members differ from the single fits"
    sides = [(f"{m} {k}", w, {"mode": m, "k": k}) for k in KS for m, w in (("members", new), ("sequential", old))]
    times, meta = mt.measure(a, i, sides, warm=sides[0::2] + sides[1:2])
    rows = []
    for k in KS:
        e, s = times[f"members {k}"], times[f"sequential {k}"]
        rows.append({
            "shape": label, "guides": guides, "replicates": reps, "timepoints": meta["conditions"], "family": fam,
            "engine_kw": kw, "members": k, "steps": a.steps, "members_wall_s": e, "sequential_parent_wall_s": s,
            "members_ms_per_fit_set": e["median"] * 1e3, "sequential_ms_per_fit_set": s["median"] * 1e3,
            **mt.gain(e, s), **loss(e, s), "member_bits_are_the_single_fits_in_warm_up": bool(same),
            "waves_per_simd": waves_per_simd(guides, reps, meta["targets"], k, meta["cus"]),
        })
        print(f"{label:44s} K={k:2d}  members {mt.ms(e)}  {k} parent fits {mt.ms(s)}  x{rows[-1]['speedup_median']:.2f}",
              flush=True)
    return rows


def bootstrap_row(a, new, i, shape):
    label, guides, reps, _, fam, kw = shape
    same = new.ask(op="bootstrap", shape=i, compare=True)["same"]
    assert same, f"{label}: batched refits differ from the refits in a row"
    tb, ts = [], []
    for _ in range(a.reps):
        tb.append(new.ask(op="bootstrap", shape=i, batched=True, steps=a.steps)["wall_s"])
        ts.append(new.ask(op="bootstrap", shape=i, batched=False, steps=a.steps)["wall_s"])
    e, s = mt.stats(tb), mt.stats(ts)
    row = {"shape": label, "guides": guides, "replicates": reps, "family": fam, "n_boot": N_BOOT, "steps": a.steps,
           "batched_refits_wall_s": e, "refits_in_a_row_wall_s": s, **mt.gain(e, s), **loss(e, s),
           "refits_bit_identical_in_warm_up": bool(same)}
    print(f"{label:44s} run_survival_bootstrap({N_BOOT})  batched {mt.ms(e)}  in a row {mt.ms(s)}  "
          f"x{row['speedup_median']:.2f}", flush=True)
    return row


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--whole", choices=("all", "small", "none"), default="all")
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "survival_members.json"))
    a = ap.parse_args()
    if a.worker:
        worker()
        sys.exit(0)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: a libbean_hip.so built from the parent commit (the sequential baseline)")
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    new, old = mt.Worker(__file__), mt.Worker(__file__, a.parent_lib)
    out = {"what": "K survival member fits (this build) vs K single fits in a row (parent build), wall time per fit-set; "
                   "run_survival_bootstrap with batched vs sequential refits",
           "steps_per_fit": a.steps, "window": mt.WINDOW, "repetitions": a.reps, "seed": mt.SEED, "rows": [], "bootstrap": []}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    try:
        for i, shape in enumerate(SHAPES):
            out["rows"] += rows_of_shape(a, new, old, i, shape)
            with open(a.out + ".partial", "w") as fh:  # (what is measured so far, should the run be cut short)
                json.dump(out, fh, indent=1)
        for i, shape in enumerate(SHAPES):
            if shape[5] or a.whole == "none" or (a.whole == "small" and i > 0):
                continue  # (the bootstrap rows: MixtureNormal without accessibility, the two shapes of DESIGN.md section 27)
            out["bootstrap"].append(bootstrap_row(a, new, i, shape))
            with open(a.out + ".partial", "w") as fh:
                json.dump(out, fh, indent=1)
    finally:
        new.close()
        old.close()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    os.remove(a.out + ".partial")
    print(f"wrote {a.out}")
