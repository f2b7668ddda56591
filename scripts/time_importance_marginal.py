"""What the importance weights with pi integrated out cost, and what they say after a 300-step fit:

    python scripts/time_importance_marginal.py [--reps 5] [--draws 1024] [--out profiles/importance_marginal.json]

One process, wall time, `--reps` (at least five) repetitions, median [min, max]; per shape (3 455 x 6 and 50 000 x 5,
MixtureNormal, both likelihoods, a 300-step fit) and per Q in 16 / 32 / 64:

  log_weights_marginal   HipSVI.log_weights(0, S, integrate_pi=Q): ceil(S / chunk) library calls of four launches each;
  log_weights            HipSVI.log_weights(0, S) of the same build, as context - there is nothing on the parent commit to
                         compare with, so there is no threshold.

Recorded next to them: the share of targets with an unresolved pair (the quadrature rule's validity predicate) and the
median joint psis_k and marginal psis_k_marg (Q = 32) of the 300-step fit at 3 455 x 6, and the same on the
tests/golden/var_mini_screen.h5ad fixture.  How common unresolved pairs are on real screens has not been measured: the
synthetic screens and a six-target fixture are all there is here.
"""
import argparse
import json
import os
import sys
import time

import member_timing as mt

SHAPES = (("README shape", 3455, 6), ("metric shape", 50_000, 5))
FAMILY = "MixtureNormal"
NODES = (16, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "importance_marginal.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model.importance import importance_summary, marginal_summary
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    S = a.draws

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    def after_fit(eng):
        """Joint and marginal (Q = 32) summaries of S draws at the engine's parameters."""
        joint = eng.log_weights(0, S, seed=mt.SEED)
        marg = eng.log_weights(0, S, seed=mt.SEED, integrate_pi=32)
        k = importance_summary(joint["logw"], joint["mu"])["psis_k"]
        m = marginal_summary(marg["logw"], marg["mu"], marg["n_unresolved"])
        left_out = m["n_pairs_unresolved"] > 0
        km = m["psis_k_marg"][~left_out]
        return {"targets": int(k.numel()), "draws": S,
                "share_of_targets_unresolved": float(left_out.double().mean()),
                "psis_k_joint": {"median": float(k.median()), "share_above_0.7": float((k > 0.7).double().mean())},
                "psis_k_marg_of_resolved_targets": ({"median": float(km.median()),
                                                     "share_above_0.7": float((km > 0.7).double().mean())}
                                                    if km.numel() else None)}

    rows, fits = [], {}
    for name, guides, reps in SHAPES:
        host = make_sorting_variant_screen(guides, reps, seed=7)
        eng = engine.HipSVI(FAMILY, host.to(dev), num_steps=300)
        eng.run(300, seed=mt.SEED)
        torch.cuda.synchronize(dev)
        if guides == SHAPES[0][1]:
            fits[f"{guides} x {reps}, 300 steps"] = after_fit(eng)
            print(fits[f"{guides} x {reps}, 300 steps"], flush=True)
        calls = {None: lambda: eng.log_weights(0, S, seed=mt.SEED)}
        for Q in NODES:
            calls[Q] = lambda Q=Q: eng.log_weights(0, S, seed=mt.SEED, integrate_pi=Q)
        times = {k: [] for k in calls}
        for fn in calls.values():
            fn()  # first calls apart
        torch.cuda.synchronize(dev)
        for _ in range(a.reps):
            for k, fn in calls.items():  # the sides alternate
                times[k].append(timed(fn)[0])
        R, G = host.n_reps, host.n_guides
        chunk = max(1, min(S, eng.LOGW_PAIR_BYTES // (8 * R * G)))
        eng.invalidate_resume()
        eng.close()
        w = mt.stats(times[None])
        row = {"shape": name, "guides": guides, "replicates": reps, "conditions": int(host.n_condits), "family": FAMILY,
               "targets": int(host.n_targets), "draws": S, "likelihoods": 2, "draws_per_library_call": chunk,
               "library_calls": -(-S // chunk), "log_weights_wall_s": w,
               "log_weights_marginal_wall_s": {str(Q): mt.stats(times[Q]) for Q in NODES}}
        print(f"{name}: log_weights({S}) {mt.ms(w)}; integrate_pi "
              + "; ".join(f"Q = {Q}: {mt.ms(mt.stats(times[Q]))}" for Q in NODES), flush=True)
        rows.append(row)

    # the fixture screen, read as `bean run` reads it
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import get_parser

    var = os.path.join(mt.ROOT, "tests", "golden", "var_mini_screen.h5ad")
    import tempfile

    args = get_parser().parse_args(["run", "sorting", "variant", var, "-o", tempfile.mkdtemp(), "--sample-mask-col", ""])
    mini = cli_run.main(args, return_data=True)
    eng = engine.HipSVI(FAMILY, mini.to(dev), num_steps=300)
    eng.run(300, seed=mt.SEED)
    torch.cuda.synchronize(dev)
    fits["tests/golden/var_mini_screen.h5ad, 300 steps"] = after_fit(eng)
    print(fits["tests/golden/var_mini_screen.h5ad, 300 steps"], flush=True)
    eng.close()

    out = {"what": "per-target log importance weights with pi integrated out (bean_hip_log_weights_marginal, Q-node "
                   "quadrature per (draw, replicate, guide)) next to bean_hip_log_weights of the same build; one process, "
                   "wall time, the calls alternating; no parent figure exists, so no threshold",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "rows": rows, "after_a_fit": fits,
           "note": "how common unresolved pairs are on real screens has not been measured"}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
