"""What the per-target importance weights cost, against the only route the parent commit offers to log p - log q of a
draw: bean_hip_elbo_grad, five launches with the whole backward pass, one number for the whole screen.

    python scripts/time_importance.py [--reps 5] [--draws 1024] [--out profiles/importance_check.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_importance.py --trace-run
    python scripts/time_importance.py --merge-trace DIR [--out profiles/importance_check.json]

One process, this build (the protocol of time_bootstrap.py; stats / gain / ms of member_timing.py).  For each shape - the
README shape, 3 455 guides x 6 replicates, and the metric shape, 50 000 x 5 - MixtureNormal, both likelihoods, an engine
fitted for 300 steps.  After one untimed pass of every side, `reps` times, the sides one after the other, each between two
device synchronisations:

  log_weights       HipSVI.log_weights(0, S): ceil(S / chunk) library calls of three launches each (the chunk keeps the pair
                    plane at or below 256 MiB), then importance_summary of the result (timed apart: `summary_wall_s`);
  elbo_grad         S HipSVI.elbo_grad(step=d) calls, as a user of the parent reaches them: each synchronises and copies
                    its gradients;
  elbo_grad_queued  S bean_hip_elbo_grad calls enqueued through the library, one synchronisation at the end - the floor of
                    that route (no per-call host work beyond the five launches).

The warm-up compares - sum_t logw[d, t] with elbo_grad's loss for d = 0 (1e-9 relative).  Kernel times come from a run of
its own under rocprofv3 (`--trace-run`: one log_weights call of S draws and 32 elbo_grad calls per shape, nothing timed),
merged into the JSON by `--merge-trace`.  Nothing is promised: the figures are what they are.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import member_timing as mt

SHAPES = (("README shape", 3455, 6), ("metric shape", 50_000, 5))
FAMILY = "MixtureNormal"
KERNELS = ("k_logw_consts", "k_logw_pairs", "k_logw_targets", "k_guide_wave2", "k_param", "k_set_step", "k_loss_finalize")


def merge_trace(directory, out_path):
    rows = []
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r.get("Name", "")
                if any(k in name for k in KERNELS):
                    rows.append({"kernel": name, "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                                 "average_ns": float(r["AverageNs"]), "min_ns": int(float(r["MinNs"])),
                                 "max_ns": int(float(r["MaxNs"]))})
    if not rows:
        sys.exit(f"no kernel_stats.csv with the kernels of this script under {directory}")
    with open(out_path) as fh:
        out = json.load(fh)
    out["kernel_trace"] = {"how": "rocprofv3 --kernel-trace --stats, a run of its own (--trace-run): per shape one "
                                  "log_weights call of the draws above and 32 elbo_grad calls; both shapes in one trace, "
                                  "so a kernel's row covers both",
                           "rows": rows}
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"merged {len(rows)} kernel rows into {out_path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge-trace", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "importance_check.json"))
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.merge_trace, a.out)
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model.importance import importance_summary
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

    rows = []
    for name, guides, reps in SHAPES:
        host = make_sorting_variant_screen(guides, reps, seed=7)
        eng = engine.HipSVI(FAMILY, host.to(dev), num_steps=max(S, 300))
        eng.run(300, seed=mt.SEED)
        torch.cuda.synchronize(dev)

        def weights():
            return eng.log_weights(0, S, seed=mt.SEED)

        def grads():
            return [eng.elbo_grad(step=d, seed=mt.SEED, loss_index=d)[0] for d in range(S)]

        def queued():
            with eng._on_stream():
                for d in range(S):
                    eng._check(eng.lib.bean_hip_elbo_grad(eng._h, mt.SEED, d, d, eng._sptr()), "elbo_grad")

        if a.trace_run:
            weights()
            for d in range(32):
                eng.elbo_grad(step=d, seed=mt.SEED, loss_index=d)
            torch.cuda.synchronize(dev)
            eng.close()
            continue
        out = weights()
        loss0 = eng.elbo_grad(step=0, seed=mt.SEED)[0]
        rel = abs(-float(out["logw"][0].sum()) - loss0) / abs(loss0)
        assert rel <= 1e-9, f"- sum logw differs from elbo_grad's loss: relative {rel:.3e}"
        queued()
        torch.cuda.synchronize(dev)
        t_w, t_g, t_q, t_s = [], [], [], []
        for _ in range(a.reps):
            dt, out = timed(weights)
            t_w.append(dt)
            t_s.append(timed(lambda: importance_summary(out["logw"], out["mu"]))[0])
            t_g.append(timed(grads)[0])
            t_q.append(timed(queued)[0])
        k = importance_summary(out["logw"], out["mu"])["psis_k"]
        R, G = host.n_reps, host.n_guides
        chunk = max(1, min(S, eng.LOGW_PAIR_BYTES // (8 * R * G)))
        tiles = (guides + 63) // 64
        waves = (tiles + 7) // 8 * 8 * reps
        eng.invalidate_resume()
        eng.close()
        w, g, q, s = mt.stats(t_w), mt.stats(t_g), mt.stats(t_q), mt.stats(t_s)
        row = {"shape": name, "guides": guides, "replicates": reps, "conditions": int(host.n_condits), "family": FAMILY,
               "targets": int(host.n_targets), "draws": S, "likelihoods": 2, "draws_per_library_call": chunk,
               "library_calls": -(-S // chunk), "log_weights_wall_s": w, "summary_wall_s": s, "elbo_grad_wall_s": g,
               "elbo_grad_queued_wall_s": q, "against_elbo_grad": mt.gain(w, g), "against_elbo_grad_queued": mt.gain(w, q),
               "relative_difference_to_elbo_grad_loss_draw_0": rel,
               "waves_per_simd": {"k_logw_pairs": waves * chunk / (4 * cus), "k_guide_wave2": waves / (4 * cus)},
               "psis_k_after_300_steps": {"median": float(k.median()), "share_above_0.7": float((k > 0.7).double().mean())}}
        print(f"{name}: log_weights({S}) {mt.ms(w)} + summary {mt.ms(s)};  {S} x elbo_grad {mt.ms(g)} "
              f"(x{row['against_elbo_grad']['speedup_median']:.2f}), queued {mt.ms(q)} "
              f"(x{row['against_elbo_grad_queued']['speedup_median']:.2f}); psis_k median {float(k.median()):.2f}", flush=True)
        rows.append(row)
    if a.trace_run:
        return
    out = {"what": "per-target log importance weights of S draws in ceil(S / chunk) bean_hip_log_weights calls against S "
                   "bean_hip_elbo_grad calls (through the engine, and enqueued with one synchronisation); one process, wall "
                   "time; elbo_grad returns one number per draw for the whole screen, log_weights one per (draw, target)",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
