"""What the grid posterior of (mu, sd) per target costs, and what it says after a 300-step fit:

    python scripts/time_grid_posterior.py [--reps 5] [--draws 1024] [--out profiles/grid_posterior.json]

One process, wall time, `--reps` (at least five) repetitions, median [min, max]; per shape (3 455 x 6 and 50 000 x 5,
MixtureNormal, both likelihoods, a 300-step fit):

  grid_posterior   model/grid_posterior.py::grid_posterior(engine) with its defaults: five 17 x 17 zoom passes (16
                   quadrature nodes) and the 41 x 21 grid (32), then the null line (five passes of 17 and 21 nodes) -
                   2 412 node evaluations per target; host synchronisation only at the end;
  log_weights      HipSVI.log_weights(0, S, integrate_pi=32) of the same build, S = 1 024 draws, alternating with it, as
                   context - there is nothing on the parent commit to compare with, so there is no threshold.

Recorded next to them: the library calls a grid_posterior makes, the share of targets that are grid_ok, left out as
unresolved, and the median of the fitted mu_sd over mu_sd_grid on the others.
"""
import argparse
import json
import os
import sys
import time

import member_timing as mt

SHAPES = (("README shape", 3455, 6), ("metric shape", 50_000, 5))
FAMILY = "MixtureNormal"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "grid_posterior.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.model.grid_posterior import grid_posterior
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
        eng = engine.HipSVI(FAMILY, host.to(dev), num_steps=300)
        eng.run(300, seed=mt.SEED)
        torch.cuda.synchronize(dev)
        n_calls = [0]
        inner = eng.marginal_grid

        def counted(*args, **kw):
            n_calls[0] += 1
            return inner(*args, **kw)

        eng.marginal_grid = counted
        res = grid_posterior(eng)  # first calls apart
        eng.marginal_grid = inner
        eng.log_weights(0, S, seed=mt.SEED, integrate_pi=32)
        torch.cuda.synchronize(dev)
        calls = {"grid": lambda: grid_posterior(eng), "logw": lambda: eng.log_weights(0, S, seed=mt.SEED, integrate_pi=32)}
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():  # the sides alternate
                times[k].append(timed(fn)[0])
        left_out = res["n_pairs_unresolved"] > 0
        ok = res["grid_ok"]
        fitted_sd = eng.unconstrained["mu_scale"].detach().double().reshape(-1).exp()
        ratio = (fitted_sd / res["mu_sd_grid"])[ok]
        shift = ((eng.unconstrained["mu_loc"].detach().double().reshape(-1) - res["mu_grid"]) / res["mu_sd_grid"])[ok]
        R, G = host.n_reps, host.n_guides
        eng.close()
        g, w = mt.stats(times["grid"]), mt.stats(times["logw"])
        row = {"shape": name, "guides": guides, "replicates": reps, "conditions": int(host.n_condits), "family": FAMILY,
               "targets": int(host.n_targets), "likelihoods": 2, "node_evaluations_per_target": 5 * 17 * 17 + 41 * 21 + 5 * 17 + 21,
               "marginal_grid_calls": n_calls[0],
               "nodes_per_library_call_at_most": max(1, min(4096, eng.LOGW_PAIR_BYTES // (8 * R * G))),
               "grid_posterior_wall_s": g, "log_weights_marginal_q32_wall_s": w, "draws": S,
               "share_of_targets_grid_ok": float(ok.double().mean()),
               "share_of_targets_unresolved": float(left_out.double().mean()),
               "share_of_targets_not_settled": float((~ok & ~left_out).double().mean()),
               "median_mu_sd_over_mu_sd_grid": float(ratio.median()) if ratio.numel() else None,
               "median_abs_mu_loc_less_mu_grid_in_sd": float(shift.abs().median()) if shift.numel() else None}
        print(f"{name}: grid_posterior {mt.ms(g)} in {n_calls[0]} marginal_grid calls; log_weights({S}, integrate_pi=32) "
              f"{mt.ms(w)}; grid_ok {row['share_of_targets_grid_ok']:.3f}, unresolved "
              f"{row['share_of_targets_unresolved']:.3f}, mu_sd / mu_sd_grid {row['median_mu_sd_over_mu_sd_grid']}", flush=True)
        rows.append(row)

    out = {"what": "grid posterior of (mu, sd) per target (bean_hip_marginal_grid through grid_posterior's defaults) next "
                   "to HipSVI.log_weights(integrate_pi=32) of the same build; one process, wall time, the calls "
                   "alternating; no parent figure exists, so no threshold",
           "repetitions": a.reps, "compute_units": cus, "seed": mt.SEED, "rows": rows}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
