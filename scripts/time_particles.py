"""P particles per step on one small screen: what the P draws cost, and what they buy.

    python scripts/time_particles.py [--reps 5] [--steps 2000] [--out profiles/particles_small_screens.json]

One process, this build.  For every P and every repetition three fits of the README shape run one after the other, so
drift of the box hits all of them: the single fit on the path it has always taken (`eng.run`, resumed windows), the
particle fit (`eng.run_particles`, P draws per step and one update) and the seed ensemble of K = P members
(`eng.run_ensemble`, P draws per step and P updates: the other way to spend the same draws).  A fit is `steps` SVI steps
in windows of 100, as run_inference steps them, between two device synchronisations; engines are built and warmed (200
untimed steps: graphs captured) outside the timed region.  The P = 1 row is the price of the particle step's two extra
launches.

Then the seed-to-seed spread, with README.md's metric: fits of 8 base seeds at P = 1 and at P = 8, and for every pair
of them the median over the strong variants (|mu_loc / mu_scale| > 2 in the first seed's fit) of |a - b| / |b| of mu_loc.
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

import member_timing as mt

GUIDES, REPS, FAMILY = 3455, 6, "MixtureNormal"  # 4 sort bins + bulk: make_sorting_variant_screen's default conditions
PS = (1, 2, 4, 8, 16)
SPREAD_PS = (1, 8)
BASE_SEEDS = tuple(101 + 17 * i for i in range(8))


def _windows(steps, step_window):
    for first in range(0, steps, mt.WINDOW):
        step_window(min(mt.WINDOW, steps - first), first)


def _reset(eng, start):
    for t, t0 in zip(_tensors(eng), start):
        t.copy_(t0)


def _tensors(eng):
    return [t for d in (eng.unconstrained, eng._m, eng._v) for t in d.values()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(mt.ROOT, "profiles", "particles_small_screens.json"))
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least five repetitions")
    sys.path.insert(0, mt.ROOT)
    import torch

    import bean_amd  # noqa: F401
    from bean_amd import engine
    from bean_amd.preprocessing.synthetic import make_sorting_variant_screen

    dev = torch.device("cuda:0")
    data = make_sorting_variant_screen(GUIDES, REPS, seed=7).to(dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def timed(eng, start, fit):
        _reset(eng, start)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fit()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(eng.loss_hist[..., :a.steps]).all())
        return dt

    rows = []
    single = engine.HipSVI(FAMILY, data, num_steps=a.steps)
    for P in PS:
        part = engine.HipSVI(FAMILY, data, num_steps=a.steps, n_particles=P)
        ens = engine.HipSVI(FAMILY, data, num_steps=a.steps, n_members=P)
        assert part._particles_native and single.dominant_kernel == "k_guide_wave2"
        seeds = [mt.SEED + j for j in range(P)]
        sides = [
            ("single", single, lambda n, first: single.run(n, seed=mt.SEED, first_step=first, resume=True)),
            ("particles", part, lambda n, first: part.run_particles(n, mt.SEED, first_step=first)),
            ("ensemble", ens, lambda n, first: ens.run_ensemble(n, seeds, first_step=first)),
        ]
        starts = {name: [t.clone() for t in _tensors(eng)] for name, eng, _ in sides}
        for name, eng, window in sides:  # untimed: graphs captured
            timed(eng, starts[name], lambda: _windows(200, window))
        times = {name: [] for name, _, _ in sides}
        for _ in range(a.reps):
            for name, eng, window in sides:
                times[name].append(timed(eng, starts[name], lambda: _windows(a.steps, window)))
        s, p, e = (mt.stats(times[name]) for name in ("single", "particles", "ensemble"))
        rows.append({
            "guides": GUIDES, "replicates": REPS, "family": FAMILY, "particles": P, "steps": a.steps,
            "single_fit_wall_s": s, "particles_wall_s": p, "ensemble_of_p_members_wall_s": e,
            "single_fit_us_per_step": s["median"] / a.steps * 1e6, "particles_us_per_step": p["median"] / a.steps * 1e6,
            "ensemble_us_per_step": e["median"] / a.steps * 1e6,
            "particles_over_single": p["median"] / s["median"], "particles_over_ensemble": p["median"] / e["median"],
            "waves_per_simd": mt.waves_per_simd(GUIDES, REPS, int(single.T), P, cus),
        })
        print(f"P={P:2d}  single {mt.ms(s)}  particles {mt.ms(p)}  ensemble of {P} {mt.ms(e)}  "
              f"particles / single x{rows[-1]['particles_over_single']:.2f}", flush=True)
        part.close()
        ens.close()
    single.close()

    spread = []
    for P in SPREAD_PS:
        eng = engine.HipSVI(FAMILY, data, num_steps=a.steps, n_particles=P)
        start = [t.clone() for t in _tensors(eng)]
        fits = []
        for seed in BASE_SEEDS:
            _reset(eng, start)
            _windows(a.steps, lambda n, first: eng.run_particles(n, seed, first_step=first))
            c = eng.constrained()
            fits.append((c["mu_loc"].flatten().double().cpu(), c["mu_scale"].flatten().double().cpu()))
        eng.close()
        strong = (fits[0][0] / fits[0][1]).abs() > 2.0
        pairs = [float((((x - y).abs() / y.abs())[strong]).median())
                 for (x, _), (y, _) in itertools.combinations(fits, 2)]
        spread.append({"particles": P, "base_seeds": list(BASE_SEEDS), "n_strong": int(strong.sum()), "pairs": len(pairs),
                       "median_rel_distance_mu_loc": {"median_over_pairs": statistics.median(pairs), "min": min(pairs),
                                                      "max": max(pairs)}})
        print(f"P={P:2d}  seed-to-seed distance of mu_loc on {int(strong.sum())} strong variants: median "
              f"{statistics.median(pairs) * 100:.2f} % over {len(pairs)} pairs [{min(pairs) * 100:.2f}, {max(pairs) * 100:.2f}]",
              flush=True)

    out = {"what": "P particles per step (bean_hip_svi_run_particles) against the single fit and the seed ensemble of "
                   "K = P, one process, wall time per fit; seed-to-seed spread of mu_loc at P = 1 and P = 8",
           "steps_per_fit": a.steps, "window": mt.WINDOW, "repetitions": a.reps, "compute_units": cus, "rows": rows,
           "seed_to_seed_spread": spread}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
