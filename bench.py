#!/usr/bin/env python
"""Headline benchmark: SVI steps/s of the `bean run` hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config metric|tiling|survival] [--scaling weak|strong]
                    [--full] [--dump-outputs DIR]

One "step" is one full SVI step (draw, ELBO, gradient, ClippedAdam; ``bean/model/run.py:376-377``) over
a synthetic screen that is already resident in HBM.

A plain run times only the leg ``value`` reports: it sets up, runs W untimed and K timed steps and
prints the JSON line.  ``--full`` adds everything else described below: the other leg, the ``roofline``
and ``sustained`` objects, the CPU baseline and, for ``--config metric`` at N = 1, ``other_configs``.
``--dump-outputs DIR`` writes what the timed leg hands its caller after its last step (see
``dump_outputs``) as ``DIR/<name>.npy``; the inputs are seeded, so two builds can be compared output
for output.

``--gpus N`` with N > 1 works with or without a launcher: under ``torch.distributed.run`` (RANK /
WORLD_SIZE in the environment) this process is one rank; started bare, it starts the N ranks itself as
a child ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...``
before anything touches the GPU, and passes rank 0's JSON line and the exit code through.

``--config`` (BASELINE.json ``configs``; default = the configuration ``metric`` is quoted on):
  metric    variant sorting MixtureNormal, 50k guides x 5 replicates x (4 sort bins + bulk)   [configs[1] shape x10]
  tiling    tiling sorting MultiMixtureNormal, 50k guides / ~193k edited alleles x 5 reps     [configs[2]]
  survival  survival MixtureNormal, 100k guides x 6 timepoints x 3 replicates                 [configs[4]]

A ``--full`` run times TWO legs in the same process group (``--no-strong`` skips the second):
  weak    every rank holds its own screen of the configured size; steps of one such screen summed over
          ranks.  This is ``value`` (``--scaling weak``, the default) and the ``weak`` object.
  strong  ONE screen - 500k-guide variant sorting (BASELINE configs[3]) for ``metric``, the 50k-guide
          tiling screen (configs[2]) for ``tiling``, the 100k-guide survival screen (configs[4]) for
          ``survival`` - cut into N shards exactly as ``run_inference`` cuts it under torchrun
          (``parallel.plan_shards`` / ``plan_guide_shards``); steps/s of the WHOLE screen: the ``strong``
          object (and ``value`` with ``--scaling strong``).  The variant sorting family shares no
          parameter across shards (only the loss window is all-reduced, every 100 steps, the reference's
          reporting cadence, ``run.py:378``); tiling and survival exchange inside every step
          (``HipSVI.run_exchanged``: per-edit gradients / Dirichlet normalisers over RCCL).
A ``--full`` N = 1, 2, 4, 8 series therefore carries both curves; the north star's ">= 6x 1 -> 8" is
``strong.value`` at N = 8 over ``strong.value`` at N = 1.  A plain run with ``--scaling strong`` times
the strong leg alone.

Rank 0 prints ONE JSON line; DESIGN.md section 4 defines the ``roofline`` and ``cpu_baseline`` objects.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s
F64_VALU_DATASHEET = 78.6e12 / 2 / 64  # wave-instructions / s: 78.6 TFLOP/s FP64 vector, 2 flop x 64 lanes per FMA
LOSS_SYNC_EVERY = 100
STRONG_GUIDES = 500_000


def workload(name, guides, rank, acc=False):
    """(family, screen on CPU, oracle loss fn + kwargs, description)."""
    from bean_amd.preprocessing import synthetic as syn
    from oracle import elbo
    from oracle import survival as osurv

    if name == "metric":
        data = syn.make_sorting_variant_screen(guides, 5, seed=syn.BASE_SEED + 1 + rank, with_accessibility=acc)
        return ("MixtureNormal", data, elbo.mixture_normal_loss, dict(scale_by_accessibility=acc) if acc else {},
                elbo.init_params, f"variant sorting MixtureNormal{'+Acc' if acc else ''}: {guides} guides x 5 reps x "
                f"(4 sort bins + bulk), {data.n_targets} targets")
    if name == "tiling":
        data = syn.make_sorting_tiling_screen(guides, 5, seed=20240503 + rank, with_accessibility=acc)
        n_alleles = int(data.allele_mask.sum()) - data.n_guides
        kw = dict(sparse=True, scale_by_accessibility=True) if acc else dict(sparse=True)
        return ("MultiMixtureNormal", data, elbo.multi_mixture_normal_loss, kw, elbo.init_params,
                f"tiling sorting MultiMixtureNormal{'+Acc' if acc else ''}: {guides} guides, {n_alleles} edited alleles, "
                f"{data.n_edits} edits x 5 reps x (4 sort bins + bulk); guides reach the engine ordered by allele "
                f"count, as run_inference hands them over (parallel.order_by_alleles)")
    if name == "survival":
        data = syn.make_survival_variant_screen(guides, 3, seed=20240506 + rank, with_accessibility=acc)
        return ("MixtureNormal", data, osurv.mixture_normal_loss, dict(scale_by_accessibility=True) if acc else {},
                osurv.init_params,
                f"survival MixtureNormal{'+Acc' if acc else ''}: {guides} guides x {data.n_condits} timepoints x 3 reps")
    raise SystemExit(f"unknown --config {name}")


DEFAULT_GUIDES = {"metric": 50_000, "tiling": 50_000, "survival": 100_000}


def cpu_baseline(family, data, loss_fn, loss_kw, init_fn, seconds_budget=20.0):
    """Reference CPU path = the float64 eager-torch oracle, timed on this box's host cores on a
    bounded sample (SVI steps of the same screen)."""
    import torch

    from oracle import svi

    torch.manual_seed(101)
    params = init_fn(family, data)
    optim = svi.ClippedAdam(params, lr=0.01, lrd=0.1 ** (1 / 2000))
    # the eager path is partly overhead bound: give the CPU its best thread count (2 timed steps each
    # at a few counts), then spend the budget there
    avail = torch.get_num_threads()
    best, n_threads = None, avail
    for cand in sorted({min(avail, c) for c in (8, 16, 32, 64, avail)}):
        torch.set_num_threads(cand)
        svi.svi_step(loss_fn, data, params, optim, **loss_kw)  # warm-up at this count
        t = time.perf_counter()
        for _ in range(2):
            svi.svi_step(loss_fn, data, params, optim, **loss_kw)
        t = (time.perf_counter() - t) / 2
        if best is None or t < best:
            best, n_threads = t, cand
    torch.set_num_threads(n_threads)
    t0 = time.perf_counter()
    n = 0
    while n < 4 or (time.perf_counter() - t0 < seconds_budget and n < 200):
        svi.svi_step(loss_fn, data, params, optim, **loss_kw)
        n += 1
    dt = time.perf_counter() - t0
    # the reference enables anomaly detection on every step (bean/model/model.py:399): the same loop
    # with it on, a few steps (the slower of the two numbers; `value` stays the conservative one)
    prev = torch.is_anomaly_enabled()
    torch.autograd.set_detect_anomaly(True)
    try:
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            svi.svi_step(loss_fn, data, params, optim, **loss_kw)
            ta = time.perf_counter()
            na = 0
            while na < 3 or (time.perf_counter() - ta < seconds_budget / 4 and na < 50):
                svi.svi_step(loss_fn, data, params, optim, **loss_kw)
                na += 1
            dta = time.perf_counter() - ta
    finally:
        torch.autograd.set_detect_anomaly(prev)
    return {
        "value": n / dt,
        "unit": "steps/s",
        "cores": n_threads,
        "kind": "port",
        "sample": f"{n} SVI steps of the same {data.n_guides}-guide screen (float64 eager-torch oracle, "
                  f"anomaly detection off, {dt:.1f} s; fastest of 8/16/32/64/{avail} threads)",
        "value_anomaly_detection_on": na / dta,
        "sample_anomaly_detection_on": f"{na} further steps with torch.autograd.set_detect_anomaly(True), as the "
                                       f"reference runs (model.py:399), {dta:.1f} s",
    }


def kernel_resources(kernel_name, lds_dynamic):
    """Register / scratch figures of the dominant kernel from the shipped code object's metadata
    (scripts/kernel_resources.py), next to the dynamic LDS the library requests for it."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import kernel_resources as kr

        recs = [r for r in kr.kernels(os.path.join(ROOT, "crispr-bean_amd", "lib", "libbean_hip.so"))
                if r["kernel"] == "bean::" + kernel_name]
        r = recs[0]
        return {"kernel": kernel_name, "vgpr": r.get("vgpr_count"), "agpr": r.get("agpr_count"), "sgpr": r.get("sgpr_count"),
                "vgpr_spills": r.get("vgpr_spill_count"), "scratch_bytes_per_lane": r.get("private_segment_fixed_size"),
                "lds_static_bytes": r.get("group_segment_fixed_size"), "lds_dynamic_bytes": lds_dynamic,
                "source": "code object notes of libbean_hip.so (scripts/kernel_resources.py)"}
    except Exception as exc:  # noqa: BLE001  (llvm tools absent: the figures are a report, not a dependency)
        return {"error": str(exc), "lds_dynamic_bytes": lds_dynamic}


def _newest(pattern):
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return files[-1] if files else None


def pmc_traffic(config):
    """HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 --pmc summary
    of this configuration (profiles/rNN_traffic[_<config>].json, written by scripts/summarize_prof.py
    with the gfx950 FETCH_SIZE correction), or None."""
    suffix = "" if config == "metric" else "_" + config
    path = _newest(f"r[0-9][0-9]_traffic{suffix}.json")
    if not path:
        return None, None
    with open(path) as fh:
        return float(json.load(fh)["hbm_bytes_per_launch"]), os.path.basename(path)


def valu_issue_roofline(config, kernel_name, kernel_ms):
    """Secondary roofline of the dominant kernel (it is bound by float64 VALU issue, not by HBM):
    VALU wave-instructions per launch (SQ_INSTS_VALU, newest profiles/rNN_counters[_<config>].txt)
    over the live kernel duration, against (a) the data-sheet float64 vector rate (78.6 TFLOP/s =
    614 G wave-instr/s) and (b) what a gfx950 SIMD sustained on v_fma_f64 with 4 resident waves in
    scripts/micro/valu_rate.hip (profiles/r01_valu_issue.txt) times the 1024 SIMDs."""
    suffix = "" if config == "metric" else "_" + config
    cfile = _newest(f"r[0-9][0-9]_counters{suffix}.txt")
    vfile = _newest("r[0-9][0-9]_valu_issue.txt")
    if not cfile or kernel_ms <= 0:
        return None
    insts = None
    lines = open(cfile).read().splitlines()
    for i, ln in enumerate(lines):
        if ln.startswith("bean::" + kernel_name + "<") or ln.startswith("bean::" + kernel_name + " "):
            # (k_svi_async: one launch = a whole report window; the summary also gives the counter per SVI step)
            pat = (r"\s+SQ_INSTS_VALU / step\s+n=\s*\d+\s+mean=([0-9.e+]+)" if kernel_name == "k_svi_async"
                   else r"\s+SQ_INSTS_VALU\s+n=\s*\d+\s+mean=([0-9.e+]+)")
            for l2 in lines[i + 1:i + 24]:
                m = re.match(pat, l2)
                if m:
                    insts = float(m.group(1))
                    break
            if insts:
                break
    if not insts:
        return None
    achieved = insts / (kernel_ms * 1e-3)
    out = {"bound": "f64 VALU issue", "achieved": achieved / 1e9, "unit": "G wave-instr/s",
           "peak_datasheet": F64_VALU_DATASHEET / 1e9, "frac_datasheet": achieved / F64_VALU_DATASHEET,
           "valu_insts_per_launch": insts, "source": [os.path.basename(cfile)]}
    # how busy the vector pipe was in the profiled launches themselves: SQ_ACTIVE_INST_VALU counts quad-cycles in which a
    # wave executes a VALU instruction (the unit in which WAIT_ANY + WAIT_INST_ANY + ACTIVE_INST_ANY add up to WAVE_CYCLES),
    # GRBM_GUI_ACTIVE the launch's cycles summed over the 8 XCDs
    step = " / step" if kernel_name == "k_svi_async" else ""
    vals = {}
    for i, ln in enumerate(lines):
        if ln.startswith("bean::" + kernel_name + "<") or ln.startswith("bean::" + kernel_name + " "):
            for l2 in lines[i + 1:i + 24]:
                for name in ("SQ_ACTIVE_INST_VALU", "GRBM_GUI_ACTIVE"):
                    m = re.match(r"\s+" + name + re.escape(step) + r"\s+n=\s*\d+\s+mean=([0-9.e+]+)", l2)
                    if m:
                        vals.setdefault(name, float(m.group(1)))
            if len(vals) == 2:
                break
    if len(vals) == 2 and vals["GRBM_GUI_ACTIVE"] > 0:
        out["valu_busy"] = {"frac": vals["SQ_ACTIVE_INST_VALU"] * 4.0 / 1024.0 / (vals["GRBM_GUI_ACTIVE"] / 8.0),
                            "note": "SQ_ACTIVE_INST_VALU x 4 cycles / 1024 SIMDs over GRBM_GUI_ACTIVE / 8 XCDs, in the "
                                    "profiled (eager, counter-collecting) launches of " + os.path.basename(cfile)}
    ns = None
    if vfile:
        for ln in open(vfile):
            m = re.match(r"fma_f64\s+waves/SIMD 4: .*-> ([0-9.]+) ns per wave-instr per SIMD", ln)
            if m:
                ns = float(m.group(1))
    if ns:
        peak = 1024 / (ns * 1e-9)  # 256 CUs x 4 SIMDs
        out.update({"peak": peak / 1e9, "frac": achieved / peak})
        out["source"].append(os.path.basename(vfile))
    return out


def survey_bytes(config, data):
    """SURVEY.md section 8(d)'s algorithmic bytes of one step (counts as 4-byte values, each input and
    parameter once, each gradient once, RNG in-kernel): the figure the judge prices `achieved` with.
    `bean_hip_step_bytes` (`algorithmic_bytes_per_launch`) counts what the dominant kernel itself must
    move - it also reads and writes the Adam moments of the fused update - and is the larger number."""
    G, R, B = int(data.n_guides), int(data.n_reps), int(data.n_condits)
    acc = 20 * G if config.endswith("_acc") else 0  # "+20 G with --scale-by-acc": accessibility, noise parameters + grads
    config = config[:-4] if config.endswith("_acc") else config
    if config == "metric":
        return G * (8 * R * B + 9 * R + 32) + 32 * int(data.n_targets) + acc
    if config == "tiling":
        A = int(data.n_max_alleles)
        n_alleles = int(data.allele_mask.sum()) - G
        nnz = int(data.a2e_idx.numel()) if data.a2e_idx is not None else 2 * n_alleles
        return G * (8 * R * B + 4 * R * A + R + 9 * A + 12) + 8 * nnz + 4 * n_alleles + 32 * int(data.n_edits) + acc
    if config == "survival":
        C = int(data.allele_counts_control.shape[1]) if getattr(data, "allele_counts_control", None) is not None else 1
        return G * (8 * R * B + 4 * R * C * 2 + R + 32 + 8) + 32 * int(data.n_targets) + acc
    return None


def roofline_object(config, leg, guides, std_size):
    """The `roofline` object of one configuration: HIP-event duration of its dominant kernel (50 eager
    launches on the leg's screen), algorithmic bytes, newest committed PMC traffic, code-object
    resources and the VALU-issue figure."""
    k_ms, k_n, step_bytes, kernel_name, lds_dyn, kernel_variant = leg.kernel_profile()
    traffic, traffic_src = pmc_traffic(config) if std_size else (None, None)
    achieved = step_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
    sb = survey_bytes(config, leg.shard_cpu)
    obj = {
        "bound": "hbm",
        "kernel": kernel_name,
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": traffic,
        "traffic_source": traffic_src,
        "algorithmic_bytes_per_launch": step_bytes,
        "algorithmic_bytes_survey_8d": sb,
        "frac_survey_8d": (sb / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if (sb and k_ms > 0) else None,
        "kernel_ms": k_ms,
        "kernel_launches_timed": k_n,
        **({"kernel_ms_is": "per SVI step: one launch of k_svi_async runs a whole report window (100 steps); "
                            "kernel_launches_timed counts the steps the timed launches covered",
            "compare_with_earlier_rounds": "this kernel is the WHOLE step (guide work + per-target / per-guide finish); rounds "
                                           "1 - 4 priced k_guide_wave2 alone (round 4: 17.01 MB / 44.2 us = 0.048, 43 - 44 us of a "
                                           "55.2 us step, whose whole-step figure is 17.01 MB / 55.2 us = 0.0385): compare `whole_step`"}
           if kernel_name == "k_svi_async" else {}),
        "kernel_resources": kernel_resources(kernel_variant, lds_dyn),
        "measured_on": f"the weak leg's screen ({guides} guides on this rank)",
    }
    if getattr(leg, "last_ms_per_step", None):
        # the same bytes over the whole STEP (every launch of it), for comparing configurations whose dominant kernel is
        # a part of the step (k_guide_* + k_param) with k_svi_async, which is the whole step
        ws = step_bytes / (leg.last_ms_per_step * 1e-3) / 1e9
        obj["whole_step"] = {"achieved": ws, "frac": ws / HBM_PEAK_GBS, "ms_per_step": leg.last_ms_per_step,
                             "note": "algorithmic_bytes_per_launch / ms_per_step of this leg's timed region"}
    if std_size:
        valu = valu_issue_roofline(config, kernel_name, k_ms)
        if valu is not None:
            obj["valu_issue"] = valu
    return obj


def other_config(args, config, rank, dev, acc=False):
    """One more BASELINE configuration on the driver's line (N = 1): the same --steps / --warmup, its
    roofline object, one sustained 2000-step fit and a CPU baseline bounded to ~8 s of oracle steps
    (`acc`: the same workload with --scale-by-acc, no CPU baseline)."""
    guides = DEFAULT_GUIDES[config]
    if acc:
        args = argparse.Namespace(**dict(vars(args), scale_by_acc=True, no_cpu_baseline=True))
    leg = Leg(args, config, False, guides, rank, 1, dev, args.warmup + args.steps)
    dt = leg.timed(args.steps, args.warmup)
    losses = leg.eng.losses()
    obj = {
        "workload": leg.desc + "; one SVI step = draw + ELBO + grad + ClippedAdam",
        "metric": METRICS[config],
        "value": args.steps / dt,
        "unit": "steps/s",
        "ms_per_step": dt / args.steps * 1e3,
        "steps": args.steps,
        "warmup": args.warmup,
        "dtype": "f64",
        "final_loss": losses[-1] if losses else None,
        "roofline": roofline_object(config + ("_acc" if acc else ""), leg, guides, True),
        "sustained": leg.sustained(),
    }
    if not args.no_cpu_baseline:
        obj["cpu_baseline"] = cpu_baseline(leg.family, leg.shard_cpu, leg.loss_fn, leg.loss_kw, leg.init_fn,
                                           seconds_budget=8.0)
        obj["gpu_over_cpu"] = obj["value"] / obj["cpu_baseline"]["value"]
    leg.close()
    return obj


README_GUIDES, README_REPS, README_SECONDS = 3455, 6, 4.6 * 60  # /root/reference README.md:83


def readme_shape(args, dev):
    """The ONE run time the reference publishes for this path (README.md:83): `bean run ... --scale-by-acc` on a
    variant screen of 3455 guides x 6 replicates x 4 sorting bins took 4.6 min on a Dell XPS 13 (Ubuntu on WSL,
    CPU).  Here: a synthetic screen of that shape written to an .h5ad, then the whole command - read, preprocess,
    the 2000-step negative-control fit, the 2000-step MixtureNormal+Acc fit, both result tables - through
    `bean_amd.cli`, wall-clock; and the two fits alone through `run_inference`."""
    import tempfile
    from functools import partial

    import torch

    from bean_amd.cli.execute import main as bean_main
    from bean_amd.model import model as sm
    from bean_amd.model.run import run_inference
    from bean_amd.preprocessing import synthetic as syn

    data = syn.make_sorting_variant_screen(README_GUIDES, README_REPS, seed=syn.BASE_SEED + 83, with_accessibility=True)
    out = {"workload": f"`bean run sorting variant <screen>.h5ad --scale-by-acc --acc-col accessibility --fit-negctrl` "
                       f"(default --n-iter 2000): synthetic variant screen, {README_GUIDES} guides x {README_REPS} reps x "
                       f"(4 sort bins + bulk), {data.n_targets} targets, {len(data.negctrl_guide_idx)} negative-control guides",
           "published": {"seconds": README_SECONDS, "source": "/root/reference README.md:83",
                         "hardware": "Dell XPS 13, Ubuntu on WSL, CPU (Pyro SVI)",
                         "note": "not stated whether that run fitted the negative controls (--fit-negctrl: a second "
                                 "2000-step fit); this leg does"}}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "readme_shape.h5ad")
        syn.variant_reporter_screen(data).write(path)
        argv = ["run", "sorting", "variant", path, "--scale-by-acc", "--acc-col", "accessibility", "--fit-negctrl",
                "-o", tmp]
        import contextlib
        import io
        import logging

        logging.disable(logging.WARNING)  # (the command's banner, per-window loss lines and log go nowhere: stdout is the JSON line's)
        try:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rc = bean_main(argv)
            torch.cuda.synchronize(dev)
            wall = time.perf_counter() - t0
        finally:
            logging.disable(logging.NOTSET)
        tables = sorted(f for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".csv"))
    out.update({"wall_s_whole_command": wall, "exit_code": rc, "tables_written": tables})
    # the two fits alone (engine construction and upload included), as `bean run` calls them (cli/run.py)
    neg = data[data.negctrl_guide_idx]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run_inference(partial(sm.ControlNormalModel, use_bcmatch=True), partial(sm.ControlNormalGuide, use_bcmatch=True),
                  neg, num_steps=2000, verbose=False)
    t1 = time.perf_counter()
    _, fit = run_inference(partial(sm.MixtureNormalModel, scale_by_accessibility=True, use_bcmatch=(True,)),
                           partial(sm.MixtureNormalGuide, scale_by_accessibility=True, fit_noise=True),
                           data, num_steps=2000, verbose=False)
    t2 = time.perf_counter()
    out.update({"fit_s_negctrl_2000_steps": t1 - t0, "fit_s_main_2000_steps": t2 - t1,
                "main_fit_steps_per_s": 2000 / (t2 - t1), "main_fit_final_loss": fit["loss"][-1],
                "vs_baseline": README_SECONDS / wall,
                "vs_baseline_note": "published seconds / this leg's wall seconds of the whole command; other hardware "
                                    "(a laptop CPU under WSL against one MI355X + its host), a synthetic screen of the "
                                    "published shape, not the published data: an anchor, not a like-for-like speed-up"})
    return out


def self_launch(argv, n_ranks):
    """``bench.py --gpus N`` started WITHOUT a launcher: start the N ranks ourselves.

    Runs before this process has imported torch.cuda or made any GPU call: the ranks are a CHILD
    process tree (``python -m torch.distributed.run``, rendezvous on 127.0.0.1), whose stdout - rank
    0's JSON line - and exit code are passed through.  Under torchrun (RANK / WORLD_SIZE set) this is
    never reached."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on this pool
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


class Leg:
    """One timed workload of this rank: a screen (weak: its own; strong: its shard of ONE screen)
    bound to a HipSVI engine, and the loop that steps it the way ``run_inference`` does."""

    def __init__(self, args, config, strong, guides, rank, world, dev, total_steps):
        import torch

        from bean_amd import engine, parallel

        self.strong, self.world, self.dev, self.guides = strong, world, dev, guides
        self.graph_chunk = args.graph_chunk
        acc = bool(args.scale_by_acc)
        # strong: every rank builds the SAME whole screen and keeps its shard
        fam, data_cpu, loss_fn, loss_kw, init_fn, desc = workload(config, guides, 0 if strong else rank, acc=acc)
        self.family, self.loss_fn, self.loss_kw, self.init_fn, self.desc = fam, loss_fn, loss_kw, init_fn, desc
        self.eng_kw = dict(scale_by_accessibility=True) if acc else {}
        tiling = fam == "MultiMixtureNormal"
        survival = data_cpu.selection == "survival"
        self.exchange = "none: every parameter is per target or per guide (loss window all-reduced every " \
                        f"{LOSS_SYNC_EVERY} steps)"
        if strong:
            # the cut run_inference makes under torchrun (parallel.run_sharded)
            if tiling:
                shards = parallel.plan_guide_shards(data_cpu.n_guides, world, getattr(data_cpu, "n_targets", 0))
            else:
                shards = parallel.plan_shards(data_cpu.target_lengths.numpy(), world)
            sh = shards[rank]
            self.shard_cpu = parallel.shard_screen(data_cpu, sh)
            self.offsets = dict(guide_offset=sh[0], target_offset=sh[2], n_guides_total=data_cpu.n_guides)
            if tiling:
                self.offsets["loss_owner"] = rank == 0
            if survival:
                self.offsets["t0_totals"] = (data_cpu.X[:, 0, :].to(torch.float32) + 1).sum(-1)
        else:
            self.shard_cpu = data_cpu
            n_t = getattr(data_cpu, "n_targets", 0)
            self.offsets = dict(guide_offset=rank * guides, target_offset=rank * n_t, n_guides_total=world * guides)
            if tiling or survival:
                self.offsets = {}  # independent screens: these families couple guides through shared quantities
        if tiling:
            # as run_inference hands a tiling screen to its engine: guides ordered by their number of alleles
            self.shard_cpu, ids = parallel.order_by_alleles(self.shard_cpu, self.offsets.get("guide_offset", 0))
            if ids is not None:
                self.offsets["guide_ids"] = ids
        self.data = self.shard_cpu.to(dev)
        self.eng = engine.HipSVI(fam, self.data, num_steps=max(total_steps, 1), loss_capacity=total_steps + 64,
                                 device=dev, **self.eng_kw, **self.offsets)
        # families with something shared across shards step with an exchange inside every step
        self.exchanged = strong and world > 1 and bool(self.eng.exchange_buffers())
        if self.exchanged:
            x = self.eng.exchange_buffers()
            self.exchange = "per step: " + ", ".join(f"all-reduce {k} ({v.numel()} f64)" for k, v in x.items())
            # default: the library steps with its own RCCL communicator (kernels + ncclAllReduce enqueued natively) once
            # the communicator has passed its check; otherwise, or with BEAN_HIP_NATIVE_COMM=0: the Python stepping loop +
            # torch.distributed.all_reduce
            native = False
            if parallel.native_comm_enabled():
                try:
                    native = self.eng.init_native_comm()
                except Exception as exc:  # noqa: BLE001  (never lose the run over the faster path)
                    print(f"[bench] native RCCL stepping unavailable: {exc}", file=sys.stderr)
            self.exchange += "; stepping: " + ("library-owned RCCL communicator, no host in the loop" if native
                                               else "Python loop + torch.distributed.all_reduce")

    def run_steps(self, n):
        import torch
        import torch.distributed as dist

        eng, done = self.eng, 0
        while done < n:
            k = min(LOSS_SYNC_EVERY, n - done)
            first = eng.steps_done
            if self.exchanged:
                eng.run_exchanged(k, dist.all_reduce, seed=101)
            else:
                eng.run(k, seed=101, graph_chunk=self.graph_chunk, resume=True)  # windows, as run_inference steps them
            if self.world > 1:
                with torch.cuda.stream(eng.stream):
                    dist.all_reduce(eng.loss_hist[first:first + k])
            done += k

    def fence(self):
        import torch
        import torch.distributed as dist

        torch.cuda.synchronize(self.dev)
        if self.world > 1:
            dist.barrier()
        torch.cuda.synchronize(self.dev)

    def timed(self, steps, warmup):
        """W untimed steps, then exactly K steps between barrier + synchronize; max over ranks."""
        import torch
        import torch.distributed as dist

        self.run_steps(warmup)
        self.fence()
        t0 = time.perf_counter()
        self.run_steps(steps)
        self.fence()
        dt = time.perf_counter() - t0
        if self.world > 1:
            tt = torch.tensor([dt], dtype=torch.float64, device=self.dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        self.last_ms_per_step = dt / steps * 1e3
        return dt

    def sustained(self, n_steps=2000, window=LOSS_SYNC_EVERY):
        """One whole fit of the reference's default length (`--n-iter 2000`) on this leg's screen, stepped in
        report windows as ``run_inference`` steps it: ms per step over the fit (host clock between fences) and per
        window (HIP events on the engine's stream, no host synchronisation in between).  A 20-step call sees the
        chip at the start of a run; under the tiling and survival kernels' float64 load the clock settles lower
        within a few hundred steps - this is the figure a real `bean run` gets."""
        import torch

        from bean_amd import engine

        if self.exchanged or self.world > 1:
            return None
        eng = engine.HipSVI(self.family, self.data, num_steps=n_steps, device=self.dev, **self.eng_kw, **self.offsets)
        eng.run(window, seed=101, graph_chunk=self.graph_chunk, resume=True)  # graphs instantiated, caches warm
        torch.cuda.synchronize(self.dev)
        eng.steps_done = 0
        n_win = n_steps // window
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_win + 1)]
        t0 = time.perf_counter()
        evs[0].record(eng.stream)
        for w in range(n_win):
            eng.run(window, seed=101, graph_chunk=self.graph_chunk, resume=True, first_step=w * window)
            evs[w + 1].record(eng.stream)
        torch.cuda.synchronize(self.dev)
        dt = time.perf_counter() - t0
        per_window = [evs[w].elapsed_time(evs[w + 1]) / window for w in range(n_win)]
        losses = eng.losses()
        eng.close()
        return {"steps": n_win * window, "window": window, "ms_per_step": dt / (n_win * window) * 1e3,
                "value": n_win * window / dt, "unit": "steps/s", "per_window_ms": [round(x, 5) for x in per_window],
                "final_loss": losses[-1] if losses else None,
                "note": "one 2000-step fit after a 100-step warm-up on a fresh engine; per_window_ms = ms per step of "
                        "each 100-step window (HIP events on the engine's stream)"}

    def kernel_profile(self, eng_steps=50):
        """Dominant-kernel duration: HIP events carrying the kernel's own begin/end timestamps, on the
        launch stream (eager launches of a second engine on the same screen)."""
        import torch

        from bean_amd import engine

        prof = engine.HipSVI(self.family, self.data, num_steps=400, device=self.dev, **self.eng_kw,
                             **self.offsets)
        if prof.dominant_kernel == "k_svi_async":
            # ONE launch covers all the steps of a call (csrc/bean_async_v2.hpp): a warm call, then two timed calls of
            # a report window each; get_profile() divides by the steps the launches covered, k_n counts steps
            prof.run(100, seed=101, graph_chunk=0, resume=True)
            torch.cuda.synchronize(self.dev)
            prof.set_profile(True)
            prof.run(100, seed=101, graph_chunk=0)
            prof.run(100, seed=101, graph_chunk=0, first_step=200)
        else:
            prof.set_profile(True)
            prof.run(eng_steps, seed=101, graph_chunk=0)
        torch.cuda.synchronize(self.dev)
        k_ms, k_n = prof.get_profile()
        out = (k_ms, k_n, prof.step_bytes, prof.dominant_kernel, prof.dominant_lds_bytes, prof.dominant_kernel_variant)
        prof.close()
        return out

    def close(self):
        self.eng.close()


DUMP_LIMIT_BYTES = 64 << 20
DUMP_SAMPLE_SEED = 20240501


def dump_outputs(leg, out_dir, rank, world):
    """``--dump-outputs DIR``: what the timed leg hands its caller after its last step - the parameter store
    (constrained values in screen order, as ``HipSVI.constrained`` gives them to ``run_inference``) and the
    loss of every step the engine ran - as ``DIR/[rank<r>_]<name>.npy`` in float32 / float64.  If the arrays
    together exceed 64 MB, each one is cut to a fixed, seeded sample of its flat elements (same seed, same
    indices in every run), sized so that the files stay within the budget."""
    import numpy as np

    arrays = {f"param_{k}": v.detach().cpu().numpy() for k, v in leg.eng.constrained().items()}
    arrays["loss"] = np.asarray(leg.eng.losses(), dtype=np.float64)
    total = sum(a.nbytes for a in arrays.values())
    budget = DUMP_LIMIT_BYTES - 4096 * len(arrays)  # (room for the .npy headers)
    os.makedirs(out_dir, exist_ok=True)
    prefix = f"rank{rank}_" if world > 1 else ""
    for name, a in sorted(arrays.items()):
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if total > budget:
            keep = max(1, a.size * budget // total)
            idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(a.size, keep, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, prefix + name + ".npy"), a)


def dry_rehearsal(args, rank, world):
    """BEAN_BENCH_REHEARSAL=dry (CPU containers, tests): the ranks rendezvous over gloo and rank 0
    prints the JSON line with null measurements - checks the launch path, measures nothing."""
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo")
        dist.barrier()
    if rank == 0:
        out = {"metric": METRICS[args.config], "value": None, "unit": "steps/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True,
               "scaling": args.scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "rehearsal": "dry: no GPU touched, nothing measured",
               "config": {"workload": None, "config": args.config}}
        if args.scaling == "strong" or (args.full and not args.no_strong):
            out["strong"] = {"guides": args.strong_guides or STRONG_GUIDES[args.config], "value": None,
                             "ms_per_step": None}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


METRICS = {"metric": "SVI steps/sec, 50k-guide x 20-sample sorting model",
           "tiling": "SVI steps/sec, 50k-guide x 200k-allele tiling sorting model",
           "survival": "SVI steps/sec, 100k-guide x 6-timepoint x 3-rep survival model"}
# the ONE screen of the strong leg: BASELINE configs[3] (500k-guide variant sorting), configs[2], configs[4]
STRONG_GUIDES = {"metric": 500_000, "tiling": 50_000, "survival": 100_000}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", choices=("metric", "tiling", "survival"), default="metric")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="which leg `value` reports; with --full the other one is run too (see --no-strong)")
    ap.add_argument("--guides", type=int, default=0, help="guides per GPU of the weak leg")
    ap.add_argument("--strong-guides", type=int, default=0, help="guides of the one screen of the strong leg")
    ap.add_argument("--no-strong", action="store_true", help="--full: skip the strong leg (weak `value` only)")
    ap.add_argument("--graph-chunk", type=int, default=64)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="N = 1, --config metric: skip the tiling and survival legs (`other_configs`)")
    ap.add_argument("--scale-by-acc", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="also the other leg, roofline, sustained fit, CPU baseline and other configurations; a plain "
                         "run times only the leg `value` reports")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed leg computed (parameters after its last step, losses) as DIR/<name>.npy")
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        # no launcher around us: become the launcher (nothing has touched the GPU yet)
        sys.exit(self_launch(sys.argv[1:], args.gpus))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # rehearsals, never set by the driver: "1" puts every rank on device 0 of a one-GPU box and
    # exchanges over gloo (RCCL refuses two ranks on one device); "dry" touches no GPU at all
    rehearsal = os.environ.get("BEAN_BENCH_REHEARSAL", "")
    if rehearsal == "dry":
        return dry_rehearsal(args, rank, world)

    import torch
    import torch.distributed as dist

    import bean_amd  # noqa: F401

    if rehearsal == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if rehearsal == "1":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    total = args.warmup + args.steps
    weak_guides = args.guides or DEFAULT_GUIDES[args.config]
    strong_guides = args.strong_guides or STRONG_GUIDES[args.config]
    report_strong = args.scaling == "strong"
    # a plain run times the one leg `value` reports; the other leg and everything else is --full's
    want_weak = args.full or not report_strong
    want_strong = report_strong or (args.full and not args.no_strong)
    # at one rank the strong leg of tiling / survival IS the weak leg (same screen, nothing to cut)
    same_leg = world == 1 and strong_guides == weak_guides and not args.scale_by_acc

    weak = sleg = roof = sustained = strong_obj = None
    losses = []
    if want_weak or (want_strong and same_leg):
        weak = Leg(args, args.config, False, weak_guides, rank, world, dev, total)
        dt_weak = weak.timed(args.steps, args.warmup)
        losses = weak.eng.losses()
        if args.dump_outputs and (not report_strong or same_leg):
            dump_outputs(weak, args.dump_outputs, rank, world)
        if args.full:
            std_size = weak_guides == DEFAULT_GUIDES[args.config] and not args.scale_by_acc
            roof = roofline_object(args.config, weak, weak_guides, std_size) if rank == 0 else None
            sustained = weak.sustained() if (rank == 0 and world == 1) else None
            if rank != 0:
                weak.kernel_profile()  # (every rank runs the same launches: the legs stay in step)
    if want_strong:
        if same_leg:
            sleg, dt_strong = weak, dt_weak
        else:
            if weak is not None:
                weak.close()
            sleg = Leg(args, args.config, True, strong_guides, rank, world, dev, total)
            dt_strong = sleg.timed(args.steps, args.warmup)
            if args.dump_outputs and report_strong:
                dump_outputs(sleg, args.dump_outputs, rank, world)
        strong_obj = {
            "guides": strong_guides,
            "guides_this_rank": int(sleg.data.n_guides),
            "value": args.steps / dt_strong,
            "unit": "steps/s of the WHOLE screen",
            "ms_per_step": dt_strong / args.steps * 1e3,
            "workload": sleg.desc + f"; ONE screen cut into {world} shard(s) as run_inference cuts it under torchrun",
            "exchange": sleg.exchange,
            "final_loss": sleg.eng.losses()[-1] if rank == 0 else None,
        }
        if weak is None:
            losses = sleg.eng.losses()
        if sleg is not weak:
            sleg.close()
    head = sleg if report_strong else weak

    if rank == 0:
        value = strong_obj["value"] if report_strong else world * args.steps / dt_weak
        ms = strong_obj["ms_per_step"] if report_strong else dt_weak / args.steps * 1e3
        metric = METRICS[args.config]
        if report_strong:
            metric = f"SVI steps/sec, ONE {strong_guides}-guide screen ({args.config}) guide-sharded over the ranks"
        out = {
            "metric": metric,
            "value": value,
            "unit": "steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": (strong_obj["workload"] if report_strong else
                             weak.desc + "; one SVI step = draw + ELBO + grad + ClippedAdam; per GPU"),
                "config": args.config,
                "guides": strong_guides if report_strong else weak_guides,
                "guides_this_rank": strong_obj["guides_this_rank"] if report_strong else int(weak.data.n_guides),
                "n_reps": int(head.data.n_reps),
                "n_condits": int(head.data.n_condits),
                "parallelism": (f"one screen guide-sharded x{world}" if report_strong
                                else f"one screen per GPU x{world}")
                               + f", loss all-reduce every {LOSS_SYNC_EVERY} steps",
                "graph_chunk": args.graph_chunk,
                "value_counts": ("steps of the whole screen" if report_strong
                                 else "steps of one screen, summed over ranks"),
                "final_loss": losses[-1] if losses else None,
            },
        }
        if args.full:
            out["roofline"] = roof
        if sustained is not None:
            out["sustained"] = sustained
        if strong_obj is not None:
            out["strong"] = strong_obj
        if not report_strong:
            out["weak"] = {"guides_per_gpu": weak_guides, "value": world * args.steps / dt_weak,
                           "ms_per_step": dt_weak / args.steps * 1e3}
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(weak.family, weak.shard_cpu, weak.loss_fn, weak.loss_kw, weak.init_fn)
            out["config"]["gpu_over_cpu"] = (world * args.steps / dt_weak) / out["cpu_baseline"]["value"]
        if (args.full and world == 1 and args.config == "metric" and not args.no_other_configs
                and not args.scale_by_acc):
            # BASELINE configs[2] and configs[4] on the same line, same --steps / --warmup
            weak.close()
            out["other_configs"] = {c: other_config(args, c, rank, dev) for c in ("tiling", "survival")}
            out["other_configs"]["tiling_acc"] = other_config(args, "tiling", rank, dev, acc=True)
            out["other_configs"]["readme_shape"] = readme_shape(args, dev)
            # the headline metric itself has no published number: `vs_baseline` stays null; the one
            # number the reference does publish is on another shape and is compared there
            out["vs_baseline_readme_shape"] = out["other_configs"]["readme_shape"]["vs_baseline"]
        print(json.dumps(out), flush=True)
    if weak is not None:
        weak.close()  # (closing twice is a no-op)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
