"""Record the count simulators' draws, bit for bit, on a GPU (tests/test_gpu_simulator_golden.py holds every later
build to them).

    python tests/golden/make_simulator_golden.py

Every case is one engine on one small screen, seed 101, parameters moved off their initial values as the simulator
tests move them.  What is recorded, at draw 2:

    sorting screens    simulate(alphas=True), simulate_members(2, 3), simulate_design(2, 2, (0.5, 1, 2)),
                       simulate_power(2, 2, (0, 0.75), plant = every other target), and pi of drawn_noise()
    survival screens   simulate_survival(alphas=True), simulate_survival_members(2, 3) with nothing injected (members
                       1 and 2 redraw their baseline u_g), for MixtureNormal the same call with eps_u injected, and pi
                       and the Dirichlet-over-all-guides draw of drawn_noise()

in three families (Normal, MixtureNormal, MixtureNormal with accessibility and fit_noise) on

    conditions-3       64 guides x 1 replicate x 3 bins: a lone last bin in the gamma pairs
    log-branch         128 x 2 x 5, a0 = 1e-3, the near-floor regime's bins and totals: pairs normalised in logs
    variant-70         70 x 2 x 5: a second tile with 6 valid lanes, masks, a real size-factor spread
    survival-70        70 x 2 x 6 timepoints, masks;  survival-70-t3: timepoints (0, 7, 14), an odd B
    survival-70-log    survival-70 with a0 = a0_bcmatch = 1e-3 (Normal, MixtureNormal)

A case is stored as two arrays, "<screen>/<family>/counts" and "<screen>/<family>/float64": its counts end to end in
the narrowest unsigned integer type that holds them (they are whole numbers in float32: the conversion back is exact),
and its float64 arrays end to end as they are.  unpack() cuts them back into the arrays of the calls.

THE LOG BRANCH IS REACHED.  A gamma of concentration alpha falls below the threshold of the log branch when
U < exp(-668 alpha); on the a0 = 1e-3 screens all bins of a pair do so in about half the pairs.  With the branch the
pair follows the Dirichlet-Multinomial law, under which all reads of a pair fall in ONE bin with probability
sum_b prod_{i < n} (alpha_b + i) / (A + i) - above 0.99 at a total concentration A = 1e-3 - and without it the pairs
whose gammas all underflow would share their reads evenly.  main() asserts alpha.max() < 1e-3 and that at least 90 % of
the pairs with 8 reads or more have all of them in one bin; at a number of conditions other than 5 it prints the law's
share E and the probability q that every gamma of a pair underflows, and asserts the observed share against E - 0.1,
which separates the two builds as long as q E > 0.1 (asserted as well).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import bean_amd  # noqa: E402,F401
import dm_reference as dm  # noqa: E402
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen, make_survival_variant_screen  # noqa: E402

OUT = os.path.join(HERE, "simulator_draws.npz")
MAX_BYTES = 256 * 1024
DEV = "cuda:0"
SEED = 101
DRAW = 2
K = 3
DEPTHS = (0.5, 1.0, 2.0)
EFFECTS = (0.0, 0.75)
LOG_A0 = 1e-3
T3 = (0.0, 7.0, 14.0)
FAMILIES = [("Normal", "Normal", dict()), ("MixtureNormal", "MixtureNormal", dict()),
            ("MixtureNormal+Acc", "MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True))]


def _with_a0(data, a0):
    import copy

    out = copy.copy(data)
    out.a0 = torch.full_like(data.a0, a0)
    out.a0_bcmatch = torch.full_like(data.a0_bcmatch, a0)
    return out


def screen(name, acc):
    if name == "conditions-3":
        return dm.regime_screen("conditions-3", acc)
    if name == "log-branch":
        return dm.flat_screen(128, 2, dm.regime_bins(5), dm.regime_totals("near-floor"), a0=LOG_A0, with_accessibility=acc)
    if name == "variant-70":
        return make_sorting_variant_screen(70, 2, depth_per_guide=17.0, seed=11, with_accessibility=acc, mask_fraction=0.05)
    surv = dict(depth_per_guide=17.0, seed=11, with_accessibility=acc, mask_fraction=0.05)
    if name == "survival-70":
        return make_survival_variant_screen(70, 2, **surv)
    if name == "survival-70-t3":
        return make_survival_variant_screen(70, 2, times=T3, **surv)
    if name == "survival-70-log":
        return _with_a0(make_survival_variant_screen(70, 2, **surv), LOG_A0)
    raise KeyError(name)


def cases():
    """[(screen name, family label)]"""
    out = []
    for name in ("conditions-3", "log-branch", "variant-70", "survival-70", "survival-70-t3", "survival-70-log"):
        for label, _, kw in FAMILIES:
            if name == "survival-70-log" and kw:
                continue
            out.append((name, label))
    return out


def engine_of(name, label):
    from bean_amd import engine

    family, kw = next((f, k) for lab, f, k in FAMILIES if lab == label)
    data = screen(name, bool(kw))
    eng = engine.HipSVI(family, data.to(DEV), num_steps=50, dump_noise=True, **kw)
    torch.manual_seed(3)  # parameters a fit could have reached, not the initial ones
    for v in eng.unconstrained.values():
        v.add_(0.3 * torch.randn_like(v))
    return eng, data


def record(name, label):
    """{key: cpu tensor} of one case, as the device leaves them."""
    eng, data = engine_of(name, label)
    out = {}

    def put(call, got):
        for k, v in got.items():
            out[f"{call}/{k}"] = v.cpu()

    def noise():
        return {k: v for k, v in eng.drawn_noise().items() if k in ("pi", "q_0", "initial_abundance")}

    try:
        if name.startswith("survival"):
            assert eng.survival_predictive_supported
            put("simulate", eng.simulate_survival(DRAW, seed=SEED, alphas=True))
            single = noise()
            put("noise", single)
            put("members", eng.simulate_survival_members(DRAW, K, seed=SEED))
            if label.startswith("MixtureNormal"):
                eps_u = torch.randn(data.n_guides, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
                eng.set_noise({"eps_u": eps_u})
                put("members-eps_u", eng.simulate_survival_members(DRAW, K, seed=SEED))
                eng.set_noise(None)
        else:
            assert eng.predictive_supported
            put("simulate", eng.simulate(DRAW, seed=SEED, alphas=True))
            single = noise()
            put("noise", single)
            put("members", eng.simulate_members(DRAW, K, seed=SEED))
            put("design", eng.simulate_design(DRAW, 2, DEPTHS, seed=SEED))
            put("power", eng.simulate_power(DRAW, 2, EFFECTS, plant=torch.arange(int(eng.T)) % 2 == 0, seed=SEED))
        torch.cuda.synchronize()
        # member 0 alone writes the dumped draws, and it is draw DRAW: what the single draw left is still there
        after = noise()
        assert set(after) == set(single) and all(torch.equal(after[k].cpu(), single[k].cpu()) for k in single), (name, label)
    finally:
        eng.close()
    return out


COUNT_KEYS = [f"{call}/{key}" for key in ("X", "X_bcmatch")
              for call in ("simulate", "members", "members-eps_u", "design", "power")]


def split(arrays):
    """The arrays of one case in their stored order: ([(key, float32 counts)], [(key, float64 array)]).  The counts of
    one likelihood lie next to each other, so that the planes two calls share compress to one."""
    counts = [(k, arrays[k]) for k in COUNT_KEYS if k in arrays]
    doubles = [(k, v) for k, v in arrays.items() if v.dtype == torch.float64]
    assert all(v.dtype == torch.float32 for _, v in counts) and len(counts) + len(doubles) == len(arrays)
    return counts, doubles


def pack(arrays):
    """One case as stored: its counts end to end in the narrowest unsigned type that holds them, its float64 arrays end
    to end as they are."""
    counts, doubles = split(arrays)
    c = np.concatenate([v.numpy().reshape(-1) for _, v in counts])
    assert (c >= 0).all() and (c == np.round(c)).all()
    narrow = c.astype(np.uint8 if c.max() < 256 else (np.uint16 if c.max() < 65536 else np.uint32))
    assert np.array_equal(narrow.astype(np.float32), c)
    return {"counts": narrow, "float64": np.concatenate([v.numpy().reshape(-1) for _, v in doubles])}


def unpack(stored, like):
    """{key: tensor} of one case from its two stored arrays, in the shapes of `like` (the same case drawn again)."""
    counts, doubles = split(like)
    out = {}
    for flat, group in ((torch.from_numpy(stored["counts"].astype(np.float32)), counts),
                        (torch.from_numpy(np.ascontiguousarray(stored["float64"])), doubles)):
        assert flat.numel() == sum(v.numel() for _, v in group)
        at = 0
        for k, v in group:
            out[k] = flat[at:at + v.numel()].reshape(v.shape)
            at += v.numel()
    return out


def one_bin_share(got, name, label):
    """(pairs with 8 reads or more, those with all reads in one bin, the law's expected share E, the probability q that
    every gamma of a pair underflows) over the single draw and the members of a log-branch case."""
    alpha = got["simulate/alpha"].numpy()  # (2, R, B, G)
    pairs = ones = 0
    law, under = [], []
    for lik, key in enumerate(("X", "X_bcmatch")):
        planes = [got[f"simulate/{key}"].numpy()[None], got[f"members/{key}"].numpy()]
        x = np.concatenate(planes)  # (1 + K, R, B, G)
        n = x.sum(2)
        deep = n >= 8
        pairs += int(deep.sum())
        ones += int(((x.max(2) == n) & deep).sum())
        al = alpha[lik]
        for r, g in zip(*np.nonzero(deep[0])):
            a, i = al[r, :, g], np.arange(int(n[0, r, g]), dtype=np.float64)
            law.append(np.exp((np.log(a[:, None] + i) - np.log(a.sum() + i)).sum(1)).sum())
            under.append(np.exp(-668.0 * a.sum()))
    return pairs, ones, float(np.mean(law)), float(np.mean(under))


def check_log_branch(got, name, label):
    alpha = got["simulate/alpha"]
    assert float(alpha.max()) < 1e-3, (name, label, float(alpha.max()))
    pairs, ones, law, under = one_bin_share(got, name, label)
    B = alpha.shape[2]
    bound = 0.9 if B == 5 else law - 0.1
    print(f"{name}/{label}: B = {B}, {ones} of {pairs} pairs with 8 reads or more hold them in one bin "
          f"({ones / pairs:.4f}); the law gives {law:.4f}, every gamma underflows in {under:.3f} of the pairs; "
          f"bound {bound:.4f}")
    assert pairs >= 400 and under * law > 0.1, (pairs, under, law)
    assert ones >= bound * pairs, (name, label, ones, pairs, bound)


def main():
    stored, n_arrays = {}, 0
    for name, label in cases():
        one = record(name, label)
        if "log" in name:
            check_log_branch(one, name, label)
        packed = pack(one)
        back = unpack(packed, one)
        assert set(back) == set(one) and all(torch.equal(back[k], one[k]) for k in one), (name, label)
        stored.update({f"{name}/{label}/{k}": v for k, v in packed.items()})
        n_arrays += len(one)
    np.savez_compressed(OUT, **stored)
    size = os.path.getsize(OUT)
    print(f"{len(cases())} cases, {n_arrays} arrays, {size} bytes")
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
