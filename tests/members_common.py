"""What the GPU tests of the member sets share (test_gpu_ensemble.py, test_gpu_jackknife.py, test_gpu_guide_jackknife.py,
test_gpu_sample_jackknife.py): the state of a fit, the single fit a member is compared with, the configurations, and
the CLI helpers.  A plain module imported by bare name; the autouse fixture is imported into each module's namespace."""
import csv
import io
import os

import pytest
import torch

from bean_amd.cli.execute import get_parser
from bean_amd.cli.execute import main as bean_main
from bean_amd.framework import h5ad_io

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VAR = os.path.join(GOLD, "var_mini_screen.h5ad")
SEED = 101
STEPS = 300


@pytest.fixture(autouse=True)
def _h5ad_reader_present():
    try:
        import h5py  # noqa: F401
    except ImportError:
        assert os.path.exists(h5ad_io.HELPER_PYTHON), "no h5py helper interpreter: .h5ad screens cannot be read here"


def _mini(tmp_path, *extra):
    from bean_amd.cli import run as cli_run

    args = get_parser().parse_args(["run", "sorting", "variant", VAR, *extra, "-o", str(tmp_path), "--sample-mask-col", ""])
    return cli_run.main(args, return_data=True)


def _state(eng, member=None):
    pick = (lambda t: t) if member is None else (lambda t: t[member])
    out = {f"p.{k}": pick(v).clone() for k, v in eng.unconstrained.items()}
    out.update({f"m.{k}": pick(v).clone() for k, v in eng._m.items()})
    out.update({f"v.{k}": pick(v).clone() for k, v in eng._v.items()})
    out["loss"] = pick(eng.loss_hist)[: eng.steps_done].clone()
    return out


def _single(family, data, kw, seed=SEED, steps=STEPS, **run_kw):
    from bean_amd import engine

    eng = engine.HipSVI(family, data, num_steps=STEPS, **kw)
    eng.run(steps, seed=seed, **run_kw)
    torch.cuda.synchronize()
    st = _state(eng)
    eng.close()
    return st


def _assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), (what, k, (got[k].double() - want[k].double()).abs().max().item())


def _priors(data):
    t = data.n_targets
    g = torch.Generator().manual_seed(5)
    return {"mu_loc": 0.2 * torch.randn(t, 1, generator=g), "mu_scale": 0.5 + torch.rand(t, 1, generator=g),
            "sd_loc": 0.1 * torch.randn(t, 1, generator=g), "sd_scale": 0.05 + 0.1 * torch.rand(t, 1, generator=g)}


CONFIGS = [
    ("Normal", dict()),
    ("Normal", dict(use_bcmatch=False)),
    ("MixtureNormal", dict()),
    ("MixtureNormal", dict(use_bcmatch=False)),
    ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=True)),
    ("MixtureNormal", dict(scale_by_accessibility=True, fit_noise=False)),
    ("MixtureNormal", dict(prior="yes")),
    ("Normal", dict(prior="yes")),
]


def _kw_of(kw, data):
    kw = dict(kw)
    if kw.pop("prior", None):
        kw["prior_params"] = _priors(data)
    return kw


def _same_results(got, want):
    """Two results of ``run_inference``: the same losses and, bit for bit, the same parameters in store and dict."""
    store, out = got
    ref_store, ref = want
    assert set(out) == {"loss", "params"} and out["loss"] == ref["loss"]
    assert set(out["params"]) == set(ref["params"]) == set(store.keys())
    for k, v in ref["params"].items():
        assert out["params"][k].device.type == "cpu" and torch.equal(out["params"][k], v), k
        assert torch.equal(store[k].cpu(), ref_store[k].cpu()), k


def _run(out, *argv):
    os.makedirs(out)
    assert bean_main(["run", *argv, "-o", out, "--sample-mask-col", ""]) == 0
    (d,) = [os.path.join(out, p) for p in os.listdir(out) if p.startswith("bean_run_result.")]
    return d


def _without_columns(path, names):
    """The CSV file's bytes with the named columns cut out, field text untouched."""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    keep = [i for i, c in enumerate(rows[0]) if c not in names]
    assert len(keep) == len(rows[0]) - len(names)
    buf = io.StringIO()
    csv.writer(buf, lineterminator="\n").writerows([[row[i] for i in keep] for row in rows])
    return buf.getvalue().encode()
