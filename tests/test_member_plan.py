"""The member plans (``model/jackknife.py::MemberPlan``) of the seed ensemble and the three jackknives, on the CPU: their
screens stack to exactly the tensors the public ``*_member_*`` functions give, their labels, dump tags and dump fields
are the literal ones the halts have always written, and ``_fit_plan`` splits a plan into runs led by member 0."""
import pytest
import torch

import bean_amd  # noqa: F401
from bean_amd.model import jackknife as jk
from bean_amd.model import run as model_run
from bean_amd.preprocessing.synthetic import make_sorting_variant_screen


@pytest.fixture(scope="module")
def data():
    """24 guides (6 targets of 4) x 3 replicates x 4 conditions, some (replicate, guide) pairs masked; every sample is
    alive, so there are 12 of them to leave out."""
    d = make_sorting_variant_screen(24, 3, bins=((0.0, 0.2), (0.2, 0.4), (0.8, 1.0)), guides_per_target=4, seed=5)
    assert (d.n_guides, d.n_reps, d.n_condits, d.n_targets) == (24, 3, 4, 6)
    d.repguide_mask = d.repguide_mask.clone()
    for r, g in ((0, 3), (1, 3), (2, 10), (1, 17)):
        d.repguide_mask[r, g] = False
    assert bool((d.sample_mask != 0).all()) and bool(d.repguide_mask.any(0).all())
    return d


def _screens(plan):
    return [plan.screen(k) for k in range(len(plan.seeds))]


def _equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b))


def test_seed_plan(data):
    plan = jk.seed_plan(data, [101, 7.0])
    assert plan.seeds == [101, 7] and all(s is data for s in _screens(plan))
    assert plan.labels == ["member 0", "member 1"] and plan.tags == ["member0", "member1"]
    assert plan.dump_extra == [{"member": 0, "seed": 101}, {"member": 1, "seed": 7}]
    assert plan.differ_in == () and plan.per_run is None and plan.label_halts is False and plan.chosen == ()
    _equal(jk.stack_masks(_screens(plan)), (torch.stack([data.repguide_mask != 0] * 2), torch.stack([data.sample_mask] * 2)))
    _equal(jk.stack_counts(_screens(plan)), jk.sample_member_counts(data, [[]]))
    with pytest.raises(ValueError, match="run_inference_ensemble needs at least one seed"):
        jk.seed_plan(data, [])
    with pytest.raises(Exception):  # frozen
        plan.per_run = 3


def test_replicate_plan(data):
    plan = jk.replicate_plan(data, 101)
    assert plan.chosen == ([0, 1, 2],) and plan.seeds == [101] * 4 and plan.screen(0) is data
    assert plan.labels == ["the full screen", "replicate 0 left out", "replicate 1 left out", "replicate 2 left out"]
    assert plan.tags == ["full", "without_replicate0", "without_replicate1", "without_replicate2"]
    assert plan.dump_extra == [{"left_out": None, "seed": 101}, {"left_out": 0, "seed": 101},
                               {"left_out": 1, "seed": 101}, {"left_out": 2, "seed": 101}]
    assert plan.differ_in == ("masks",) and plan.per_run is None and plan.label_halts is False
    _equal(jk.stack_masks(_screens(plan)), jk.member_masks(data, [0, 1, 2]))
    _equal(jk.stack_counts(_screens(plan)), jk.sample_member_counts(data, [[]] * 3))  # the counts are the screen's
    # a replicate that is masked already is no member: the labels carry the replicate, not the member's index
    plan = jk.replicate_plan(jk.leave_out(make_sorting_variant_screen(24, 4, seed=5), 1), 7)
    assert plan.chosen == ([0, 2, 3],) and plan.tags == ["full", "without_replicate0", "without_replicate2", "without_replicate3"]
    assert plan.dump_extra[2] == {"left_out": 2, "seed": 7}
    with pytest.raises(ValueError, match="at least two replicates that are not fully masked, found 1"):
        jk.replicate_plan(jk.leave_out(jk.leave_out(data, 0), 1), 101)


def test_guide_plan(data):
    plan = jk.guide_plan(data, 101, 63)
    positions, included = plan.chosen
    assert positions == [0, 1, 2, 3] and included.shape == (6, 4) and bool(included.all())
    assert plan.seeds == [101] * 5 and plan.screen(0) is data
    assert plan.labels == ["the full screen", "guides at position 0 of their targets left out",
                           "guides at position 1 of their targets left out", "guides at position 2 of their targets left out",
                           "guides at position 3 of their targets left out"]
    assert plan.tags == ["full", "without_guide_position0", "without_guide_position1", "without_guide_position2",
                         "without_guide_position3"]
    assert plan.dump_extra == [{"left_out_position": None, "seed": 101}, {"left_out_position": 0, "seed": 101},
                               {"left_out_position": 1, "seed": 101}, {"left_out_position": 2, "seed": 101},
                               {"left_out_position": 3, "seed": 101}]
    assert plan.differ_in == ("masks",) and plan.per_run is None and plan.label_halts is True
    _equal(jk.stack_masks(_screens(plan)), jk.guide_member_masks(data, [0, 1, 2, 3]))
    assert not bool(plan.screen(3).repguide_mask[:, [2, 6, 10, 14, 18, 22]].any())
    with pytest.raises(ValueError, match="takes 1 to 63 positions per target"):
        jk.guide_plan(data, 101, 64)
    with pytest.raises(ValueError, match="at least one guide to leave out"):
        jk.guide_plan(data, 101, 3)


def test_sample_plan(data):
    plan = jk.sample_plan(data, "sample", 101, 63)
    groups, names = plan.chosen
    pairs = [(r, b) for r in range(3) for b in range(4)]
    assert groups == [[p] for p in pairs] and plan.seeds == [101] * 13 and plan.screen(0) is data
    assert names == ["r0_c0", "r0_c1", "r0_c2", "r0_c3", "r1_c0", "r1_c1", "r1_c2", "r1_c3", "r2_c0", "r2_c1", "r2_c2", "r2_c3"]
    assert plan.labels[:3] == ["the full screen", "sample r0_c0 left out", "sample r0_c1 left out"]
    assert plan.labels[12] == "sample r2_c3 left out" and plan.labels[1:] == [f"sample r{r}_c{b} left out" for r, b in pairs]
    assert plan.tags[:3] == ["full", "without_r0_c0", "without_r0_c1"] and plan.tags[12] == "without_r2_c3"
    assert plan.tags[1:] == [f"without_r{r}_c{b}" for r, b in pairs]
    assert plan.dump_extra[:2] == [{"left_out": None, "seed": 101}, {"left_out": [[0, 0]], "seed": 101}]
    assert plan.dump_extra[7] == {"left_out": [[1, 2]], "seed": 101}
    assert plan.dump_extra[1:] == [{"left_out": [[r, b]], "seed": 101} for r, b in pairs]
    assert plan.differ_in == ("masks", "counts") and plan.per_run == 63 and plan.label_halts is True
    _equal(jk.stack_masks(_screens(plan)), jk.sample_member_masks(data, groups))
    _equal(jk.stack_counts(_screens(plan)), jk.sample_member_counts(data, groups))
    x, x_bc = jk.stack_counts(_screens(plan))
    assert x.dtype == torch.float32 and x.shape == (13, 3, 4, 24) and x_bc.shape == x.shape
    assert not bool(x[7, 1, 2].any()) and bool(x[7, 1, 1].any()) and bool(x[0, 1, 2].any())

    plan = jk.sample_plan(data, "condition", 7, 5)
    groups, names = plan.chosen
    assert groups == [[(0, b), (1, b), (2, b)] for b in range(4)] and names == ["c0", "c1", "c2", "c3"]
    assert plan.labels == ["the full screen", "condition c0 left out", "condition c1 left out", "condition c2 left out",
                           "condition c3 left out"]
    assert plan.tags == ["full", "without_c0", "without_c1", "without_c2", "without_c3"]
    assert plan.dump_extra == [{"left_out": None, "seed": 7}, {"left_out": [[0, 0], [1, 0], [2, 0]], "seed": 7},
                               {"left_out": [[0, 1], [1, 1], [2, 1]], "seed": 7}, {"left_out": [[0, 2], [1, 2], [2, 2]], "seed": 7},
                               {"left_out": [[0, 3], [1, 3], [2, 3]], "seed": 7}]
    assert plan.per_run == 5
    _equal(jk.stack_masks(_screens(plan)), jk.sample_member_masks(data, groups))
    _equal(jk.stack_counts(_screens(plan)), jk.sample_member_counts(data, groups))
    for bad in (0, 64):
        with pytest.raises(ValueError, match=r"max_groups_per_run must be in \[1, 63\]"):
            jk.sample_plan(data, "sample", 101, bad)
    with pytest.raises(ValueError, match="by must be 'sample' or 'condition'"):
        jk.sample_plan(data, "bin", 101, 63)


def test_fit_plan_splits_into_runs_led_by_member_0(data, monkeypatch):
    """12 groups, at most 5 next to the full screen: runs of 5 / 5 / 2, member 0 in each, its result from the first."""
    runs = []

    def fake(model, guide, d, plan, run, common, report_every, verbose):
        runs.append(list(run))
        return [(len(runs), k) for k in run]

    monkeypatch.setattr(model_run, "_fit_members", fake)
    plan = jk.sample_plan(data, "sample", 101, 5)
    got = model_run._fit_plan(None, None, data, plan, dict(num_steps=10), 100, False)
    assert runs == [[0, 1, 2, 3, 4, 5], [0, 6, 7, 8, 9, 10], [0, 11, 12]]
    assert got == [(1, 0)] + [(1, k) for k in range(1, 6)] + [(2, k) for k in range(6, 11)] + [(3, 11), (3, 12)]
    runs.clear()
    assert len(model_run._fit_plan(None, None, data, jk.seed_plan(data, [3]), dict(num_steps=10), 100, False)) == 1
    assert len(model_run._fit_plan(None, None, data, jk.replicate_plan(data, 101), dict(num_steps=10), 100, False)) == 4
    assert runs == [[0], [0, 1, 2, 3]]  # without per_run: all in one


def test_member_mode_keeps_each_caller_its_own_rules():
    """The parser's rule on --jackknife-guides-max is the parser's alone, and the two checkers of one flag family look at
    that family's rules only."""
    from bean_amd.cli import run as cli_run
    from bean_amd.cli.execute import check_run_switches, get_parser

    parser = get_parser()
    run = ["run", "sorting", "variant", "screen.h5ad"]
    wide = parser.parse_args(run + ["--jackknife-guides", "--jackknife-guides-max", "64"])
    assert cli_run.member_mode(wide) == "guides" and cli_run.check_guide_jackknife_switches(wide) is True
    with pytest.raises(SystemExit):
        check_run_switches(parser, wide)
    other = parser.parse_args(run + ["--jackknife-replicates", "--n-seeds", "2"])
    assert cli_run.check_guide_jackknife_switches(other) is False and cli_run.check_sample_jackknife_switches(other) is None
    with pytest.raises(ValueError, match="--jackknife-replicates fits every member with the same seed"):
        cli_run.member_mode(other)
    assert cli_run.member_mode(parser.parse_args(run)) is None
    assert cli_run.member_mode(parser.parse_args(run + ["--n-seeds", "3"])) == "seeds"
    assert cli_run.member_mode(parser.parse_args(run + ["--jackknife-conditions"])) == "condition"
