"""The composed statement of a north-star frame (tests/northstar_statement.py) on its own, without a GPU and without a solve:
the chain runs every case of tests/northstar_cases.py with the planted camera motion standing in for the solved transforms
and asserts that
  - the cases meet their conditions (seeds, hidden shares, growth, appended nodes, knife-edge shares at most 1 %, no
    field-growth knife edge);
  - every stage accepts its own output: frame() of the chain's records is empty;
  - every defect of northstar_statement.DEFECTS, planted into the stated side, makes the comparison of its case's chain fail
    (the flat regularisation graph: on nodes that do not all carry one motion).
And the C++ side of the dump's inputs: `test_host_northstar_frames` without arguments (the parameter file round-trips, a
missing or short frame file is an error)."""
import subprocess

import numpy as np
import pytest

import northstar_cases as C
import northstar_statement as NS

_CHAINS = {}


def chain(name):
    if name not in _CHAINS:
        case = C.Case(name)
        depths, colors = C.depths_of(name), C.colors_of(name)
        steps = C.steps_of(name)
        solved_of = lambda i: None if i in C.EMPTY.get(name, ()) else C.planted(steps[i])
        _CHAINS[name] = (case, NS.chain_records(case, depths, colors, solved_of), depths, colors, {})
    return _CHAINS[name]


def compare(ch, stages, defect=None, frames=None):
    case, recs, depths, colors, infos = ch
    bad = []
    for i in (range(case.frames) if frames is None else frames):
        inp = dict(index=i, depth=depths[i], color=colors[i], prev_color=colors[i - 1] if i else None)
        bad += NS.frame(recs[i - 1] if i else None, recs[i], inp, case, defect=defect, stages=stages,
                        info=infos.setdefault(i, {}) if defect is None else {})
    return bad


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_stage_accepts_its_own_output_and_the_case_meets_its_conditions(name):
    ch = chain(name)
    case, recs, depths, _, infos = ch
    assert compare(ch, NS.STAGES) == []
    D = [r["D"] for r in recs]
    print(name, "nodes", D, "vertices", [r["canonical_vertices"] for r in recs])
    assert any(b > a for a, b in zip(D, D[1:])), "no frame appends nodes"
    assert 30 <= D[0] <= 60
    for i, info in sorted(infos.items()):
        print(name, "frame", i, {k: v for k, v in info.items() if k != "rigid"})
        for k in ("raster_knife", "flags_undecided", "fusion_undecided"):
            assert info.get(k, 0.0) <= 0.01, (i, k, info[k])
        assert info.get("cost", dict(amb=0.0))["amb"] <= 0.01
        assert not info.get("growth_knife", False)
    if case.north_star_reg_hierarchy:
        assert all(sum(1 for n in r["level_counts"] if n) > 1 for r in recs[1:])
    if case.north_star_visible_only:
        hidden = [float((r["visible_flags"] == 0).mean()) for r in recs[1:]]
        print(name, "hidden shares", hidden)
        assert all(0.05 <= h <= 0.60 for h in hidden), hidden
    if name == "regrow_colour":
        assert not depths[2].any() and recs[2]["rigid_skipped"] == 1
        assert recs[3]["canonical_vertices"] >= 1.2 * recs[0]["canonical_vertices"]
        w = recs[3]["color_volume"] >> 24
        assert w.max() == 3 and (w == 3).sum() > 100


# The chain's "solved" transforms are ONE rigid motion for every node, so no regularisation edge has a residual there whichever
# graph holds it.  For the flat-graph defect the nodes before a frame are therefore given transforms that are NOT one motion —
# every other node carried 3 m further along x (the Huber weight makes an edge's energy linear in its residual) — and the record's initial cost is the statement's at those transforms: the
# flat graph must then miss it by more than the cost's budget.
def test_the_flat_graph_defect_moves_the_cost_beyond_its_budget():
    what, stages, name = NS.DEFECTS["flat_reg"]
    case, recs, depths, colors, _ = chain(name)
    caught = 0
    for i in range(1, case.frames):
        before, after = dict(recs[i - 1]), dict(recs[i])
        dq = before["node_dq"].astype(np.float64)
        tq = np.zeros((len(dq), 4))
        tq[::2, 1] = 3.0
        dq[:, 4:] += 0.5 * NS.RS.qmul(tq, dq[:, :4])  # a translation t after the transform: d += 1/2 (0, t) r
        before["node_dq"] = dq.astype(np.float32)
        start = NS.compose(before["node_dq"], after["rigid_pose"])
        lv = NS.levels(before, case)
        after["initial_cost"] = NS.solve_start(before, after, case, start, after["visible_flags"], lv).cost
        inp = dict(index=i, depth=depths[i], color=colors[i], prev_color=colors[i - 1])
        assert NS.frame(before, after, inp, case, stages="f") == []
        bad = NS.frame(before, after, inp, case, defect="flat_reg", stages="f")
        print("frame", i, bad)
        caught += bad != []
    assert caught == case.frames - 1


@pytest.mark.parametrize("defect", [d for d in NS.DEFECTS if d != "flat_reg"])  # (flat_reg: the test above)
def test_a_planted_defect_changes_a_stage_by_more_than_its_bar(defect):
    what, stages, name = NS.DEFECTS[defect]
    ch = chain(name)
    bad = compare(ch, stages, defect=defect, frames=range(1, ch[0].frames))
    print(defect, "(%s):" % what, bad[:2])
    assert bad != []


def test_dump_program_reads_its_inputs_strictly():
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_northstar_frames"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "2 tests, 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
