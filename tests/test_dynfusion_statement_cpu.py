"""The composed statement of a reference-mode frame (tests/dynfusion_statement.py) on its own, without a GPU: the chain runs
every case of tests/dynfusion_cases.py with the project's C oracle of the reference's solve standing in for the device's and
asserts that
  - the cases meet the conditions that need no device (seeds, appended nodes, a frame that appends none before a frame that
    reuses the graph, Tukey weights at 0 and strictly between 0 and 1, tied live vertices, fusion that changes the volume, undecided shares
    at most knn_field_statement.AMBIGUOUS_CAP, no field-growth knife edge);
  - every stage accepts its own output: frame() of the chain's records is empty;
  - the Tukey statement is the oracle's (orc_tukey_weights), and Statement.cost with it the oracle's initial and final cost;
  - every defect of dynfusion_statement.DEFECTS, planted into the stated side, makes the comparison of its case's chain fail
    (compose_right: on nodes that are rotated — see the statement's docstring).
And the C++ side of the dump's inputs: `test_host_dynfusion_frames` without arguments, and the parameter file the cases write
against the program's reader."""
import subprocess

import numpy as np
import pytest

import dynfusion_cases as C
import dynfusion_statement as DS
import warp_statement as WS
from knn_field_statement import AMBIGUOUS_CAP

_CHAINS = {}


def chain(name):
    if name not in _CHAINS:
        import oracle
        oracle.build()
        case = C.Case(name)
        depths = C.depths_of(name)
        _CHAINS[name] = (case, DS.chain_records(case, depths), depths, {})
    return _CHAINS[name]


def compare(ch, stages, defect=None, frames=None):
    case, recs, depths, infos = ch
    bad = []
    for i in (range(case.frames) if frames is None else frames):
        bad += DS.frame(recs[i - 1] if i else None, recs[i], dict(index=i, depth=depths[i]), case, defect=defect, stages=stages,
                        info=infos.setdefault(i, {}) if defect is None else {})
    return bad


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_stage_accepts_its_own_output_and_the_case_meets_its_conditions(name):
    ch = chain(name)
    case, recs, depths, infos = ch
    assert compare(ch, DS.STAGES) == []
    D = [r["D"] for r in recs]
    print(name, "nodes", D, "live vertices", [len(r["live_v"]) for r in recs])
    assert 30 <= D[0] <= 60 and any(b > a for a, b in zip(D, D[1:])), D
    for i, info in sorted(infos.items()):
        print(name, "frame", i, info)
        if not i:
            continue
        assert not info["growth_knife"]
        cost = info["cost"]
        assert cost["zero"] > 0.05 and cost["partial"] > 0.05 and cost["near"] <= AMBIGUOUS_CAP
        assert info["live_ties"] >= 0.1
        assert abs(recs[i]["oracle_costs"][0] - cost["initial"][1]) <= 1e-5 * cost["initial"][1]
        assert abs(recs[i]["oracle_costs"][1] - cost["final"][1]) <= 1e-5 * cost["final"][1]
        if case.fuse_canonical:
            assert info["fusion"]["changed"] >= 0.01 and info["fusion"]["undecided"] <= AMBIGUOUS_CAP
            assert info["fusion"]["unsupported_in_band"] >= 100
            assert info["fusion"]["unsupported_updated"] == (info["fusion"]["unsupported_in_band"] if case.fuse_unsupported_rigid else 0)


def test_some_case_has_a_frame_that_appends_nothing_before_a_frame_that_reuses_the_graph():
    found = []
    for name in C.CASES:
        D = [r["D"] for r in chain(name)[1]]
        found += [(name, i) for i in range(1, len(D) - 1) if D[i] == D[i - 1]]
    print(found)
    assert found
    what, stages, name = DS.DEFECTS["stale_graph"]
    D = [r["D"] for r in chain(name)[1]]
    assert any(D[i - 1] > D[i - 2] for i in range(2, len(D))), "no frame warps after a frame that appended nodes"


@pytest.mark.parametrize("k", [4, 8])
def test_the_tukey_statement_is_the_oracles(k):
    """dynfusion_statement.tukey (numpy, float64, from opt_solver.cpp:204-231) against orc_tukey_weights (float32): rows away from
    the cut-off within the float32 evaluation's error, rows at the cut-off within what the cut can carry"""
    import oracle
    oracle.build()
    c = WS.matrix_case(63, k, 2000)
    rng = np.random.default_rng(k)
    dq = WS.dq_from_euler(*np.zeros((3, 63)), *rng.uniform(-0.03, 0.03, (3, 63))).astype(np.float32)
    canon = c["verts"]
    live = (canon + rng.uniform(-0.04, 0.04, canon.shape)).astype(np.float32)
    live[::7] = canon[::7]  # rows of weight one (up to the warp)
    tau, d = DS.tukey(c["nodes"], dq, c["node_w"], k, canon, live, 4.652, 0.01)
    ref = oracle.tukey_weights(c["nodes"], dq, c["node_w"], k, canon, live, 4.652, 0.01)
    psi = float(np.float32(0.01))
    dd = (WS.ORACLE_DEVIATION * np.sqrt(3.0) + 4 * 2.0 ** -24 * 1.2) / 4.652 + 2 * 2.0 ** -24 * d
    bar = np.where(d < psi, 4 * (1 - d * d / psi ** 2) * d / psi ** 2 * dd, 0.0) + (2 * np.minimum(dd / psi, 1.0)) ** 2 + 4 * 2.0 ** -24
    print("k", k, "zero", float((tau == 0).mean()), "between", float(((tau > 0) & (tau < 1)).mean()), "worst", float(np.abs(tau - ref).max()),
          "worst / bar", float((np.abs(tau - ref) / bar).max()))
    assert (tau == 0).mean() > 0.05 and ((tau > 0) & (tau < 1)).mean() > 0.05
    assert (np.abs(tau - ref) <= bar).all()


def rotated(before, after, case):
    """a record pair for compose_right: every node of `before` rotated by 0.05 rad about the middle of the volume (composed on
    the left), t the oracle's solve from those nodes, the nodes of `after` the left composition DQ(0,0,0,t) * dq in float32 as
    the host forms it, the costs the statement's"""
    import oracle
    Db = before["D"]
    c = np.array([0.9, 0.9, 0.9])
    to, back = WS.dq_from_euler(0, 0, 0, *c), WS.dq_from_euler(0, 0, 0, *-c)
    rot = WS.dq_mul(to, WS.dq_mul(WS.dq_from_euler(0.05, 0.0, 0.0, 0.0, 0.0, 0.0), back))
    b, a = dict(before), dict(after)
    b["node_dq"] = WS.dq_mul(rot[None], before["node_dq"].astype(np.float64)).astype(np.float32)
    t = oracle.solve_ref(b["node_pos"], b["node_dq"], b["node_w"], case.k, a["corresponding_v"], a["live_v"], num_iter=1,
                         nonlinear_iter=case.solver_nonLinearIter, linear_iter=case.solver_linearIter, lambda_=float(np.float32(case.lambda_)), threads=8)[0]
    step = np.zeros((Db, 8))
    step[:, 0], step[:, 5:] = 1.0, 0.5 * t.astype(np.float64)
    a["node_dq"] = np.concatenate([WS.dq_mul(step, b["node_dq"].astype(np.float64)).astype(np.float32), after["node_dq"][Db:]])
    nd = (b["node_pos"], b["node_dq"], b["node_w"])
    S0, tau, d, idx = DS.solve_statement(nd, a["corresponding_v"], a["live_v"], case)
    a["initial_cost"] = S0.cost
    a["final_cost"] = DS.Statement(nd[0], nd[2], case.k, a["corresponding_v"], a["live_v"], idx, tau, float(np.float32(case.lambda_)),
                                   t=DS.recover_t(b["node_dq"], a["node_dq"][:Db])[0]).cost
    return b, a


def test_t_composed_on_the_right_shows_on_rotated_nodes():
    """every rotation of a reference-mode sequence is the identity, where left and right composition coincide: the defect is
    planted on a record whose nodes are rotated, and stage e must accept the left composition and refuse the right one"""
    case, recs, depths, _ = chain("plain")
    for i in range(1, case.frames):
        b, a = rotated(recs[i - 1], recs[i], case)
        inp = dict(index=i, depth=depths[i])
        assert DS.frame(b, a, inp, case, stages="e") == []
        bad = DS.frame(b, a, inp, case, stages="e", defect="compose_right")
        print("frame", i, bad)
        assert bad != []
    # ... and on the chain's own records (identity rotations) the two compositions are the same bits
    b, a = recs[1], recs[2]
    assert np.array_equal(DS.recover_t(b["node_dq"], a["node_dq"][:b["D"]])[0], DS.recover_t(b["node_dq"], a["node_dq"][:b["D"]], right=True)[0])
    assert all((r["node_dq"][:, :4] == np.array([1, 0, 0, 0], np.float32)).all() for r in recs)


@pytest.mark.parametrize("defect", [d for d in DS.DEFECTS if d != "compose_right"])  # (compose_right: the test above)
def test_a_planted_defect_changes_a_stage_by_more_than_its_bar(defect):
    what, stages, name = DS.DEFECTS[defect]
    ch = chain(name)
    bad = compare(ch, stages, defect=defect, frames=range(1, ch[0].frames))
    print(defect, "(%s):" % what, bad[:2])
    assert bad != []


def test_dump_program_reads_the_parameter_file_the_cases_write(tmp_path):
    """the no-GPU tests of the dump program, and its reader on every case's file: `params DIR` reads the file as `dump` does and
    prints every key back — each value the case wrote comes back as written, the reference-mode keys among them"""
    from dynfu_amd import build as B
    exe = B.build_cpp_tests()["test_host_dynfusion_frames"]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "2 tests, 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    parse = lambda text: {line.split()[0]: line.split()[1:] for line in text.splitlines()}
    for name in C.CASES:
        d = tmp_path / name
        d.mkdir()
        C.write_case(name, str(d))
        r = subprocess.run([exe, "params", str(d)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        wrote, read = parse(open(d / "params.txt").read()), parse(r.stdout)
        for key in ("fuse_canonical", "solver_numIter", "solver_nonLinearIter", "solver_linearIter", "warp_knn", "nodeStep", "epsilon", "frames"):
            assert key in wrote
        for key, vals in wrote.items():
            assert read[key] == vals, (name, key, vals, read[key])
    (tmp_path / "bad").mkdir()
    (tmp_path / "bad" / "params.txt").write_text("cols 96\nnonLinearIter 3\n")  # (the key carries its prefix: solver_nonLinearIter)
    assert subprocess.run([exe, "params", str(tmp_path / "bad")], capture_output=True, text=True, timeout=120).returncode == 2
