"""DynFusion::operator() in reference mode (north_star = 0) on the device against the composed statement
(tests/dynfusion_statement.py), frame by frame and stage by stage.

Per case (tests/dynfusion_cases.py) the frames are written to a directory, `test_host_dynfusion_frames dump` runs DynFusion
over them ONCE as a child process and writes what every frame left behind; each stage is then stated from the device's own
recorded inputs (the record of frame i - 1 is frame i's "before"), so that a last bit in one stage does not cascade.  Stages
and bars: the docstring of tests/dynfusion_statement.py and profiles/dynfusion_frame_statement.md.  Every entry of
dynfusion_statement.DEFECTS, planted into the stated side, must make the comparison of its record fail.

The conditions a run must meet to prove anything are asserted on the device's record (test_the_run_has_something_to_show,
test_a_cached_graph_is_reused): results False, True, True, True; 30 to 60 nodes after frame 0; every case appends nodes in some
frame; some case has a frame that appends none, followed by a frame whose warp reuses the cached graph; Tukey weights at 0 and
strictly between 0 and 1 in every solved frame; at least a tenth of the live vertices share their coordinates with a
lower-indexed one; the fusion changes at least 1 % of the voxels per frame, and at least a hundred voxels no node supports lie
where an integration would update them (Rigid does, Skip does not); undecided shares at most knn_field_statement.AMBIGUOUS_CAP per frame and stage.

compose_right: left and right composition are the same dual quaternion while every rotation is the identity, and in this mode
every rotation is (tests/dynfusion_statement.py's docstring).  The device's record therefore cannot show that defect: its test
asserts what the record can hold — the rotations are the identity, bit for bit, and the two recoveries of t agree, bit for bit —
and the comparison itself is made on rotated nodes by tests/test_dynfusion_statement_cpu.py."""
import subprocess

import numpy as np
import pytest

import dynfusion_cases as C
import dynfusion_statement as DS
from knn_field_statement import AMBIGUOUS_CAP

pytestmark = pytest.mark.gpu

_RUNS = {}
_CLEAN = {}
GROUPS = {"measured_and_live_cloud": "ab", "warp_and_correspondence": "cd", "solve": "e", "fusion": "f", "growth": "g"}


@pytest.fixture(scope="module")
def exe():
    from dynfu_amd import build as B
    import oracle
    oracle.build()
    return B.build_cpp_tests()["test_host_dynfusion_frames"]


def run(exe, name, tmp_path_factory):
    """the dump of one case, made ONCE: a failed or faulted child is kept and raised again by every test of the case"""
    if name not in _RUNS:
        try:
            d = str(tmp_path_factory.mktemp("dynfusion_" + name))
            case = C.write_case(name, d)
            r = subprocess.run(["timeout", "-k", "10", "120", exe, "dump", d], capture_output=True, text=True, timeout=150)
            assert r.returncode == 0, "dump exit %d: %s %s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
            _RUNS[name] = (case, C.read_records(d, case), C.depths_of(name), {}, C.read_derived(d))
        except Exception as e:  # noqa: BLE001  (a failed assertion, a child that timed out or could not be started)
            _RUNS[name] = e
    if isinstance(_RUNS[name], Exception):
        raise _RUNS[name]
    return _RUNS[name]


def compare(run_, stages, defect=None, frames=None):
    """the failed checks of the frames (all of them by default); without a defect a frame's stage group is stated once"""
    case, recs, depths, infos = run_[:4]
    bad = []
    for i in (range(case.frames) if frames is None else frames):
        key = (case.name, "".join(sorted(stages)), i)
        if defect is None and key in _CLEAN:
            bad += _CLEAN[key]
            continue
        info = infos.setdefault(i, {}) if defect is None else {}
        got = DS.frame(recs[i - 1] if i else None, recs[i], dict(index=i, depth=depths[i]), case, defect=defect, stages=stages, info=info)
        if defect is None:
            _CLEAN[key] = got
        bad += got
    return bad


@pytest.mark.parametrize("frame", range(C.FRAMES))
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("name", list(C.CASES))
def test_stages_against_the_statement(exe, tmp_path_factory, name, group, frame):
    r = run(exe, name, tmp_path_factory)
    bad = compare(r, GROUPS[group], frames=[frame])
    print(name, "frame", frame, r[3].get(frame))
    assert bad == []


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_run_has_something_to_show(exe, tmp_path_factory, name):
    r = run(exe, name, tmp_path_factory)
    case, recs, depths, infos = r[:4]
    trunc, voxel, max_weight = r[4]  # what the constructor derived from the parameters
    assert C.same(trunc, np.float32(case.kinfu.trunc)) and C.same(voxel, case.kinfu.voxel_size) and max_weight == case.kinfu.tsdf_max_weight
    assert [x["result"] for x in recs] == [False, True, True, True] and [x["counter"] for x in recs] == [1, 2, 3, 4]
    D = [x["D"] for x in recs]
    print(name, "nodes", D, "live vertices", [len(x["live_v"]) for x in recs])
    assert 30 <= D[0] <= 60, D
    assert any(b > a for a, b in zip(D, D[1:])), "no frame appends nodes"
    for stages in GROUPS.values():  # (stated once per group and frame: the stage tests' own)
        compare(r, stages)
    for i in range(1, case.frames):
        info = infos[i]
        cost = info["cost"]
        print(name, "frame", i, "Tukey: zero %.3f, between %.3f, at the cut-off %.4f; tied live vertices %.3f" %
              (cost["zero"], cost["partial"], cost["near"], info["live_ties"]))
        assert cost["zero"] > 0 and cost["partial"] > 0, "Tukey is not active"
        assert cost["near"] <= AMBIGUOUS_CAP
        assert info["live_ties"] >= 0.1
        if case.fuse_canonical:
            f = info["fusion"]
            print(name, "frame", i, "fusion", f)
            assert f["changed"] >= 0.01 and f["undecided"] <= AMBIGUOUS_CAP
            assert f["unsupported_in_band"] >= 100, "no voxel without support that an integration where it stands would update: Skip and Rigid agree"
            assert f["unsupported_updated"] == (f["unsupported_in_band"] if case.fuse_unsupported_rigid else 0)
            if case.fuse_knn_field:
                assert recs[i]["knn_field_k"] == case.k and recs[i]["knn_field_nodes"] == recs[i - 1]["D"]


def test_a_cached_graph_is_reused(exe, tmp_path_factory):
    """some case has a frame that appends no node, followed by a frame: that frame's warp finds the cloud, N, D and k of the
    call before and reuses its graph — Warpfield::warpGraphSearches does not move over it, and moves by one over every other
    solved frame (stage c asserts the count frame by frame)"""
    found = []
    for name in C.CASES:
        recs = run(exe, name, tmp_path_factory)[1]
        D = [x["D"] for x in recs]
        S = [x["warp_graph_searches"] for x in recs]
        print(name, "nodes", D, "k-NN searches of the warp so far", S)
        assert S[0] == 0 and S[1] == 1
        for i in range(2, len(D)):
            assert S[i] - S[i - 1] == (0 if D[i - 1] == D[i - 2] else 1), (name, i)
            if S[i] == S[i - 1]:
                found.append((name, i))
    print("frames that warp with the cached graph:", found)
    assert found


def test_growth_knife_edges_are_rare(exe, tmp_path_factory):
    knives = 0
    for name in C.CASES:
        r = run(exe, name, tmp_path_factory)
        compare(r, GROUPS["growth"])
        knives += sum(1 for info in r[3].values() if info.get("growth_knife"))
    assert knives <= 1


@pytest.mark.parametrize("defect", [d for d in DS.DEFECTS if d != "compose_right"])
def test_a_planted_defect_fails_the_comparison(exe, tmp_path_factory, defect):
    what, stages, name = DS.DEFECTS[defect]
    r = run(exe, name, tmp_path_factory)
    bad = []
    for i in range(1, r[0].frames):  # up to the first frame that shows it
        assert compare(r, stages, frames=[i]) == [], "the record does not pass without the defect"
        bad = compare(r, stages, defect=defect, frames=[i])
        if bad:
            break
    print(defect, "(%s):" % what, len(bad), "failed checks;", bad[:2])
    assert bad != []


def test_t_composed_on_the_right_is_the_left_composition_on_this_record(exe, tmp_path_factory):
    """compose_right (the module's docstring): the record's rotations are the identity, bit for bit, so that the defect and the
    adaptor's composition state the same nodes; stage e passes either way.  tests/test_dynfusion_statement_cpu.py plants the
    defect on rotated nodes, where it fails the comparison."""
    what, stages, name = DS.DEFECTS["compose_right"]
    r = run(exe, name, tmp_path_factory)
    case, recs = r[:2]
    assert compare(r, stages) == []
    identity = np.array([1, 0, 0, 0], np.float32)
    for i in range(1, case.frames):
        b, a = recs[i - 1], recs[i]
        assert all(C.same(q, identity) for q in a["node_dq"][:, :4])
        left, right = (DS.recover_t(b["node_dq"], a["node_dq"][:b["D"]], right=side)[0] for side in (False, True))
        assert np.array_equal(left, right) and np.abs(left).max() > 1e-3
    assert compare(r, stages, defect="compose_right", frames=range(1, case.frames)) == []


def test_write_up_figures(exe, tmp_path_factory):
    """the table of profiles/dynfusion_frame_statement.md: every solved frame has its figures, and prints them"""
    for name in C.CASES:
        r = run(exe, name, tmp_path_factory)
        case = r[0]
        for stages in GROUPS.values():
            compare(r, stages)
        for i, info in sorted(r[3].items()):
            assert "nodes" in info
            if not i:
                print("| %s | 0 | - | - | - | - | - | %s -> %s |" % (name, *info["nodes"]))
                continue
            cost, w = info["cost"], info["warped"]
            assert np.isfinite([*cost["initial"], *cost["final"]]).all()
            assert ("fusion" in info) == bool(case.fuse_canonical)
            print("| %s | %d | %.2e / %.2e / %.2e%s | %.9g / %.9g / %.2e | %.9g / %.9g / %.2e | zero %.3f between %.3f cut-off %.4f ties %.3f | %s | %s -> %s |" % (
                name, i, w["vertices"], w["normals"], w["bound"], " (cached graph, no search)" if w["reused_graph"] and not w["searched"] else "", *cost["initial"], *cost["final"],
                cost["zero"], cost["partial"], cost["near"], info["live_ties"],
                "changed %.4f undecided %.5f" % (info["fusion"]["changed"], info["fusion"]["undecided"]) if "fusion" in info else "-", *info["nodes"]))
