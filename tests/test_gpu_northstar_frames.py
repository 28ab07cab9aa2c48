"""DynFusion::operator() in north-star mode on the device against the composed statement (tests/northstar_statement.py), frame
by frame and stage by stage.

Per case (tests/northstar_cases.py) the frames are written to a directory, `test_host_northstar_frames dump` runs DynFusion
over them ONCE as a child process and writes what every frame left behind; each stage is then stated from the device's own
recorded inputs (the record of frame i - 1 is frame i's "before"), so that a last bit in one stage does not cascade.  Stages
and bars: the docstring of tests/northstar_statement.py and profiles/northstar_frame_statement.md.  Every entry of
northstar_statement.DEFECTS, planted into the stated side, must make the comparison of its record fail.

The conditions a run must meet to prove anything are asserted on the device's record: knife-edge shares at most
knn_field_statement.AMBIGUOUS_CAP per frame and stage (inside frame()), at most one frame over all cases whose field growth
hangs on a knife-edge vertex, every case appends nodes in some frame, the regrown cloud outgrows frame 0's by a fifth, colour
weights reach their cap at frame 3, and the hidden share of the model lies between 5 % and 60 % in every frame from 1 on of
the two masked cases.  regrow_colour regrows at the weight floor 1: at floor 2 the cloud is what two frames BOTH saw, and the
empty frame 2 would start with it at the very pose it was last seen from, where nothing of it can be hidden."""
import os
import subprocess

import numpy as np
import pytest

import northstar_cases as C
import northstar_statement as NS

pytestmark = pytest.mark.gpu

_RUNS = {}
GROUPS = {"measured_and_levels": "ab", "rigid_visibility_cost": "cef", "warped_cloud_and_fusion": "gh", "regrow_and_growth": "ij"}
HIDDEN_FRAMES = {"aligned_visible_fused": (1, 2, 3), "regrow_colour": (1, 2, 3)}


@pytest.fixture(scope="module")
def exe():
    from dynfu_amd import build as B
    import oracle
    oracle.build()
    return B.build_cpp_tests()["test_host_northstar_frames"]


def run(exe, name, tmp_path_factory):
    """the dump of one case, made ONCE: a failed or faulted child is kept and raised again by every test of the case"""
    if name not in _RUNS:
        try:
            d = str(tmp_path_factory.mktemp("northstar_" + name))
            case = C.write_case(name, d)
            r = subprocess.run(["timeout", "-k", "10", "120", exe, "dump", d], capture_output=True, text=True, timeout=150)
            assert r.returncode == 0, "dump exit %d: %s %s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
            _RUNS[name] = (case, C.read_records(d, case), C.depths_of(name), C.colors_of(name), {})
        except Exception as e:  # noqa: BLE001  (a failed assertion, a child that timed out or could not be started)
            _RUNS[name] = e
    if isinstance(_RUNS[name], Exception):
        raise _RUNS[name]
    return _RUNS[name]


def inputs(i, depths, colors):
    return dict(index=i, depth=depths[i], color=colors[i], prev_color=colors[i - 1] if i else None)


def compare(run_, stages, defect=None, frames=None):
    case, recs, depths, colors, infos = run_
    key = (case.name, "".join(sorted(stages)))
    if defect is None and frames is None and key in _CLEAN:  # (the statement without a defect: computed once per stage group)
        return _CLEAN[key]
    bad = _compare(run_, stages, defect, frames)
    if defect is None and frames is None:
        _CLEAN[key] = bad
    return bad


_CLEAN = {}


def _compare(run_, stages, defect, frames):
    case, recs, depths, colors, infos = run_
    bad = []
    for i in (range(case.frames) if frames is None else frames):
        info = infos.setdefault(i, {}) if defect is None else {}
        bad += NS.frame(recs[i - 1] if i else None, recs[i], inputs(i, depths, colors), case, defect=defect, stages=stages, info=info)
    return bad


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("name", list(C.CASES))
def test_stages_against_the_statement(exe, tmp_path_factory, name, group):
    r = run(exe, name, tmp_path_factory)
    bad = compare(r, GROUPS[group])
    for i, info in sorted(r[4].items()):
        print(name, "frame", i, info)
    assert bad == []


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_run_has_something_to_show(exe, tmp_path_factory, name):
    case, recs, depths, colors, _ = run(exe, name, tmp_path_factory)
    assert [r["result"] for r in recs] == [False, True, True, True] and [r["counter"] for r in recs] == [1, 2, 3, 4]
    D = [r["D"] for r in recs]
    print(name, "nodes", D, "canonical vertices", [r["canonical_vertices"] for r in recs])
    assert 30 <= D[0] <= 60, D
    assert any(b > a for a, b in zip(D, D[1:])), "no frame appends nodes"
    for i in HIDDEN_FRAMES.get(name, ()):
        hidden = float((recs[i]["visible_flags"] == 0).mean())
        print(name, "frame", i, "hidden share %.4f" % hidden)
        assert 0.05 <= hidden <= 0.60, (i, hidden)
    if case.north_star_reg_hierarchy:
        assert all(sum(1 for n in r["level_counts"] if n) > 1 for r in recs[1:]), "one level only"
    if name == "plain":
        assert recs[1]["knn"] == 4
    if name == "regrow_colour":
        assert recs[3]["canonical_vertices"] >= 1.2 * recs[0]["canonical_vertices"]
        assert not depths[2].any() and recs[2]["rigid_skipped"] == recs[1]["rigid_skipped"] + 1 and recs[2]["valid_rows"] == 0
        assert NS.same(recs[2]["rigid_pose"], NS.K.IDENTITY)
        assert NS.same(recs[2]["canonical_volume"], recs[1]["canonical_volume"]) and NS.same(recs[2]["color_volume"], recs[1]["color_volume"])
        w = recs[3]["color_volume"] >> 24
        assert w.max() == case.canonical_max_color_weight == 3 and (w == 3).sum() > 100, "the cap does not bind by frame 3"


def test_growth_knife_edges_are_rare(exe, tmp_path_factory):
    knives = 0
    for name in C.CASES:
        r = run(exe, name, tmp_path_factory)
        compare(r, "j")
        knives += sum(1 for info in r[4].values() if info.get("growth_knife"))
    assert knives <= 1


@pytest.mark.parametrize("defect", list(NS.DEFECTS))
def test_a_planted_defect_fails_the_comparison(exe, tmp_path_factory, defect):
    what, stages, name = NS.DEFECTS[defect]
    r = run(exe, name, tmp_path_factory)
    assert compare(r, stages) == [], "the record does not pass without the defect"
    bad = compare(r, stages, defect=defect, frames=range(1, r[0].frames))
    print(defect, "(%s):" % what, len(bad), "failed checks;", bad[:2])
    assert bad != []


def test_write_up_figures(exe, tmp_path_factory):
    """the table of profiles/northstar_frame_statement.md: every solved frame has its figures, and prints them"""
    for name in C.CASES:
        r = run(exe, name, tmp_path_factory)
        case = r[0]
        compare(r, NS.STAGES)
        for i, info in sorted(r[4].items()):
            rg, cost = info.get("rigid"), info.get("cost")
            assert "nodes" in info
            if i:
                assert cost is not None and np.isfinite([cost["device"], cost["statement"], cost["budget"]]).all()
                assert (rg is not None) == bool(case.north_star_rigid_prealign and i not in C.EMPTY.get(name, ()))
                assert ("hidden" in info) == bool(case.north_star_visible_only)
            print("| %s | %d | %s | %s | %s | %s | %s |" % (
                name, i, "%.2e / %.2e / %.2e" % (rg["e32"], rg["gap"], rg["tol"]) if rg else "-",
                "%.9g / %.9g / %.2e" % (cost["device"], cost["statement"], cost["budget"]) if cost else "-",
                " ".join("%s %.4f" % (k[:6], info[k]) for k in ("raster_knife", "flags_undecided", "fusion_undecided", "colour_undecided",
                                                               "canonical_colors_undecided") if k in info)
                + (" solve %.4f" % cost["amb"] if cost else ""), "%s -> %s" % info.get("nodes", ("-", "-")),
                "%.4f" % info["hidden"] if "hidden" in info else "-"))
