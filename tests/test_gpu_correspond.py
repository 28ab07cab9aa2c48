"""-m gpu: dfa_correspond and dfa_correspond_projective against their numpy statements (tests/correspond_statement.py) on
the hand-placed cases of tests/correspond_cases.py — every grid dfa_correspond can build, every stage of
knn_grid_query<1, TIGHT> (csrc/knn_device.hpp), the thresholds between the search forms, and the edges of the projective
gates.  Every comparison is exact: indices, pixel numbers, or the bits of float32 values.

Not reachable through the C ABI: the exhaustive scan over 1 024 canonical points or more (want_grid takes the grid from
there on whatever the number of queries); it is checked on the hand-placed points alone, which are fewer."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import correspond_cases as Cc  # noqa: E402
import correspond_statement as S  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402

ORDERS = ("interleaved", "grouped", "ragged")


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


@functools.lru_cache(maxsize=None)
def _device_cloud(name):
    c = Cc.grid_case(name)
    return dev(c["canon"]), dev(c["normals"])


def _check(A, canon, normals, dcanon, dnormals, queries, want_idx, what):
    """one call with every output, compared with the statement; then the calls that leave outputs out"""
    dq = dev(queries)
    ov, on, idx = A.correspond(dcanon, dnormals, dq)
    got = host(idx)
    bad = np.flatnonzero(got != want_idx)
    assert len(bad) == 0, "%s: %d wrong neighbours, first at query %d %r: got %d, want %d" % (
        what, len(bad), bad[0], queries[bad[0]].tolist(), got[bad[0]], want_idx[bad[0]])
    wv, wn = S.gather(canon, normals, want_idx)
    assert np.array_equal(bits(host(ov)), bits(wv)) and np.array_equal(bits(host(on)), bits(wn)), what
    ov2, on2, idx2 = A.correspond(dcanon, None, dq)
    assert on2 is None and np.array_equal(host(idx2), want_idx) and np.array_equal(bits(host(ov2)), bits(wv)), what
    ov3, on3, idx3 = A.correspond(dcanon, dnormals, dq, want_index=False)
    assert idx3 is None and np.array_equal(bits(host(ov3)), bits(wv)) and np.array_equal(bits(host(on3)), bits(wn)), what


# ------------------------------------------------------------------------------------------ the grids, stage by stage
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(Cc.GRIDS))
def test_every_stage_of_the_grid_search_equals_the_statement(A, name, order):
    c = Cc.grid_case(name)
    sel = Cc.orders(name)[order]
    assert S.search_form(len(c["canon"]), len(sel)) == c["grid"].form
    want = Cc.expected(name)[0][sel]
    _check(A, c["canon"], c["normals"], *_device_cloud(name), c["queries"][sel], want, "%s, %s" % (name, order))


@pytest.mark.parametrize("name", sorted(Cc.GRIDS))
def test_the_exhaustive_scan_gives_the_same_answers_on_the_placed_points(A, name):
    """the hand-placed points without the filler are fewer than 1 024: the same queries take the exhaustive scan"""
    c = Cc.grid_case(name)
    canon, normals = c["canon"][c["placed"]], c["normals"][c["placed"]]
    for order in ORDERS:
        sel = Cc.orders(name)[order]
        assert S.search_form(len(canon), len(sel)) == "scan"
        queries = c["queries"][sel]
        want = S.nearest(canon, queries)[0]
        # where the plan names the answer it is a placed point: the same point, by its new number (a few class-8 queries
        # outside the z faces have a filler point as their nearest in the full cloud; the statement decides those)
        full = Cc.expected(name)[0][sel]
        known = c["target"][sel] >= 0
        assert np.array_equal(c["placed"][want[known]], full[known])
        _check(A, canon, normals, dev(canon), dev(normals), queries, want, "%s, %s, scan" % (name, order))


@pytest.mark.parametrize("name", sorted(Cc.GRIDS))
def test_a_grown_ball_that_scans_all_of_its_cells_again_finds_the_same(A, devlib, monkeypatch, name):
    """classes 5 and 6 (the ball of cells, grown or taken from a known point) with the first form of the growth as well:
    DFA_BALL_RESCAN=1 in the development library"""
    c = Cc.grid_case(name)
    sel = np.flatnonzero((c["cls"] == "5") | (c["cls"] == "6"))
    want = Cc.expected(name)[0][sel]
    dcanon, _ = _device_cloud(name)
    dq = dev(c["queries"][sel])
    for form in ("grow", "rescan"):
        if form == "rescan":
            monkeypatch.setenv("DFA_BALL_RESCAN", "1")
        else:
            monkeypatch.delenv("DFA_BALL_RESCAN", raising=False)
        _, _, idx = A.correspond(dcanon, None, dq)
        assert np.array_equal(host(idx), want), form
    monkeypatch.delenv("DFA_BALL_RESCAN")


# ------------------------------------------------------------------------------------------ between the forms
@pytest.mark.parametrize("n_canon,n_live,form", Cc.THRESHOLDS)
def test_both_sides_of_every_threshold_between_the_forms(A, n_canon, n_live, form):
    assert S.search_form(n_canon, n_live) == form
    canon, live = Cc.threshold_case(n_canon, n_live)
    want = S.nearest(canon, live)[0]
    ov, _, idx = A.correspond(dev(canon), None, dev(live))
    assert np.array_equal(host(idx), want)
    assert np.array_equal(bits(host(ov)), bits(canon[want]))


@pytest.mark.parametrize("pair", [("point_thin", "node_3d"), ("point_thin", "point_3d"), ("node_thin", "node_3d")],
                         ids=lambda p: "+".join(p))
def test_two_searches_in_flight_on_two_streams_from_one_thread(A, pair):
    """the grids are scratch kept per (device, stream), one object per kind of grid: two searches built and run on two
    streams by one host thread each equal their statement.  A point grid beside a node grid uses two scratch objects
    whatever the stream; the two pairs of ONE kind are the ones that would share a grid if the scratch were not kept per
    stream."""
    import torch
    sets = []
    for name in pair:
        c = Cc.grid_case(name)
        sel = Cc.orders(name)["interleaved"]
        sets.append((_device_cloud(name)[0], dev(c["queries"][sel]), Cc.expected(name)[0][sel]))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    out = [None, None]
    for rep in range(6):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                out[i] = A.correspond(sets[i][0], None, sets[i][1])[2]
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(host(out[i]), sets[i][2])


# ------------------------------------------------------------------------------------------ projective association
@pytest.mark.parametrize("cols,rows,principal", Cc.PROJECTIVE_CASES)
@pytest.mark.parametrize("pitched", [False, True])
def test_projective_association_equals_the_statement_bit_for_bit(A, cols, rows, principal, pitched):
    """every combination of vertex normals and normal map, the case's distance threshold and a threshold of zero; pitched:
    the maps are column slices of images twice as wide (row pitch 32 * cols bytes)"""
    import torch
    c = Cc.projective_case(cols, rows, principal)

    def device_map(m):
        if not pitched:
            return dev(m)
        wide = dev(np.concatenate([m, np.full_like(m, 7.0)], 1))
        view = wide[:, :cols]
        assert view.stride(0) == 8 * cols and not view.is_contiguous()
        return view

    dv, dn, dvm, dnm = dev(c["vertices"]), dev(c["normals"]), device_map(c["vmap"]), device_map(c["nmap"])
    for with_normals in (True, False):
        for with_nmap in (True, False):
            for thresh in (c["dist_thresh"], 0.0):
                args = (*c["intr"], thresh, c["min_cosine"])
                wv, wn, wp, tie = S.projective(c["vertices"], c["normals"] if with_normals else None, c["vmap"],
                                               c["nmap"] if with_nmap else None, *args)
                assert not tie.any()
                gv, gn, gp = A.correspond_projective(dv, dn if with_normals else None, dvm, dnm if with_nmap else None, *args)
                what = (with_normals, with_nmap, thresh)
                assert np.array_equal(host(gp), wp), what
                assert np.array_equal(bits(host(gv)), bits(wv)), what
                assert (gn is None) == (wn is None) and (gn is None or np.array_equal(bits(host(gn)), bits(wn))), what
    torch.cuda.synchronize()
