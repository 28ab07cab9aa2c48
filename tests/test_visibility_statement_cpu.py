"""CPU checks of tests/visibility_statement.py, the numpy statement the GPU test compares dfa_visible_vertices with: the
hand-worked answers of the edge_values case, and the two_planes case classified as its geometry says (the near quad
rasterised by the rasteriser's own statement)."""
import numpy as np

import raster_statement as R
import visibility_cases as C
from visibility_statement import visible_vertices


def test_edge_values_have_their_hand_worked_answers():
    store = C.edge_values_map()
    m = store[:, :C.EV["cols"]]
    for name, v, expected in C.edge_values_variants():
        flags, count = visible_vertices(v, m, *C.EV["intr"], C.EV["z_tol"])
        assert flags.dtype == np.uint8 and flags.shape == (len(v),), name
        assert np.array_equal(flags, expected), (name, np.flatnonzero(flags != expected))
        assert count == int(expected.sum()), name
    # both answers occur, and so does every way to a zero
    _, e = C.edge_values_vertices()
    assert 8 <= int(e.sum()) <= len(e) - 8


def test_edge_values_do_not_depend_on_the_padding():
    store = C.edge_values_map()
    v, expected = C.edge_values_vertices()
    packed = np.ascontiguousarray(store[:, :C.EV["cols"]])
    a, _ = visible_vertices(v, store[:, :C.EV["cols"]], *C.EV["intr"], C.EV["z_tol"])
    b, _ = visible_vertices(v, packed, *C.EV["intr"], C.EV["z_tol"])
    assert np.array_equal(a, b) and np.array_equal(a, expected)


def test_two_planes_are_classified_by_their_geometry():
    quad, idx = C.two_planes_quad()
    cols, rows = C.TP["cols"], C.TP["rows"]
    zbuf, points, _ = R.rasterize32(quad, None, idx, None, *C.TP["intr"], C.TP["z_near"], cols, rows)
    hit = zbuf != R.MISS
    assert hit[:, :C.TP["quad_cols"]].all() and not hit[:, C.TP["quad_cols"]:].any()  # the left 40 columns, all rows
    assert np.abs(points[hit][:, 2] - 1.0).max() < 1e-5
    verts, expected = C.two_planes_cloud()
    assert len(verts) == C.TP["n_plane"] + 4 and len(verts) % 64 and C.TP["n_plane"] % 64 and C.TP["n_plane"] % 256
    flags, count = visible_vertices(verts, points, *C.TP["intr"], C.TP["z_tol"])
    assert np.array_equal(flags, expected), np.flatnonzero(flags != expected)[:10]
    assert count == int(expected.sum())
    n = C.TP["n_plane"]
    assert 300 < int(expected[:n].sum()) < n - 300  # behind and beside, both well populated
    assert expected[n:].all()                         # the quad's own vertices
