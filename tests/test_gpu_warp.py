"""-m gpu parity tests of the warp-field seam (k-NN graph, RBF weights, DQ warp) vs the oracle.

Bar: k-NN indices bit-exact (integer work); weights within 1 float ulp (double exp on two
different libms, rounded to float); warped vertices within 2e-6 m absolute (float DQ algebra
with identical operation order, exp as above)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
import reference_data  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _ulp_diff(a, b):
    ia = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("D,k,n", [(2048, 4, 20000), (500, 8, 5000), (3000, 16, 3000), (5, 8, 100), (1, 4, 10),
                                    (1025, 5, 777)])
def test_knn_bit_exact_and_weights(A, D, k, n):
    rng = np.random.default_rng(D + k)
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = rng.uniform(0.05, 0.5, D).astype(np.float32)
    q = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    q[: min(n, D)] = nodes[: min(n, D)]  # queries sitting exactly on nodes (distance 0)
    idx, w = A.knn(dev(nodes), dev(node_w), dev(q), k)
    ref = O.knn(nodes, q, k, threads=8)
    assert np.array_equal(host(idx), ref)
    wref = np.zeros((n, k), np.float32)
    for v in range(0, n, max(1, n // 500)):
        for j in range(k):
            if ref[v, j] >= 0:
                wref[v, j] = O.transformation_weight(nodes[ref[v, j]], float(node_w[ref[v, j]]), q[v])
        assert _ulp_diff(host(w)[v], wref[v]).max() <= 1
    assert np.all(host(w)[ref < 0] == 0)


def test_knn_on_two_streams_from_one_thread(A):
    # the search grid of dfa_knn is internal scratch kept per (device, stream): two searches in flight on two streams,
    # driven by ONE host thread, over different node sets must not see each other's grid
    import torch
    rng = np.random.default_rng(3)
    sets = []
    for i in range(2):
        D, n = 1500 + 700 * i, 40000
        nodes = rng.uniform(-1 - i, 1 + i, (D, 3)).astype(np.float32)
        q = rng.uniform(-1 - i, 1 + i, (n, 3)).astype(np.float32)
        sets.append((dev(nodes), dev(np.full(D, 0.1, np.float32)), dev(q), O.knn(nodes, q, 4, threads=8)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    out = [None, None]
    for rep in range(6):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                out[i] = A.knn(sets[i][0], sets[i][1], sets[i][2], 4)[0]
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(host(out[i]), sets[i][3])


@pytest.mark.parametrize("kind", ["clustered", "planar", "far_queries", "duplicates", "line", "lattice", "hand_placed"])
@pytest.mark.parametrize("k", [4, 8])
def test_knn_grid_path_is_exact_on_awkward_geometry(A, kind, k):
    # sizes above the grid threshold (D * n >= 2^22); the uniform grid must return exactly the
    # exhaustive (distance, index)-ordered answer whatever the node distribution
    if kind == "hand_placed":
        # the 32 x 32 x 4 node grid of tests/correspond_cases.py with the queries next to walls, edges and corners of their
        # cells, exactly on walls, and outside the grid — against the numpy statement.  Once as they are (few queries: one
        # wave per query) and once repeated beyond 32 768 (one lane per query: knn_grid_query<K>, which shares cell_of,
        # scan_block3 and the shell stop rule with the 1-NN search of dfa_correspond).
        import correspond_cases as Cc
        import warp_statement as W
        c = Cc.grid_case("node_3d")
        q = c["queries"][np.isin(c["cls"], ("2", "4", "8"))]
        want = W.knn(c["canon"], q, k)
        dn, dw = dev(c["canon"]), dev(np.full(len(c["canon"]), 0.3, np.float32))
        assert np.array_equal(host(A.knn(dn, dw, dev(q), k)[0]), want)
        rep = np.resize(np.arange(len(q)), 32768 + 64 + 1)
        assert np.array_equal(host(A.knn(dn, dw, dev(q[rep]), k)[0]), want[rep])
        return
    rng = np.random.default_rng(hash(kind) % 1000 + k)
    D, n = 1500, 6000
    q = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    if kind == "clustered":
        centres = rng.uniform(-1, 1, (6, 3))
        nodes = (centres[rng.integers(0, 6, D)] + rng.normal(0, 0.01, (D, 3))).astype(np.float32)
    elif kind == "planar":
        nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
        nodes[:, 2] = 0.25  # zero extent along z
    elif kind == "far_queries":
        nodes = rng.uniform(-0.1, 0.1, (D, 3)).astype(np.float32)
        q = (q * 50).astype(np.float32)  # far outside the node bounding box
    elif kind == "duplicates":
        nodes = np.repeat(rng.uniform(-1, 1, (D // 10, 3)), 10, axis=0).astype(np.float32)
    elif kind == "line":
        nodes = np.zeros((D, 3), np.float32)
        nodes[:, 0] = np.linspace(-1, 1, D)
    else:  # integer lattice: massive exact ties
        g = np.stack(np.meshgrid(*[np.arange(12.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
        nodes = g[:D].astype(np.float32)
        q = rng.integers(0, 12, (n, 3)).astype(np.float32) + np.float32(0.5)
    idx, _ = A.knn(dev(nodes), dev(np.full(len(nodes), 0.3, np.float32)), dev(q), k)
    assert np.array_equal(host(idx), O.knn(nodes, q, k, threads=8))


def test_knn_exact_ties_keep_lower_index(A):
    # integer lattice: many exactly equal distances
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    q = (g[::5] + np.float32(0.5)).astype(np.float32)
    idx, _ = A.knn(dev(g), dev(np.ones(len(g), np.float32)), dev(q), 8)
    assert np.array_equal(host(idx), O.knn(g, q, 8))


@pytest.mark.parametrize("name", ["T0", "T1"])
def test_warp_to_live_matches_oracle(A, name):
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    D, k = cfg["D"], cfg["k"]
    rng = np.random.default_rng(5)
    # general rigid node transforms (rotation + translation), not only the solver's translations
    dq = np.stack([O.dq_from_euler(*rng.uniform(-0.2, 0.2, 3), *rng.uniform(-0.05, 0.05, 3)) for _ in range(D)])
    verts, normals = c["verts"][:20000], c["normals"][:20000]
    ov, on = A.warp_to_live(dev(c["node_pos"]), dev(dq), dev(c["node_w"]), k, dev(verts), dev(normals))
    rv, rn = O.warp_to_live(c["node_pos"], dq, c["node_w"], k, verts, normals, threads=8)
    np.testing.assert_allclose(host(ov), rv, atol=2e-6, rtol=0)
    np.testing.assert_allclose(host(on), rn, atol=2e-6, rtol=0)
    # identity transforms warp nothing
    ov, _ = A.warp_to_live(dev(c["node_pos"]), dev(c["node_dq"]), dev(c["node_w"]), k, dev(verts))
    assert np.array_equal(host(ov), verts)


@pytest.mark.parametrize("name", ["T1", "C1"])
def test_warp_with_a_given_graph_equals_the_warp_that_searches(A, name):
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    D, k = cfg["D"], cfg["k"]
    rng = np.random.default_rng(9)
    dq = np.stack([O.dq_from_euler(*rng.uniform(-0.2, 0.2, 3), *rng.uniform(-0.05, 0.05, 3)) for _ in range(D)])
    verts, normals = c["verts"], c["normals"]
    args = (dev(c["node_pos"]), dev(dq), dev(c["node_w"]))
    ov, on = A.warp_to_live(*args, k, dev(verts), dev(normals))
    idx, _ = A.knn(args[0], args[2], dev(verts), k)
    gv, gn = A.warp_to_live_graph(*args, idx, dev(verts), dev(normals))
    assert np.array_equal(bits(host(gv)), bits(host(ov))) and np.array_equal(bits(host(gn)), bits(host(on)))


def test_warp_empty_and_errors(A):
    import torch
    nodes = torch.zeros((4, 3), device="cuda")
    dq = torch.zeros((4, 8), device="cuda")
    w = torch.ones(4, device="cuda")
    ov, _ = A.warp_to_live(nodes, dq, w, 4, torch.zeros((0, 3), device="cuda"))
    assert ov.shape == (0, 3)
    with pytest.raises(A.DynfuAmdError):
        A.knn(nodes, w, torch.zeros((3, 3), device="cuda"), 17)


# ------------------------------------------------------------------ correspondence (dyn_fusion.cpp:212-242)
@pytest.mark.parametrize("n_canon,n_live", reference_data.CORRESPOND_CASES)
def test_correspond_bit_exact(A, n_canon, n_live):
    cv, cn, lv = reference_data.correspond_clouds(n_canon, n_live)  # (half of the live points are exact hits)
    ov, on, idx = A.correspond(dev(cv), dev(cn), dev(lv))
    rv, rn, ridx = O.correspond(cv, cn, lv, threads=8)
    assert np.array_equal(host(idx), ridx)
    assert np.array_equal(host(ov), rv) and np.array_equal(host(on), rn)
    # the reference's own KD-tree (nanoflann: tests/golden/ref_knn.npz) agrees wherever the nearest point is unique
    nq = reference_data.CORRESPOND_QUERIES
    ref = reference_data.knn("correspond_%d_%d" % (n_canon, n_live), cv, lv[:nq], 1)[:, 0]
    d = ((lv[:nq].astype(np.float64) - cv[ref].astype(np.float64)) ** 2).sum(1)
    dm = ((lv[:nq].astype(np.float64) - rv[:nq].astype(np.float64)) ** 2).sum(1)
    assert np.all((ref == ridx[:nq]) | (np.abs(d - dm) <= 1e-12))


@pytest.mark.parametrize("n,shift_cells", [(120000, 1.6), (120000, 2.7), (600000, 2.2), (120000, 6.0)])
def test_correspond_a_surface_that_has_moved_by_cells(A, n, shift_cells):
    """A live surface one to a few grid cells away from the canonical one (along its normal: the 3 x 3 x 3 block of a query
    is then empty or holds only far points): the search leaves shells 0 / 1 and takes the exact ball of cells around the
    query (up to four cells of reach) or, beyond that, the shell walk.  Same indices as the oracle's exhaustive scan."""
    cv, cn, lv = reference_data.surface_clouds(n, 40000, n + int(10 * shift_cells))
    # the grid's cell size as pgrid_finalize_kernel picks it: the cap of 128 (256 above half a million points) cells per axis
    ext = cv.max(0) - cv.min(0)
    cs = max((0.5 if n > 500000 else 0.7) * float(np.cbrt(ext.prod() / n)), float(ext.max()) / (256 if n > 500000 else 128))
    d = lv - synth.SPHERE_C
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rng = np.random.default_rng(3)
    lv = (lv + d * (shift_cells * cs * rng.uniform(0.6, 1.0, (len(lv), 1)))).astype(np.float32)
    _, _, idx = A.correspond(dev(cv), None, dev(lv))
    _, _, ridx = O.correspond(cv, None, lv, threads=8)
    assert np.array_equal(host(idx), ridx)


def test_correspond_a_sparse_neighbourhood_grows_its_ball_without_scanning_it_again(A, devlib, monkeypatch):
    """Queries two to four cells away from the cloud find their 3 x 3 x 3 block EMPTY: the ball of cells starts at two cells
    and grows by one until it holds a point, and a grown ball scans only what the larger radius adds (the first
    form scanned the whole ball again on every growth — DFA_BALL_RESCAN=1 in the development library keeps it).  Same indices
    as the oracle's exhaustive scan and as the first form; not slower than it."""
    import torch
    n = 600000
    cv, cn, lv = reference_data.surface_clouds(n, 200000, n + 5)
    ext = cv.max(0) - cv.min(0)
    cs = max(0.5 * float(np.cbrt(ext.prod() / n)), float(ext.max()) / 256)
    d = lv - synth.SPHERE_C
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rng = np.random.default_rng(9)
    lv = (lv + d * (cs * rng.uniform(2.2, 4.4, (len(lv), 1)))).astype(np.float32)  # every block empty, two to three growths
    _, _, ridx = O.correspond(cv, None, lv, threads=8)
    dcv, dlv = dev(cv), dev(lv)
    ms = {}
    for form in ("grow", "rescan"):
        if form == "rescan":
            monkeypatch.setenv("DFA_BALL_RESCAN", "1")
        _, _, idx = A.correspond(dcv, None, dlv)
        assert np.array_equal(host(idx), ridx), form
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            A.correspond(dcv, None, dlv)
        e1.record()
        torch.cuda.synchronize()
        ms[form] = e0.elapsed_time(e1) / 5
    monkeypatch.delenv("DFA_BALL_RESCAN")
    assert ms["grow"] <= 1.1 * ms["rescan"], ms


def test_correspond_a_million_points_against_the_reference_kd_tree(A):
    """Clouds of more than half a million points switch to the finer grid (up to 256 cells per axis): a million canonical
    points on the synthetic surface, checked against the reference's own nanoflann KD-tree (tests/golden/ref_knn.npz) on
    60 000 queries and by the defining property on all of them (no canonical point of a random sample is closer than the
    one returned)."""
    cv, cn, lv = reference_data.surface_clouds(*reference_data.MILLION)
    ov, on, idx = A.correspond(dev(cv), dev(cn), dev(lv))
    idx_h, ov_h = host(idx), host(ov)
    assert np.array_equal(ov_h, cv[idx_h]) and np.array_equal(host(on), cn[idx_h])
    d_ret = ((lv.astype(np.float64) - ov_h.astype(np.float64)) ** 2).sum(1)
    rng = np.random.default_rng(1)
    for _ in range(4):  # random canonical points are never closer than the returned one
        cand = cv[rng.integers(0, len(cv), len(lv))]
        assert np.all(((lv.astype(np.float64) - cand.astype(np.float64)) ** 2).sum(1) >= d_ret - 1e-12)
    nq = reference_data.MILLION_QUERIES
    r = reference_data.knn("correspond_million", cv, lv[:nq], 1)[:, 0]
    d_ref = ((lv[:nq].astype(np.float64) - cv[r].astype(np.float64)) ** 2).sum(1)
    assert np.all((r == idx_h[:nq]) | (np.abs(d_ref - d_ret[:nq]) <= 1e-12))
    assert (r == idx_h[:nq]).mean() > 0.999


def test_correspond_duplicates_optional_outputs_and_errors(A):
    import torch
    cv = np.tile(np.array([[0, 0, 1], [0.5, 0, 1], [0, 0, 1]], np.float32), (50, 1))  # every point 50 (or 100) times
    lv = np.array([[0, 0, 1.01], [0.4, 0, 1], [9, 9, 9]], np.float32)
    ov, on, idx = A.correspond(dev(cv), None, dev(lv))
    assert on is None and host(idx).tolist() == [0, 1, 1]  # ties -> lowest index
    assert np.array_equal(host(ov), cv[[0, 1, 1]])
    ov, on, idx = A.correspond(dev(cv), dev(cv), torch.zeros((0, 3), device="cuda"))
    assert ov.shape == (0, 3) and idx.shape == (0,)
    with pytest.raises(A.DynfuAmdError):
        A.correspond(torch.zeros((0, 3), device="cuda"), None, dev(lv))


@pytest.mark.parametrize("kind", ["planar", "coincident", "clustered_far", "lattice", "line", "volume"])
def test_correspond_point_grid_is_exact_on_awkward_geometry(A, kind):
    rng = np.random.default_rng(11)
    n = 30000
    if kind == "planar":
        cv = np.c_[rng.uniform(-1, 1, (n, 2)), np.full(n, 1.25)]
    elif kind == "coincident":
        cv = np.tile([[0.25, -0.5, 2.0]], (n, 1))
    elif kind == "clustered_far":
        cv = np.r_[rng.normal(0, 0.01, (n - 10, 3)), rng.uniform(50, 60, (10, 3))]
    elif kind == "lattice":  # many exactly equidistant candidates
        g = np.arange(31) * 0.125
        cv = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    elif kind == "line":
        cv = np.c_[np.linspace(-3, 3, n), np.zeros(n), np.zeros(n)]
    else:
        cv = rng.uniform(-1, 1, (n, 3))
    cv = cv.astype(np.float32)
    lo, hi = cv.min(0), cv.max(0)
    lv = np.r_[rng.uniform(lo - 0.3, hi + 0.3, (3000, 3)), cv[::50] + 0.0625,  # lattice: cell centres
               rng.uniform(-100, 100, (200, 3))].astype(np.float32)
    _, _, idx = A.correspond(dev(cv), None, dev(lv))
    _, _, ridx = O.correspond(cv, None, lv, threads=8)
    assert np.array_equal(host(idx), ridx)


# ------------------------------------------------------------- node insertion pieces (warp_field.cpp:34-95)
@pytest.mark.parametrize("D,k,n", [(300, 8, 20000), (2048, 8, 60000), (3, 8, 500), (8192, 8, 150000), (4096, 4, 50000)])
def test_unsupported_vertices_and_calc_dqb_match_the_oracle(A, D, k, n):
    rng = np.random.default_rng(D)
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = rng.uniform(0.05, 0.3, D).astype(np.float32)
    verts = rng.uniform(-1.3, 1.3, (n, 3)).astype(np.float32)
    verts[:D] = nodes  # distance 0: supported
    flags = host(A.unsupported_vertices(dev(nodes), dev(node_w), k, dev(verts)))
    ref = O.unsupported_flags(nodes, node_w, k, verts, threads=8)
    assert np.array_equal(flags, ref) and 0 < ref.mean() < 1 and not ref[:D].any()
    # blended transforms at the first points
    dq = np.zeros((D, 8), np.float32)
    for i in range(D):
        dq[i] = O.dq_from_euler(*rng.uniform(-0.3, 0.3, 3), *rng.uniform(-0.05, 0.05, 3))
    m = min(n, 400)
    got = host(A.calc_dqb(dev(nodes), dev(dq), dev(node_w), k, dev(verts[:m])))
    want = np.stack([O.calc_dqb(nodes, dq, node_w, k, verts[i]) for i in range(m)])
    assert np.abs(got - want).max() < 2e-6


def test_unsupported_vertices_without_nodes(A):
    import torch
    v = torch.zeros((7, 3), device="cuda")
    assert host(A.unsupported_vertices(None, None, 8, v)).tolist() == [1] * 7  # min stays HUGE_VALF (:40,:53)


# ------------------------------------------------------------- projective association
def _live_maps(cfg, frame):
    fx, fy, cx, cy = synth.intrinsics(cfg)
    P, Nm = O.points_normals(synth.depth_frame(cfg, frame), fx, fy, cx, cy)
    return (fx, fy, cx, cy), P, Nm


@pytest.mark.parametrize("name,with_normals", [("T1", True), ("T1", False), ("C1", True)])
def test_correspond_projective_bit_exact(A, name, with_normals):
    """dfa_correspond_projective vs the oracle's find_coresp gates: the canonical cloud of the synthetic scene against
    the vertex / normal maps of a later frame, plus vertices behind the camera, outside the image and on the far plane"""
    cfg = synth.CONFIGS[name]
    c = synth.canonical(cfg)
    intr, P, Nm = _live_maps(cfg, 5)
    extra = np.array([[0, 0, -1], [0, 0, 0], [50, 0, 1], [0, -50, 1], [0.01, 0.01, 2.5], [np.nan, 0, 1]], np.float32)
    v = np.concatenate([c["verts"], extra]).astype(np.float32)
    n = np.concatenate([c["normals"], np.tile([[0, 0, -1]], (len(extra), 1))]).astype(np.float32)
    args = (intr[0], intr[1], intr[2], intr[3], 0.05, 0.7)
    rv, rn, rp = O.correspond_projective(v, n if with_normals else None, P, Nm, *args)
    gv, gn, gp = A.correspond_projective(dev(v), dev(n) if with_normals else None, dev(P), dev(Nm), *args)
    assert np.array_equal(host(gp), rp)
    assert np.array_equal(bits(host(gv)), bits(rv)) and np.array_equal(bits(host(gn)), bits(rn))
    matched = rp >= 0
    assert 0.5 * len(c["verts"]) < matched.sum() < len(v)          # most of the visible surface is associated
    assert (rp[-6:-2] == -1).all() and rp[-1] == -1                # behind / outside / NaN: no association
    assert np.isnan(rv[~matched]).all() and np.isfinite(rv[matched]).all()
    # every association obeys the gates
    assert (np.linalg.norm(rv[matched] - v[matched], axis=1) <= 0.05 * (1 + 1e-6)).all()
    if with_normals:
        assert (np.abs(np.sum(rn[matched] * n[matched], axis=1)) >= 0.7 - 1e-6).all()
    # without a normal map: vertices only
    gv2, gn2, gp2 = A.correspond_projective(dev(v), None, dev(P), None, *args)
    rv2, _, rp2 = O.correspond_projective(v, None, P, None, *args)
    assert gn2 is None and np.array_equal(host(gp2), rp2) and np.array_equal(bits(host(gv2)), bits(rv2))


def test_correspond_projective_errors(A):
    import torch
    P = torch.zeros((4, 4, 4), device="cuda")
    v = torch.zeros((3, 3), device="cuda")
    with pytest.raises(A.DynfuAmdError):
        A.correspond_projective(v, None, P, None, 0.0, 1.0, 0.0, 0.0, 0.1, 0.5)  # fx = 0
    ov, on, pix = A.correspond_projective(torch.zeros((0, 3), device="cuda"), None, P, None, 1.0, 1.0, 0.0, 0.0, 0.1, 0.5)
    assert ov.shape == (0, 3) and pix.shape == (0,)


# ---- point-cloud plumbing between the seams (csrc/points.hip): bit copies, checked against numpy
@pytest.mark.parametrize("n", [0, 1, 63, 4096, 4097, 100003])
@pytest.mark.parametrize("ss,ds", [(4, 3), (3, 4), (3, 3), (4, 4), (5, 7)])
def test_repack_points_is_a_bit_copy_of_xyz(A, n, ss, ds):
    rng = np.random.default_rng(n + ss)
    src = rng.standard_normal((n, ss)).astype(np.float32)
    if n:
        src[0, :3] = [np.nan, -0.0, np.inf]
    out = host(A.repack_points(dev(src), ds, pad=1.0)) if n else np.zeros((0, ds), np.float32)
    assert out.shape == (n, ds)
    assert np.array_equal(bits(out[:, :3]), bits(src[:, :3]))
    assert np.all(out[:, 3:] == 1.0)


@pytest.mark.parametrize("n,density", [(0, 0.5), (1, 1.0), (15, 0.5), (4096, 0.0), (4096, 1.0), (4097, 0.01), (70001, 0.3),
                                        (1 << 20, 0.001), (3 * (1 << 20) + 5, 0.5)])
def test_compact_points_keeps_flagged_points_in_index_order(A, n, density):
    import torch
    rng = np.random.default_rng(n)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    flags = (rng.random(n) < density).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)  # any non-zero value counts
    out, idx = A.compact_points(dev(pts) if n else None, dev(flags) if n else torch.zeros(0, dtype=torch.uint8, device="cuda"))
    want = np.flatnonzero(flags)
    assert np.array_equal(host(idx), want.astype(np.int32))
    assert np.array_equal(bits(host(out)), bits(pts[want]))
    # a flag array that does not start on a 16-byte boundary (the kernel's wide loads must not assume it)
    if n > 100:
        f2 = dev(flags)[3:]
        out2, idx2 = A.compact_points(dev(pts[3:]), f2)
        assert np.array_equal(host(idx2), np.flatnonzero(flags[3:]).astype(np.int32))


@pytest.mark.parametrize("n", [1, 257, 100003])
def test_transform_points_matches_the_host_loop_bit_for_bit(A, n):
    from gpu_util import rot
    rng = np.random.default_rng(n)
    p = rng.standard_normal((n, 3)).astype(np.float32)
    R = rot([0.3, -1.0, 0.5], 0.7).astype(np.float32)
    t = np.array([-1.5, -1.5, 0.5], np.float32)
    aff = np.concatenate([R.reshape(-1), t])
    for with_t in (True, False):
        out = host(A.transform_points(dev(p), aff, with_t))
        ref = np.stack([(R[c, 0] * p[:, 0] + R[c, 1] * p[:, 1]) + R[c, 2] * p[:, 2] for c in range(3)], 1)
        if with_t:
            ref = ref + t
        assert np.array_equal(bits(out), bits(ref.astype(np.float32)))


# ------------------------------------------------------------------------------------------------------------------------
# Against tests/warp_statement.py: the k-NN contract and the support flags stated in numpy (exact), the blend and the warp
# stated in fp64 (the mathematical statement, not the oracle's float32 copy of the kernels' operation order).
import warp_statement as WS  # noqa: E402

# Twice the float32 oracle's own largest deviation from the fp64 statement over WS.MATRIX, the inputs below (measured on
# the CPU: 8.783e-07 m, recorded as 9.0e-07 in warp_statement.ORACLE_DEVIATION and measured again by
# tests/test_warp_statement_cpu.py): 1.8e-06.  Kernel and oracle share the operation order and differ by exp's last bit.
WARP_BOUND = WS.KERNEL_BOUND


@pytest.mark.parametrize("D,k,n", [(2048, 4, 20000), (500, 8, 5000), (3000, 16, 3000), (5, 8, 100), (1, 4, 10), (1025, 5, 777)]
                         + [(300, k, n) for k in (1, 3, 7, 9, 16) for n in (2000, 40000)]   # brute force | grid, a lane per query
                         + [(1500, k, 3000) for k in (1, 3, 7, 9, 16)]                        # grid, a wave per query
                         + [(63, 9, 70000), (64, 9, 65535), (64, 9, 65536), (1023, 3, 4000), (1024, 3, 4000)])  # want_grid's edges
def test_knn_and_weights_equal_the_statement(A, D, k, n):
    rng = np.random.default_rng(D + k)
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = rng.uniform(0.05, 0.5, D).astype(np.float32)
    q = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    q[: min(n, D)] = nodes[: min(n, D)]
    q[-1, 1] = np.nan  # a NaN query: no neighbour
    idx, w = A.knn(dev(nodes), dev(node_w), dev(q), k)
    ref = WS.knn(nodes, q, k)
    assert (ref[-1] == -1).all()
    assert np.array_equal(host(idx), ref)
    wref = WS.weights(nodes, node_w, q, ref)
    assert _ulp_diff(host(w)[ref >= 0], wref[ref >= 0]).max() <= 1
    assert np.all(host(w)[ref < 0] == 0)


@pytest.mark.parametrize("D", WS.D_LIST)
@pytest.mark.parametrize("k", WS.K_LIST)
def test_warp_shape_matrix_against_the_fp64_statement(A, D, k):
    """dfa_warp_to_live, dfa_warp_to_live_graph and dfa_calc_dqb at every (D, k), K = 16 instantiations and k below the
    template's K included, D < k (absent neighbours), brute force and grid: within WARP_BOUND of the fp64 statement;
    the graph form bit-equal to the searching form — also with an idx that is not 16-byte aligned, and normals absent."""
    import torch
    for n in WS.matrix_sizes(D):
        c = WS.matrix_case(D, k, n)
        args = (dev(c["nodes"]), dev(c["dq"]), dev(c["node_w"]))
        verts, nrm = dev(c["verts"]), dev(c["normals"])
        idx = WS.knn(c["nodes"], c["verts"], k)
        assert (idx[:, min(D, k):] == -1).all() and (idx[:, :min(D, k)] >= 0).all()
        sv, sn = WS.warp_graph(c["nodes"], c["dq"], c["node_w"], idx, c["verts"], c["normals"])
        ov, on = A.warp_to_live(*args, k, verts, nrm)
        assert WS.deviation(host(ov), sv) <= WARP_BOUND and WS.deviation(host(on), sn) <= WARP_BOUND
        ov2, on2 = A.warp_to_live(*args, k, verts)  # normals absent
        assert on2 is None and torch.equal(ov2, ov)
        m = 500
        sq = WS.calc_dqb_graph(c["nodes"], c["dq"], c["node_w"], idx[:m], c["verts"][:m])
        assert WS.deviation(host(A.calc_dqb(*args, k, verts[:m])), sq) <= WARP_BOUND
        # the given graph: the statement's own neighbour lists (not the kernel's), -1 entries where D < k
        gi = dev(idx)
        gv, gn = A.warp_to_live_graph(*args, gi, verts, nrm)
        assert torch.equal(gv, ov) and torch.equal(gn, on)
        gv2, gn2 = A.warp_to_live_graph(*args, gi, verts)
        assert gn2 is None and torch.equal(gv2, ov)
        # ... from an idx array that starts one int32 into a buffer: the scalar neighbour loads
        buf = torch.full((idx.size + 1,), -5, dtype=torch.int32, device="cuda")
        buf[1:] = gi.reshape(-1)
        view = buf[1:].view(idx.shape)
        assert view.data_ptr() % 16 == 4
        gv3, gn3 = A.warp_to_live_graph(*args, view, verts, nrm)
        assert torch.equal(gv3, ov) and torch.equal(gn3, on)


@pytest.mark.parametrize("k", [4, 8, 16])
def test_warp_with_a_graph_that_has_holes(A, k):
    """-1 entries anywhere in a given graph (a caller's pruned graph, not only the padding of D < k) are skipped: the
    statement with the same lists"""
    c = WS.matrix_case(300, k, 2000)
    idx = WS.knn(c["nodes"], c["verts"], k)
    rng = np.random.default_rng(k)
    idx[rng.random(idx.shape) < 0.3] = -1
    idx[:5] = -1  # no neighbour at all: the identity
    args = (dev(c["nodes"]), dev(c["dq"]), dev(c["node_w"]))
    gv, gn = A.warp_to_live_graph(*args, dev(idx), dev(c["verts"]), dev(c["normals"]))
    sv, sn = WS.warp_graph(c["nodes"], c["dq"], c["node_w"], idx, c["verts"], c["normals"])
    assert WS.deviation(host(gv), sv) <= WARP_BOUND and WS.deviation(host(gn), sn) <= WARP_BOUND
    assert np.array_equal(host(gv)[:5], c["verts"][:5])


@pytest.mark.parametrize("D,n", [(40, 1000), (2048, 1000)])  # brute force | grid
@pytest.mark.parametrize("k", [1, 4, 8, 16])
def test_warp_of_degenerate_vertices(A, D, k, n):
    c = WS.matrix_case(D, k, n)
    verts = c["verts"].copy()
    # NaN coordinates: every distance is NaN, so the vertex has no neighbour (include/dynfu_amd.h: dfa_knn pads with -1 and
    # the warp is the blend of the neighbours given) — the blend is the identity and the output is the NaN input
    verts[100] = np.nan
    verts[101, 1] = np.nan
    # exactly on a node (weight exp(0) = 1) — the first min(n, D) vertices already are
    verts[102] = c["nodes"][D - 1]
    # so far from every node that all weights underflow to 0 in float32: the dual part of the blend vanishes, the real
    # part is the ordered product of the neighbours' rotations
    verts[103] = [60.0, -70.0, 80.0]
    verts[104] = [-1e3, 2e3, 1e3]
    idx = WS.knn(c["nodes"], verts, k)
    assert (idx[100] == -1).all() and (idx[101] == -1).all()
    assert (WS.weights(c["nodes"], c["node_w"], verts, idx)[103:105] == 0).all()
    sv, sn = WS.warp_graph(c["nodes"], c["dq"], c["node_w"], idx, verts, c["normals"])
    assert np.isnan(sv[100]).all() and np.isnan(sv[101]).all() and np.isfinite(sv[102:105]).all()
    ov, on = A.warp_to_live(dev(c["nodes"]), dev(c["dq"]), dev(c["node_w"]), k, dev(verts), dev(c["normals"]))
    ov, on = host(ov), host(on)
    assert np.isnan(ov[100]).all() and np.isnan(ov[101]).all()
    # the far vertices: float32 rounding of a rotated coordinate of magnitude 2e3 is relative, so the absolute bound is
    # applied in units of the coordinate magnitude there (bound * max(1, |v|))
    near = np.ones(n, bool)
    near[[103, 104]] = False
    assert WS.deviation(ov[near], sv[near]) <= WARP_BOUND and WS.deviation(on[near], sn[near]) <= WARP_BOUND
    for v in (103, 104):
        scale = max(1.0, float(np.abs(verts[v]).max()))
        assert np.abs(ov[v] - sv[v]).max() <= WARP_BOUND * scale
        assert np.abs(on[v] - sn[v]).max() <= WARP_BOUND
    got = host(A.calc_dqb(dev(c["nodes"]), dev(c["dq"]), dev(c["node_w"]), k, dev(verts[100:105])))
    sq = WS.calc_dqb_graph(c["nodes"], c["dq"], c["node_w"], idx[100:105], verts[100:105])
    assert WS.deviation(got, sq) <= WARP_BOUND
    assert np.array_equal(got[0], WS.IDENTITY.astype(np.float32)) and (got[3:, 4:] == 0).all()


@pytest.mark.parametrize("D,k,n", [(300, 1, 20000), (300, 16, 20000), (2048, 1, 30000), (2048, 16, 30000), (2048, 8, 30000),
                                    (3, 16, 500), (8192, 5, 40000)])
def test_unsupported_vertices_equal_the_statement(A, D, k, n):
    rng = np.random.default_rng(D + k)
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = rng.uniform(0.05, 0.3, D).astype(np.float32)
    verts = rng.uniform(-1.3, 1.3, (n, 3)).astype(np.float32)
    verts[:D] = nodes[:n]
    verts[-1] = np.nan
    ref = WS.unsupported_flags(nodes, node_w, k, verts)
    assert 0 < ref.mean() < 1 and not ref[:min(D, n)].any() and ref[-1] == 1
    assert np.array_equal(host(A.unsupported_vertices(dev(nodes), dev(node_w), k, dev(verts))), ref)


@pytest.mark.parametrize("D,n", [(200, 5000), (2048, 30000)])  # brute force | grid (the flags-only early exit)
def test_unsupported_vertices_with_very_different_radii(A, D, n):
    """a far node with a wide radius supports a vertex its nearest node does not: the 1-NN early exit of the flags-only
    kernel must fall through to the full search there"""
    rng = np.random.default_rng(D)
    nodes = rng.uniform(-1, 1, (D, 3)).astype(np.float32)
    node_w = np.where(rng.random(D) < 0.1, 0.6, 0.01).astype(np.float32)  # a few wide nodes among narrow ones
    verts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    k = 8
    idx = WS.knn(nodes, verts, k)
    d = np.linalg.norm(verts[:, None, :].astype(np.float64) - nodes[idx], axis=2)
    q = d / node_w[idx]
    by_far_node_only = (q[:, 0] >= 1) & (q[:, 1:].min(1) < 1)
    assert by_far_node_only.sum() > n // 20  # the input contains such vertices
    ref = WS.unsupported_flags(nodes, node_w, k, verts)
    assert not ref[by_far_node_only].any() and 0 < ref.mean() < 1
    assert np.array_equal(host(A.unsupported_vertices(dev(nodes), dev(node_w), k, dev(verts))), ref)
    # with k = 1 the same vertices are unsupported
    ref1 = WS.unsupported_flags(nodes, node_w, 1, verts)
    assert ref1[by_far_node_only].all()
    assert np.array_equal(host(A.unsupported_vertices(dev(nodes), dev(node_w), 1, dev(verts))), ref1)
