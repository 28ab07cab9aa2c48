"""-m gpu tests of the k-NN field (dfa_knn_field_*) and of the warped integrations served from it, on the cases of
tests/tsdf_warped_cases.py, tests/tsdf_warped6_cases.py and tests/knn_field_cases.py.

No tolerance anywhere: the rows are the statement's (tests/knn_field_statement.py: warp_statement.knn, exact with ties), a field
that was appended to is the field built in one go, id for id, and a cached integration leaves the volume and the occupancy
map of the uncached call, bit for bit.  One cached result per case file also goes through the uncached tests' bar against
the numpy statement, which ties the chain to the statement and not only to the sibling kernel.

In a node frame (the cases of tests/tsdf_warped6_cases.py and tests/knn_field_cases.py) the rows are the statement's wherever the
k + 1 nearest nodes are more than the statement's own float32 deviation apart, and a valid list at the few voxels where they are
not; the stored set lies between the statement's lower and upper bound (profiles/knn_field_node_frame.md: the figures)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import knn_field_cases as KC  # noqa: E402
import knn_field_statement as KS  # noqa: E402
import tsdf_warped6_cases as C6  # noqa: E402
import tsdf_warped_cases as CS  # noqa: E402
from gpu_util import dev, host  # noqa: E402

MODE = {0: "skip", 1: "rigid"}  # DFA_WARPED_SKIP, DFA_WARPED_RIGID: the statements' SKIP / RIGID
WITH_NODES = [n for n in CS.CASES if CS.CASES[n][1] > 0]
BOTH = [("ref", n) for n in CS.CASES] + [("six", n) for n in C6.CASES]


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def get_case(kind, name):
    return CS.case(name) if kind == "ref" else C6.case(name)


def all_voxels(dims):
    """(n, 3) int32 (x, y, z) of every voxel, in the volume's memory order"""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)


def lookup_all(f, dims):
    """the rows of every voxel, (Z, Y, X, k)"""
    X, Y, Z = dims
    return host(f.lookup(dev(all_voxels(dims)))).reshape(Z, Y, X, f.k)


def make_field(A, c, steps=None, nodes=None, node_w=None, max_bytes=0):
    """a field of the case's geometry, k and frame, built on the first steps[0] nodes and appended to at every further step
    (default: built on all nodes) -> (field, the device arrays it was last given)"""
    nodes = c["nodes"] if nodes is None else nodes
    node_w = c["node_w"] if node_w is None else node_w
    steps = [len(nodes)] if steps is None else steps
    f = A.KnnField(c["dims"], c["voxel_size"], c["k"], vol2node=c.get("vol2node"), max_bytes=max_bytes)
    keep = None
    for i, D in enumerate(steps):
        keep = (dev(nodes[:D]), dev(node_w[:D])) if D else (None, None)
        (f.build if i == 0 else f.append)(*keep)
    return f, keep


def integrate(A, kind, c, field=None, vol=None, dists=None, occupancy=None, D=None):
    """the case's call (on its first D nodes) on a copy of its starting volume, or on `vol` -> the volume after it, uint32"""
    D = c["D"] if D is None else D
    vol = dev(c["vol"]) if vol is None else vol
    nodes, dq, w = (dev(c[n][:D]) if D else None for n in ("nodes", "node_dq", "node_w"))
    dists = dev(c["dists"] if dists is None else dists)
    if kind == "ref":
        A.tsdf_integrate_warped(vol, dists, c["voxel_size"], float(c["trunc"]), CS.MAX_WEIGHT, c["vol2cam"], *CS.INTR, nodes, dq, w,
                                c["k"], unsupported=MODE[c["mode"]], occupancy=occupancy, field=field)
    else:
        A.tsdf_integrate_warped6(vol, dists, c["voxel_size"], float(c["trunc"]), C6.MAX_WEIGHT, c["vol2node"], c["node2cam"], *c["intr"],
                                 nodes, dq, w, c["k"], unsupported=MODE[c["mode"]], occupancy=occupancy, field=field)
    return host(vol, np.uint32)


# ------------------------------------------------------------------------------------------ 1. lookup against the statement
@pytest.mark.parametrize("name", WITH_NODES)
def test_lookup_is_the_statement(A, name):
    c, s = CS.case(name), KS.case(name)
    X, Y, Z = c["dims"]
    f, _ = make_field(A, c)
    rows = lookup_all(f, c["dims"])
    has = rows[..., 0] >= 0  # (D > 0: every voxel of a stored brick has a nearest node)
    stored = np.zeros(len(s["must"]), bool)
    stored[np.unique(s["brick"][has])] = True
    info = f.info()
    print("%s: %d of %d bricks stored, %d must be; %d bytes" % (name, int(stored.sum()), len(stored), int(s["must"].sum()), info["bytes"]))
    assert np.array_equal(has, stored[s["brick"]]), "a brick is stored as a whole or not at all"
    assert not (s["must"] & ~stored).any(), "a brick that must be stored is not"
    assert np.array_equal(rows[has], s["rows"][has]), "rows of stored voxels"
    assert (rows[~has] == -1).all(), "rows of voxels that are not stored"
    assert info == dict(D=c["D"], k=c["k"], stored_bricks=int(stored.sum()), total_bricks=len(stored),
                        bytes=int(stored.sum()) * 256 * c["k"] * 4)
    outside = np.array([[-1, 0, 0], [X, 0, 0], [0, -1, 0], [0, Y, 0], [0, 0, -1], [0, 0, Z], [X + 63, Y + 3, Z], [-64, -4, -1],
                        [2 ** 31 - 1, 0, 0], [0, -2 ** 31, 0], [X - 1, Y - 1, Z - 1]], np.int32)
    got = host(f.lookup(dev(outside)))
    assert (got[:-1] == -1).all() and np.array_equal(got[-1], rows[Z - 1, Y - 1, X - 1])
    f.close()


def check_against_statement(f, c, s, label):
    """every row of the field f, its stored set and its info() against the statement s of the inputs c -> the rows"""
    rows = lookup_all(f, c["dims"])
    has = rows[..., 0] >= 0  # (D > 0: every voxel of a stored brick has a nearest node)
    stored = KS.stored_bricks(rows, s)
    assert np.array_equal(has, stored[s["brick"]]), "a brick is stored as a whole or not at all"
    bad_rows, differ = KS.check_rows(rows, s, stored)
    info = f.info()
    print("%s: %d of %d bricks stored, %d must be, %d may be; %d bytes; rho %.3g, %d voxels ambiguous, %d of them with another row "
          "than the float32 statement's" % (label, int(stored.sum()), len(stored), int(s["must"].sum()), int(s["may"].sum()), info["bytes"],
                                            s["rho"], int(s["ambiguous"].sum()), differ))
    assert KS.check_stored(stored, s) == []
    assert bad_rows == []
    assert (rows[~has] == -1).all(), "rows of voxels that are not stored"
    assert info == dict(D=s["D"], k=c["k"], stored_bricks=int(stored.sum()), total_bricks=len(stored),
                        bytes=int(stored.sum()) * 256 * c["k"] * 4)
    return rows


SIX_WITH_NODES = [n for n in C6.CASES if C6.CASES[n][1] > 0]
LAST = KC.RADII_SPECIAL["last"]
#             kind     name  k     D (None: all)
NODE_FRAME = [("six", n, None, None) for n in SIX_WITH_NODES] + [("field", "turned", None, None)] + \
             [("field", n, None, D) for n in KC.RADII for D in (LAST, None)] + [("field", n, k, None) for n in KC.TIES for k in KC.CASES[n][0]]


@pytest.mark.parametrize("kind,name,k,D", NODE_FRAME)
def test_lookup_is_the_statement_in_a_node_frame(A, kind, name, k, D):
    """rows exact at decided voxels and valid at ambiguous ones (knn_field_statement.check_rows), the stored set between its
    lower and its upper bound.  The radii cases also on their first 69 nodes, without the infinite / NaN radius that stores
    every brick.  A NaN radius is not refused: the build stores every brick, as field_mark_kernel's comment says"""
    c, s = KS.inputs(name, kind, k), KS.case(name, D, kind, k)
    X, Y, Z = c["dims"]
    f, _ = make_field(A, c, [s["D"]])
    rows = check_against_statement(f, c, s, "%s %s k = %d D = %d" % (kind, name, c["k"], s["D"]))
    if s["every_brick"] or np.isinf(s["node_w"]).any():
        assert f.info()["stored_bricks"] == f.info()["total_bricks"] and f.info()["bytes"] == len(s["must"]) * 256 * c["k"] * 4
    outside = np.array([[-1, 0, 0], [X, 0, 0], [0, -1, 0], [0, Y, 0], [0, 0, -1], [0, 0, Z], [X + 63, Y + 3, Z], [-64, -4, -1],
                        [2 ** 31 - 1, 0, 0], [0, -2 ** 31, 0], [X - 1, Y - 1, Z - 1]], np.int32)
    got = host(f.lookup(dev(outside)))
    assert (got[:-1] == -1).all() and np.array_equal(got[-1], rows[Z - 1, Y - 1, X - 1])
    f.close()


D_TIES = 111
APPENDS = [("six", "main_posed_rigid_junk", None, [2, 63, 64, 300]),  # padded lists (D < k), then the scan, then the node grid
           ("six", "odd_scan_moved", None, [0, 63]),                  # an empty field first
           ("six", "tiny_k3_grid_moved", None, [1, 64]),
           ("field", "turned", None, [150, 300])] + \
          [("field", n, k, steps) for n in KC.TIES for k in KC.CASES[n][0]
           for steps in ([1, 50, 63, 64, D_TIES], [64, D_TIES - KC.LATTICE_DUPLICATES, D_TIES])]  # ... the last step: the duplicates alone


@pytest.mark.parametrize("kind,name,k,steps", APPENDS)
def test_append_equals_build_in_a_node_frame(A, kind, name, k, steps):
    """id for id at every intermediate step, with no allowance: both fields saw the same float positions.  On the tie cases the
    merge meets candidates at the distance of list entries (and, with the duplicates, at the position of one)"""
    c = KS.inputs(name, kind, k)
    assert steps[-1] == c["D"]
    for upto in range(1, len(steps)):
        part = steps[:upto + 1]
        built, _ = make_field(A, c, [part[-1]])
        grown, _ = make_field(A, c, part)
        a, b = lookup_all(built, c["dims"]), lookup_all(grown, c["dims"])
        print("%s %s k = %d %s: %d rows differ" % (kind, name, c["k"], part, int((a != b).any(-1).sum())))
        assert np.array_equal(a, b), part
        assert built.info() == grown.info()
        if part[-1] == c["D"]:
            check_against_statement(grown, c, KS.case(name, None, kind, k), "%s %s grown" % (kind, name))
        built.close(), grown.close()


@pytest.mark.parametrize("name", ["turned", "radii_posed"])
def test_a_field_grown_then_used(A, name):
    """the new geometries through the sweeps: a field built on half the nodes and appended to serves dfa_tsdf_integrate_warped6_field;
    the volume is the searching call's bit for bit, and passes the uncached tests' bar against the numpy statement"""
    import test_gpu_tsdf_warped6 as T6
    c = KC.warped6_case(name)
    want = integrate(A, "six", c)
    f, _ = make_field(A, c, [c["D"] // 2, c["D"]])
    got = integrate(A, "six", c, field=f)
    print("%s: %d voxels differ of %d; %d changed by the call" % (name, int((got != want).sum()), want.size, int((want != c["vol"]).sum())))
    assert np.array_equal(got, want)
    T6.check(got, c)
    f.close()


# ------------------------------------------------------------------------------------------ 2. append equals build
def largest_radius_last(c):
    order = np.argsort(c["node_w"], kind="stable")
    return c["nodes"][order], c["node_w"][order]


@pytest.mark.parametrize("name,steps,reorder", [
    ("main_skip", [2, 63, 64, 300], False),  # padded lists (D < k), then the scan, then the node grid
    ("k16", [1000, 1024], False),
    ("odd_scan", [0, 63], False),            # an empty field first
    ("main_skip", [299, 300], True),         # the new node's radius exceeds every old one
])
def test_append_equals_build(A, name, steps, reorder):
    c = CS.case(name)
    nodes, w = largest_radius_last(c) if reorder else (c["nodes"], c["node_w"])
    if reorder:
        assert w[-1] > w[:-1].max()
    for upto in range(1, len(steps)):  # every intermediate field too
        part = steps[:upto + 1]
        built, _ = make_field(A, c, [part[-1]], nodes, w)
        grown, _ = make_field(A, c, part, nodes, w)
        a, b = lookup_all(built, c["dims"]), lookup_all(grown, c["dims"])
        print("%s %s: %d rows differ" % (name, part, int((a != b).any(-1).sum())))
        assert np.array_equal(a, b), part
        assert built.info() == grown.info()
        if part[-1] == c["D"] and not reorder:
            has = a[..., 0] >= 0
            assert np.array_equal(a[has], KS.case(name)["rows"][has])
        built.close(), grown.close()


def test_append_of_no_nodes_changes_nothing(A):
    c = CS.case("main_skip")
    f, (nodes, w) = make_field(A, c)
    before, info = lookup_all(f, c["dims"]), f.info()
    f.append(nodes, w)
    assert np.array_equal(lookup_all(f, c["dims"]), before) and f.info() == info
    with pytest.raises(A.DynfuAmdError, match="D_new is smaller"):
        f.append(nodes[:10], w[:10])
    f.close()


# ------------------------------------------------------------------------------------------ 3. cached = uncached, bit for bit
@pytest.mark.parametrize("kind,name", BOTH)
def test_cached_is_uncached(A, kind, name):
    """every case of both files in its own mode: from a field built in one go, and from one built on a prefix and appended to"""
    c = get_case(kind, name)
    want = integrate(A, kind, c)
    f, _ = make_field(A, c)
    got = integrate(A, kind, c, field=f)
    print("%s %s: %d voxels differ of %d; %d changed by the call" % (kind, name, int((got != want).sum()), want.size,
                                                                     int((want != c["vol"]).sum())))
    assert np.array_equal(got, want)
    g, _ = make_field(A, c, [c["D"] // 3, c["D"] - c["D"] // 4, c["D"]])
    assert np.array_equal(integrate(A, kind, c, field=g), want), "from an appended field"
    f.close(), g.close()


@pytest.mark.parametrize("kind,name", [("ref", "main_skip"), ("ref", "main_rigid_junk"), ("ref", "odd_scan"), ("ref", "thin"),
                                       ("six", "main_posed_rigid_junk"), ("six", "odd_scan_moved")])
def test_cached_occupancy_is_uncached(A, kind, name):
    """the map pre-filled as in test_gpu_tsdf_warped.test_occupancy_superset: the same map bytes, the same volume"""
    import torch
    c = get_case(kind, name)
    f, _ = make_field(A, c)
    before = np.random.default_rng(5).integers(0, 4, tuple(A.tsdf_occupancy(dev(c["vol"])).shape)).astype(np.uint8)
    before[::2] = 0
    maps, vols = [], []
    for field in (None, f):
        occ = A.tsdf_occupancy(dev(c["vol"]))
        occ.copy_(torch.from_numpy(before))
        vols.append(integrate(A, kind, c, field=field, occupancy=occ))
        maps.append(host(occ))
    assert np.array_equal(vols[0], vols[1]) and np.array_equal(maps[0], maps[1])
    assert (maps[1] != before).any(), "the call marks boxes"
    f.close()


@pytest.mark.parametrize("kind,name", [("ref", "main_skip"), ("six", "main_posed_rigid_junk")])
def test_two_frames_from_one_field(A, kind, name):
    """the field is not consumed: a second frame (the depth shifted by three texels) into the same volume"""
    c = get_case(kind, name)
    f, _ = make_field(A, c)
    second = np.roll(c["dists"], 3, axis=1)
    out = []
    for field in (None, f):
        vol = dev(c["vol"])
        first = integrate(A, kind, c, field=field, vol=vol)
        out.append((first, integrate(A, kind, c, field=field, vol=vol, dists=second)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert (out[0][1] != out[0][0]).any(), "the second frame changes the volume"
    f.close()


def test_cached_against_the_numpy_statement(A):
    """the bar of the uncached tests (their check()) on a cached result, once per case file"""
    import test_gpu_tsdf_warped as T
    import test_gpu_tsdf_warped6 as T6
    for kind, name, check in (("ref", "main_skip", T.check), ("six", "main_posed_rigid_junk", T6.check)):
        c = get_case(kind, name)
        f, _ = make_field(A, c)
        check(integrate(A, kind, c, field=f), c)
        f.close()


def test_a_stale_field_is_refused(A):
    c = CS.case("main_skip")
    f, _ = make_field(A, c, [200])
    with pytest.raises(A.DynfuAmdError, match="another number of nodes"):
        integrate(A, "ref", c, field=f)
    f.close()
    with pytest.raises(A.DynfuAmdError, match="closed"):
        integrate(A, "ref", c, field=f)


# ------------------------------------------------------------------------------------------ 4. capacity
def test_capacity_of_a_build(A):
    c = CS.case("main_skip")
    f, _ = make_field(A, c)
    need, rows = f.info()["bytes"], lookup_all(f, c["dims"])
    nodes, w = dev(c["nodes"]), dev(c["node_w"])
    small = A.KnnField(c["dims"], c["voxel_size"], c["k"], max_bytes=need - 1)
    with pytest.raises(A.CapacityError, match="max_bytes"):
        small.build(nodes, w)
    assert small.info() == dict(D=0, k=c["k"], stored_bricks=0, total_bricks=f.info()["total_bricks"], bytes=0)
    assert (lookup_all(small, c["dims"]) == -1).all(), "an empty, valid field"
    exact = A.KnnField(c["dims"], c["voxel_size"], c["k"], max_bytes=need)
    exact.build(nodes, w)
    assert exact.info() == f.info() and np.array_equal(lookup_all(exact, c["dims"]), rows)
    for x in (f, small, exact):
        x.close()


def test_capacity_of_an_append(A):
    """a field capped at what its first 20 nodes need: the append of the rest is refused and leaves every row as it was"""
    c = CS.case("main_skip")
    part, _ = make_field(A, c, [20])
    whole, _ = make_field(A, c)
    assert whole.info()["stored_bricks"] > part.info()["stored_bricks"]
    f, _ = make_field(A, c, [20], max_bytes=part.info()["bytes"])
    before, info = lookup_all(f, c["dims"]), f.info()
    assert np.array_equal(before, lookup_all(part, c["dims"]))
    with pytest.raises(A.CapacityError, match="max_bytes"):
        f.append(dev(c["nodes"]), dev(c["node_w"]))
    assert f.info() == info and np.array_equal(lookup_all(f, c["dims"]), before)
    assert np.array_equal(integrate(A, "ref", c, field=f, D=20), integrate(A, "ref", c, D=20)), "the field still serves its 20 nodes"
    for x in (part, whole, f):
        x.close()


# ------------------------------------------------------------------------------------------ 5. two streams
def test_two_streams(A):
    """two fields with different node sets built and used on two streams at once: the rows are per field, the node grid per
    stream; the volumes are the single-stream ones"""
    import torch
    ca, cb = CS.case("main_skip"), CS.case("k16")
    single = integrate(A, "ref", ca), integrate(A, "ref", cb)
    torch.cuda.synchronize()
    streams = torch.cuda.Stream(), torch.cuda.Stream()
    for rep in range(3):
        out = []
        for c, s in zip((ca, cb), streams):
            vol = dev(c["vol"])
            args = [dev(c[n]) for n in ("dists", "nodes", "node_dq", "node_w")]
            f = A.KnnField(c["dims"], c["voxel_size"], c["k"])
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                f.build(args[1][:200].contiguous(), args[3][:200].contiguous())
                f.append(args[1], args[3])
                A.tsdf_integrate_warped(vol, args[0], c["voxel_size"], float(c["trunc"]), CS.MAX_WEIGHT, c["vol2cam"], *CS.INTR,
                                        args[1], args[2], args[3], c["k"], unsupported=MODE[c["mode"]], field=f)
            out.append((vol, args, f))
        torch.cuda.synchronize()
        got = [host(v, np.uint32) for v, _, _ in out]
        assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1])
        for _, _, f in out:
            f.close()
