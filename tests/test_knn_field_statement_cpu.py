"""CPU checks of the k-NN field's statement (tests/knn_field_statement.py) against itself on the cases of
tests/tsdf_warped_cases.py — every brick that holds a supported voxel must be stored, and the cases exercise stored and
unstored bricks and both branches of the support rule —; of the statement in a node frame (tests/tsdf_warped6_cases.py,
tests/knn_field_cases.py): the measured deviation behind rho, the share of ambiguous voxels, the tie density of the tie cases, the
order of the stored set's bounds, and that check_rows / check_stored flag planted defects and nothing else; and of the C calls'
argument checks, which come before any HIP call."""
import ctypes

import numpy as np
import pytest

import knn_field_cases as KC
import knn_field_statement as KS
import tsdf_warped6_cases as C6
import tsdf_warped_cases as CS

WITH_NODES = [n for n in CS.CASES if CS.CASES[n][1] > 0]
# bricks that must be stored / bricks of the volume, per case (on all of them: exactly the bricks with a supported voxel)
MUST_STORE = {"main_skip": (230, 256), "main_rigid_junk": (228, 256), "odd_scan": (422, 440), "odd_grid_rigid": (432, 440),
              "k16": (234, 256), "padded": (7, 28), "thin": (10, 12), "thin_padded": (6, 12),
              "tiny_k4_grid": (26, 28), "tiny_k16_scan": (28, 28)}


@pytest.mark.parametrize("name", WITH_NODES)
def test_every_brick_with_a_supported_voxel_must_be_stored(name):
    """a supported voxel has a node with |v - g_m| < w_m (warp_statement.unsupported_flags, through the case's statement), and
    the box of its brick is no farther from that node than the voxel"""
    c, s = CS.case(name), KS.case(name)
    held = np.zeros(len(s["must"]), bool)
    held[np.unique(s["brick"][c["ref"]["supported"]])] = True
    print("%s: %d of %d bricks must be stored, %d hold a supported voxel" % (name, int(s["must"].sum()), len(s["must"]), int(held.sum())))
    assert not (held & ~s["must"]).any()
    assert (int(s["must"].sum()), len(s["must"])) == MUST_STORE[name]


@pytest.mark.parametrize("name", CS.MAIN)
def test_cases_are_not_vacuous(name):
    c, s = CS.case(name), KS.case(name)
    sup = c["ref"]["supported"]
    assert s["must"].any() and not s["must"].all(), "stored and unstored bricks"
    assert sup.any(), "a supported voxel"
    assert (~sup & s["must"][s["brick"]]).any(), "an unsupported voxel inside a stored brick"


def test_rows_are_dfa_knns_contract():
    """padding when D < k, ascending (distance, index) order, and the brick index of a voxel"""
    s = KS.case("padded")
    assert s["rows"].shape == (14, 7, 9, 8) and (s["rows"][..., 2:] == -1).all() and (np.sort(s["rows"][..., :2], -1) == [0, 1]).all()
    c, s = CS.case("odd_scan"), KS.case("odd_scan")
    z, y, x = 17, 5, 49
    v = np.array([x, y, z], np.float32) * c["voxel_size"]
    d = c["nodes"] - v
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert s["rows"][z, y, x].tolist() == sorted(range(len(d2)), key=lambda i: (d2[i], i))[:c["k"]]
    assert KS.brick_grid(c["dims"]) == (1, 10, 44) and s["brick"][z, y, x] == (17 * 10 + 1) * 1 + 0
    assert KS.brick_grid((130, 4, 2)) == (3, 1, 2)


def test_must_store_by_hand():
    """(70, 5, 2) voxels of 0.5: bricks x {0..63, 64..69}, y {0..3, 4}, z {0}, {1}.  One node at (40, 0, 0): the box of x brick 1
    ends at voxel 69 = 34.5, 5.5 away (x brick 0: 8.5); y brick 1 is the plane y = 2.0, z brick 1 the plane z = 0.5.  So brick
    (1, 0, 0) is 5.5 away, (1, 0, 1) 5.523, (1, 1, 0) 5.852 and (1, 1, 1) 5.874"""
    for radius, want in ((5.1, []), (5.6, [(1, 0, 0), (1, 0, 1)]), (5.9, [(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)])):
        m = KS.must_store((70, 5, 2), [0.5] * 3, np.array([[40.0, 0, 0]], np.float32), np.array([radius], np.float32)).reshape(2, 2, 2)
        got = sorted((int(x), int(y), int(z)) for z, y, x in zip(*np.nonzero(m)))
        assert got == sorted(want), (radius, got)


# ------------------------------------------------------------------------------------------ the statement in a node frame
SIX_WITH_NODES = [n for n in C6.CASES if C6.CASES[n][1] > 0]
EVERY = [("ref", n, None) for n in WITH_NODES] + [("six", n, None) for n in SIX_WITH_NODES] + \
        [("field", n, k) for n in KC.CASES for k in KC.CASES[n][0]]
FRAMED = [(kind, n, k) for kind, n, k in EVERY if (kind == "six" and C6.CASES[n][6] != "volume") or (kind == "field" and KC.CASES[n][1])]


def test_every_framed_case_has_its_constant():
    assert sorted(KS.FIELD_DEVIATION) == sorted({(kind, n) for kind, n, _ in FRAMED})


@pytest.mark.parametrize("kind,name,k", FRAMED)
def test_deviation_and_ambiguous_share_of_a_framed_case(kind, name, k):
    """rho is measured again and stays within the recorded constant; at most 2 % of the voxels are ambiguous"""
    s = KS.case(name, kind=kind, k=k)
    share = float(s["ambiguous"].mean())
    print("%s %s k = %d: max |d32 - d64| = %.3e m (recorded %.1e), rho = %.3e m, %d of %d voxels ambiguous (%.3f %%), %.1f %% with a tie" %
          (kind, name, s["k"], s["deviation"], KS.FIELD_DEVIATION[kind, name], s["rho"], int(s["ambiguous"].sum()), s["ambiguous"].size,
           100 * share, 100 * float(KS.case_pairs(name, None, kind, k)["tie"].mean())))
    assert s["deviation"] <= KS.FIELD_DEVIATION[kind, name]
    assert share <= KS.AMBIGUOUS_CAP
    if name in KC.TIES:
        assert s["rho"] == 0.0 and not s["ambiguous"].any(), "an exact frame: every voxel is decided, ties included"
    else:
        assert s["rho"] == 2 * s["deviation"] > 0


@pytest.mark.parametrize("kind,name,k", EVERY)
def test_bounds_of_the_stored_set_are_ordered(kind, name, k):
    """the voxel rule's set lies within the box rule's (no frame), and the lower bound within the upper one"""
    s, held = KS.case(name, kind=kind, k=k), KS.case_pairs(name, None, kind, k)["must_voxel"]
    print("%s %s: %d bricks hold a supported voxel, %d must be stored, %d may be, of %d" %
          (kind, name, int(held.sum()), int(s["must"].sum()), int(s["may"].sum()), len(s["must"])))
    assert not (held & ~s["must"]).any() and (not s["framed"] or np.array_equal(held, s["must"]))
    assert not (s["must"] & ~s["may"]).any()
    assert s["framed"] or not s["ambiguous"].any()


@pytest.mark.parametrize("name,k", [(n, k) for n in KC.TIES for k in KC.CASES[n][0]])
def test_tie_cases_have_ties(name, k):
    c, s = KC.case(name, k), KS.case(name, kind="field", k=k)
    _, c32, c64 = KS.positions(c["dims"], c["voxel_size"], c["vol2node"])
    density = float(KS.case_pairs(name, None, "field", k)["tie"].mean())
    print("%s k = %d: D = %d, %.1f %% of the voxels have an exact tie among their k + 1 nearest" % (name, k, c["D"], 100 * density))
    assert density >= 0.25
    assert np.array_equal(c32.astype(np.float64), c64), "the frame is exact in float32"
    assert 100 < c["D"] < 128 and len(np.unique(c["nodes"], axis=0)) == c["D"] - KC.LATTICE_DUPLICATES
    assert np.array_equal(c["nodes"][-3:], c["nodes"][[5, 40, 77]])
    # exact arithmetic: the float32 squared distances are the fp64 ones
    q = c32[::97]
    d = q[:, None, :] - c["nodes"][None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    e = c64[::97, None, :] - c["nodes"].astype(np.float64)[None]
    assert np.array_equal(d2.astype(np.float64), (e * e).sum(-1))


def test_radii_cases_are_what_they_say():
    S = KC.RADII_SPECIAL
    for name in ("radii", "radii_nan"):
        c = KC.case(name)
        w, g, edge = c["node_w"], c["nodes"], 1.0
        assert w[S["zero"]] == 0 and w[S["negative"]] < 0 and g[S["far_outside"]][0] - edge >= 10 * edge
        assert -w[S["half_outside"]] < g[S["half_outside"]][0] < 0
        assert np.array_equal(g[S["far_corner"]], (np.array(c["dims"], np.float32) - 1) * c["voxel_size"])
        assert (np.isnan(w).sum(), np.isinf(w).sum()) == ((1, 0) if name == "radii_nan" else (0, 1))
        whole, part = KS.case(name, kind="field"), KS.case(name, D=S["last"], kind="field")
        assert whole["may"].all() and whole["every_brick"] == (name == "radii_nan")
        assert part["must"].any() and not part["may"].all() and not part["every_brick"], "without the last node the others decide"
    assert KS.case("radii", kind="field")["must"].all(), "an infinite radius supports every voxel"


def test_the_turned_frame_is_far_from_the_existing_ones():
    c = KC.case("turned")
    R, t = c["vol2node"][:9].reshape(3, 3).astype(np.float64), c["vol2node"][9:]
    assert abs(np.arccos((np.trace(R) - 1) / 2) - 2.6) < 1e-6 and np.abs(t).max() == 5.0 and t[0] == 3.0
    s = KS.case("turned", kind="field")
    assert s["must"].any() and not s["may"].all()


def test_the_warped6_statement_holds_its_bound_on_the_new_cases():
    """tsdf_warped6_statement.WARPED6_DEVIATION was measured on tsdf_warped6_cases; the two cases that go through
    dfa_tsdf_integrate_warped6 here stay within it, so test_gpu_tsdf_warped6.check applies to them as it stands"""
    import tsdf_warped6_statement as W6
    for name in ("turned", "radii_posed"):
        c = KC.warped6_case(name)
        with np.errstate(all="ignore"):
            dev = W6.deviation(c["vol"].shape, c["voxel_size"], c["vol2node"], c["node2cam"], c["nodes"], c["node_dq"], c["node_w"], c["k"],
                               c["mode"])
        print("%s: |vc32 - vc64| / L = %.3e" % (name, dev))
        assert dev <= W6.WARPED6_DEVIATION
        assert c["ref"]["updated"].any() and c["ref"]["supported"].any()


def answer(s, stored=None):
    """the statement's own answer as a lookup of every voxel would return it: its rows in the bricks `stored` (default: the ones
    that must be), -1 elsewhere"""
    stored = s["must"] if stored is None else stored
    return np.where(stored[s["brick"]][..., None], s["rows"], -1).astype(np.int32), stored.copy()


def flagged(got, stored, s):
    bad, _ = KS.check_rows(got, s, stored)
    return bad + KS.check_stored(stored, s)


def test_the_comparison_catches_planted_defects():
    import tsdf_warped6_statement as W6
    import warp_statement as WS
    s, c = KS.case("turned", kind="field"), KC.case("turned")
    X, Y, Z = c["dims"]
    k = c["k"]
    clean, stored = answer(s)
    assert flagged(clean, stored, s) == [], "nothing on the statement's own answer"
    for kind, name, kk in (("ref", "main_skip", None), ("six", "big_moved", None), ("field", "ties_lattice", 8), ("field", "radii_nan", None)):
        t = KS.case(name, kind=kind, k=kk)
        assert flagged(*answer(t, t["may"] if t["every_brick"] else None), t) == [], name
    has = stored[s["brick"]]
    z, y, x = (int(a[7]) for a in np.nonzero(has & ~s["ambiguous"]))  # a decided voxel of a stored brick
    # 1. two adjacent ids swapped at a decided voxel
    got = clean.copy()
    got[z, y, x, [2, 3]] = got[z, y, x, [3, 2]]
    assert flagged(got, stored, s)
    # 2. one id replaced by the (k + 1)-th nearest
    _, c32, _ = KS.positions(c["dims"], c["voxel_size"], c["vol2node"])
    flat = (z * Y + y) * X + x
    got = clean.copy()
    got[z, y, x, k - 1] = WS.knn(c["nodes"], c32[flat:flat + 1], k + 1)[0, k]
    assert flagged(got, stored, s)
    # 3. the frame ignored: rows searched at v;  4. its translation dropped: rows searched at R v
    v = KS.positions(c["dims"], c["voxel_size"])[1]
    turn_only = np.concatenate([c["vol2node"][:9], np.zeros(3, np.float32)])
    for where in (v, W6.apply32(turn_only, v)):
        got = np.where(has[..., None], WS.knn(c["nodes"], where, k).reshape(Z, Y, X, k), -1).astype(np.int32)
        assert flagged(got, stored, s)
    # 5. tie order reversed at a tied voxel of ties_lattice
    t, tc = KS.case("ties_lattice", kind="field", k=4), KC.case("ties_lattice", 4)
    tclean, tstored = answer(t)
    tz, ty, tx = 2, 2, 30
    row = tclean[tz, ty, tx]
    d = np.array([tx, ty, tz], np.float32) * tc["voxel_size"] - tc["nodes"][row]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    j = int(np.flatnonzero(np.diff(d2) == 0)[0])
    assert row[j] < row[j + 1], "equal distances: the lower index first"
    got = tclean.copy()
    got[tz, ty, tx, [j, j + 1]] = row[[j + 1, j]]
    assert flagged(got, tstored, t)
    # 6. one must-store brick removed
    b = int(np.flatnonzero(s["must"])[11])
    fewer = stored.copy()
    fewer[b] = False
    assert flagged(answer(s, fewer)[0], fewer, s)
    # 7. every brick stored
    every = np.ones_like(stored)
    assert not s["may"].all() and flagged(answer(s, every)[0], every, s)
    # the allowance at an ambiguous voxel is for the near-tie alone: the two ids that are within 2 rho of each other may come in
    # either order, an id from farther away may not
    az, ay, ax = (int(a[0]) for a in np.nonzero(has & s["ambiguous"]))
    e = s["c64"][(az * Y + ay) * X + ax] - c["nodes"][clean[az, ay, ax]].astype(np.float64)
    near = np.flatnonzero(np.diff(np.sqrt((e * e).sum(-1))) <= 2 * s["rho"])
    if len(near):  # (the near-tie may also be between the k-th and the (k + 1)-th nearest)
        j = int(near[0])
        got = clean.copy()
        got[az, ay, ax, [j, j + 1]] = clean[az, ay, ax, [j + 1, j]]
        assert flagged(got, stored, s) == []
    got = clean.copy()
    far = int(np.setdiff1d(s["rows"][Z - 1 - az, Y - 1 - ay, X - 1 - ax], clean[az, ay, ax])[0])  # a neighbour of the opposite voxel
    got[az, ay, ax, 0] = far
    assert flagged(got, stored, s)
    got = clean.copy()
    got[az, ay, ax, 1] = got[az, ay, ax, 0]
    assert flagged(got, stored, s), "an id twice"


# ------------------------------------------------------------------------------------------ the C calls' validation
@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.dfa_knn_field_create.argtypes = [i, i, i, vp, i, vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.dfa_knn_field_destroy.argtypes = [vp]
    L.dfa_knn_field_destroy.restype = None
    L.dfa_knn_field_build.argtypes = [vp, vp, vp, i, vp]
    L.dfa_knn_field_append.argtypes = [vp, vp, vp, i, vp]
    warped = [vp, i, i, i, vp, i, i, i, vp, vp, f, i, vp, f, f, f, f, vp, vp, vp, i, i, i, vp, vp]
    L.dfa_tsdf_integrate_warped_field.argtypes = warped
    L.dfa_tsdf_integrate_warped6_field.argtypes = warped[:12] + [vp] + warped[12:]
    L.dfa_last_error.restype = ctypes.c_char_p
    return L


VS = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
IDENT = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
TURN = (ctypes.c_float * 12)(0, -1, 0, 1, 0, 0, 0, 0, 1, 0.5, 0, 0)  # a quarter turn about z and a translation: rigid


def create(lib, dims=(8, 8, 8), vs=VS, k=8, vol2node=None):
    h = ctypes.c_void_p()
    rc = lib.dfa_knn_field_create(dims[0], dims[1], dims[2], vs, k, vol2node, 0, ctypes.byref(h))
    return rc, h


def test_create_refuses_bad_arguments(lib):
    shear = (ctypes.c_float * 12)(1, 0.1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    nan = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, float("nan"), 0, 0)
    for kw, msg in ((dict(k=0), b"k out of range"), (dict(k=17), b"k out of range"), (dict(dims=(8, 0, 8)), b"bad volume dimensions"),
                    (dict(dims=(-3, 8, 8)), b"bad volume dimensions"), (dict(vs=None), b"null voxel_size"),
                    (dict(vol2node=shear), b"vol2node must be rigid"), (dict(vol2node=nan), b"vol2node must be rigid")):
        rc, h = create(lib, **kw)
        assert rc == 1 and not h.value, kw
        err = lib.dfa_last_error()
        assert b"dfa_knn_field_create" in err and msg in err, (kw, err)
    assert lib.dfa_knn_field_create(8, 8, 8, VS, 8, None, 0, None) == 1 and b"null out" in lib.dfa_last_error()


def test_append_refuses_fewer_nodes(lib):
    """a fresh field holds no nodes; building it with none makes no HIP call, and neither does the refusal"""
    rc, h = create(lib)
    assert rc == 0 and h.value
    assert lib.dfa_knn_field_build(h, None, None, 0, None) == 0
    assert lib.dfa_knn_field_append(h, None, None, 0, None) == 0  # nothing new: nothing happens
    assert lib.dfa_knn_field_append(h, None, None, -1, None) == 1
    err = lib.dfa_last_error()
    assert b"dfa_knn_field_append" in err and b"D_new is smaller" in err, err
    p = ctypes.c_void_p(0x1000)  # never dereferenced
    assert lib.dfa_knn_field_build(h, p, None, 3, None) == 1 and b"nodes without" in lib.dfa_last_error()
    assert lib.dfa_knn_field_build(h, None, None, -2, None) == 1 and b"negative node count" in lib.dfa_last_error()
    assert lib.dfa_knn_field_build(None, None, None, 0, None) == 1 and b"null field" in lib.dfa_last_error()
    lib.dfa_knn_field_destroy(h)
    lib.dfa_knn_field_destroy(None)


def test_integrate_refuses_a_field_that_does_not_match(lib):
    """each of geometry, k, D and frame, both calls; every refusal names its function and reason, before any HIP call"""
    p = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
    fields = {}
    for name, kw in (("plain", {}), ("turned", dict(vol2node=TURN)), ("ident", dict(vol2node=IDENT))):
        rc, fields[name] = create(lib, **kw)
        assert rc == 0

    def call(six, field, dims=(8, 8, 8), vs=VS, D=0, k=8, vol2node=None):
        head = [p, 16, 8, 8, p, dims[0], dims[1], dims[2], None, vs, 0.1, 64]
        tail = [10.0, 10.0, 4.0, 4.0, p, p, p, D, k, 0, field, None]
        if six:
            return lib.dfa_tsdf_integrate_warped6_field(*head, vol2node, None, *tail)
        return lib.dfa_tsdf_integrate_warped_field(*head, IDENT, *tail)

    other_vs = (ctypes.c_float * 3)(0.1, 0.1, 0.2)
    almost = (ctypes.c_float * 12)(*TURN)
    almost[11] = 1e-7
    for six, fn in ((False, b"dfa_tsdf_integrate_warped_field"), (True, b"dfa_tsdf_integrate_warped6_field")):
        mine = dict(field=fields["turned"], vol2node=TURN) if six else dict(field=fields["plain"])
        assert call(six, **mine) == 0  # matches; no nodes, SKIP mode: nothing to do, no HIP call
        for kw, msg in ((dict(dims=(8, 8, 9)), b"another volume geometry"), (dict(vs=other_vs), b"another volume geometry"),
                        (dict(k=4), b"another k"), (dict(D=5), b"another number of nodes"), (dict(field=None), b"null field")):
            assert call(six, **dict(mine, **kw)) == 1, (six, kw)
            err = lib.dfa_last_error()
            assert fn in err and msg in err, (six, kw, err)
    # the frame
    assert call(False, fields["turned"]) == 1 and b"dfa_tsdf_integrate_warped_field" in lib.dfa_last_error() and \
        b"the field has a vol2node" in lib.dfa_last_error()
    for field, vol2node in ((fields["plain"], TURN), (fields["turned"], None), (fields["turned"], almost), (fields["turned"], IDENT),
                            (fields["ident"], None)):
        assert call(True, field, vol2node=vol2node) == 1
        assert b"dfa_tsdf_integrate_warped6_field" in lib.dfa_last_error() and b"vol2node differs" in lib.dfa_last_error()
    assert call(True, fields["ident"], vol2node=IDENT) == 0 and call(True, fields["plain"]) == 0
    # the uncached calls' own checks still come first
    assert lib.dfa_tsdf_integrate_warped_field(p, 16, 8, 8, None, 8, 8, 8, None, VS, 0.1, 64, IDENT, 10.0, 10.0, 4.0, 4.0, p, p, p, 0, 8, 0,
                                               fields["plain"], None) == 1 and b"bad volume" in lib.dfa_last_error()
    for h in fields.values():
        lib.dfa_knn_field_destroy(h)
