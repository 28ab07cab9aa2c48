"""CPU checks of the k-NN field's statement (tests/knn_field_statement.py) against itself on the cases of
tests/tsdf_warped_cases.py — every brick that holds a supported voxel must be stored, and the cases exercise stored and
unstored bricks and both branches of the support rule —, and of the C calls' argument checks, which come before any HIP call."""
import ctypes

import numpy as np
import pytest

import knn_field_statement as KS
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
