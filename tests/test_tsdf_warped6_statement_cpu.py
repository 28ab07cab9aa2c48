"""CPU checks of the north-star warped-integrate statement (tests/tsdf_warped6_statement.py) and of its cases: it reduces to the
rigid statement where the node transforms are the identity, a voxel worked by hand, q and -q give the same volume, the cases
are not vacuous and almost all of their voxels are decided, the recorded float32 deviation holds — and the C call checks its
arguments before it touches the GPU."""
import ctypes

import numpy as np
import pytest

import tsdf_statement as TS
import tsdf_warped6_cases as C6
import tsdf_warped6_statement as W6
import tsdf_warped_statement as WST
import warp_statement as WS
from extract_statement import pack, unpack

f32 = np.float32
IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f32)


@pytest.mark.parametrize("name", ["odd_grid_rigid_posed", "no_nodes_rigid", "thin"])
def test_identity_transforms_give_the_rigid_statement(name):
    """identity node transforms move no voxel: with RIGID mode — or SKIP mode over the supported voxels — the call is
    tsdf_statement.integrate with vol2cam = node2cam . vol2node, on decided voxels"""
    c = C6.case(name)
    ref = c["ref"]
    v2n = IDENTITY12 if c["vol2node"] is None else c["vol2node"]
    n2c = IDENTITY12 if c["node2cam"] is None else c["node2cam"]
    rigid = TS.integrate(c["vol"], c["dists"], c["voxel_size"], c["trunc"], C6.MAX_WEIGHT, W6.compose(n2c, v2n), *c["intr"])
    where = ref["decided"] & (ref["supported"] if c["mode"] == W6.SKIP else True)
    assert where.sum() > 0
    changed = rigid != c["vol"]
    sat = (c["vol"] >> 16) == C6.MAX_WEIGHT  # (a saturated voxel may be updated to the very same bits)
    assert np.array_equal(changed[where & ~sat], (ref["vol"] != c["vol"])[where & ~sat])
    Fa, Wa = unpack(ref["vol"][where])
    Fb, Wb = unpack(rigid[where])
    assert np.array_equal(Wa, Wb)
    assert np.abs(Fa - Fb).max() <= WST.tsdf_tolerance(ref["rho"], c["trunc"])
    if c["mode"] == W6.SKIP:  # ... and no unsupported voxel moves
        assert np.array_equal(ref["vol"][~ref["supported"]], c["vol"][~ref["supported"]])


def test_one_voxel_by_hand():
    """A (1, 1, 2) volume of 0.5 m voxels; no frame transforms; f = 10, c = 2.5.  Two nodes, k = 2:
      A at (0, 0, 0.5) = voxel 1, radius 0.5, rotating by 90 degrees about z (r = (s, 0, 0, s), s = sqrt(1/2)) and then
        translating by t = (0.25, 0, 0.5): d = 1/2 (0, t) r;
      B at (0, 0, 1.5), radius 1, the identity.
    Voxel 1, c = (0, 0, 0.5): raw weights w_A = exp(0) = 1, w_B = exp(-1 / 2) — a sum of 1.6065, so normalisation matters:
      with u = w~_A, v = w~_B (u + v = 1) a = (u s + v, 0, 0, u s), b = u d.  The rotations are about z and c is on the z axis, so
      vec(a c a*) = |a|^2 c; 2 vec(b a*) = 2 u vec(d a*) with d = 1/2 (0, t) r, a* = conj: a point p = c + (2 u vec(d a*)) / |a|^2.
      Not the translation sum: B's share turns A's translation.  The numbers below are the formula evaluated in fp64 by hand
      (plain Python floats), the statement has to agree to 1e-12.
    Voxel 0, c = 0: |c - A| / 0.5 = 1 -> not < 1; |c - B| / 1 = 1.5: unsupported."""
    s = np.sqrt(0.5)
    t = np.array([0.25, 0.0, 0.5])
    rA = np.array([s, 0, 0, s])
    dA = 0.5 * WS.qmul(np.array([0.0, *t]), rA)
    dq = np.array([np.concatenate([rA, dA]), WS.IDENTITY], f32)
    nodes = np.array([[0, 0, 0.5], [0, 0, 1.5]], f32)
    w = np.array([0.5, 1.0], f32)
    # by hand, from the float32 inputs
    wA, wB = 1.0, float(np.exp(-1.0 / 2.0))
    u, v = wA / (wA + wB), wB / (wA + wB)
    r32, d32 = dq[0, :4].astype(np.float64), dq[0, 4:].astype(np.float64)
    a = u * r32 + v * np.array([1.0, 0, 0, 0])
    b = u * d32
    m = float(a @ a)
    conj = a * np.array([1, -1, -1, -1])
    cq = np.array([0.0, 0, 0, 0.5])
    p = (WS.qmul(WS.qmul(a, cq), conj)[1:] + 2 * WS.qmul(b, conj)[1:]) / m
    assert abs(p[2] - 0.5 - u * 0.5 * (a[0] * s + a[3] * s) / m * 1.0) < 1e-6  # z: c_z + u t_z (a . r) / |a|^2
    assert abs(np.hypot(p[0], p[1]) - u * 0.25 * np.sqrt((a[0] * s + a[3] * s) ** 2 + (a[0] * s - a[3] * s) ** 2) / m) < 1e-6
    assert np.abs(p - (np.array([0, 0, 0.5]) + u * t)).max() > 0.02  # not the weighted translation

    dists = np.ones((5, 5), np.float16).view(np.uint16)
    old = pack(np.array([0.25, 0.5], f32), np.array([7, 1])).reshape(2, 1, 1)
    cam = W6.camera_points((2, 1, 1), [0.5] * 3, None, None, nodes, dq, w, 2, W6.SKIP)
    assert cam["supported"].tolist() == [False, True]
    assert np.abs(cam["vc64"][1] - p).max() < 1e-12
    for mode in (W6.SKIP, W6.RIGID):
        r = W6.integrate(old, dists, [0.5] * 3, 0.125, 64, None, None, 10, 10, 2.5, 2.5, nodes, dq, w, 2, mode)
        assert r["supported"].ravel().tolist() == [False, True]
        # voxel 1: Dp = 1, sdf = 1 - |p| within the truncation band or in front of it
        sdf = 1.0 - float(np.linalg.norm(p))
        want = min(1.0, sdf / 0.125)
        assert sdf >= -0.125 and r["updated"][1, 0, 0]
        assert abs(float(r["tsdf"][1, 0, 0]) - want) < 1e-5
        F, W = unpack(r["vol"][1, 0, 0])
        assert W == 2 and abs(float(F) - (0.5 + want) / 2) <= 2.0 ** -11
        # voxel 0 is at the camera centre (z = 0): never updated, in either mode
        assert r["vol"][0, 0, 0] == old[0, 0, 0]


def test_antipodal_equality():
    """q and -q are the same motion: the hemisphere sign makes the statement's volume the same, exactly"""
    for name, base in C6.ANTIPODAL_OF.items():
        a, b = C6.case(name), C6.case(base)
        assert np.array_equal(a["node_dq"][0::2], b["node_dq"][0::2]) and np.array_equal(a["node_dq"][1::2], -b["node_dq"][1::2])
        assert np.array_equal(a["vol"], b["vol"]) and np.array_equal(a["nodes"], b["nodes"])
        assert np.array_equal(a["ref"]["vol"], b["ref"]["vol"])
        assert np.array_equal(a["ref"]["decided"], b["ref"]["decided"])
        assert (a["ref"]["vol"] != a["vol"]).sum() > 500


@pytest.mark.parametrize("name", list(C6.CASES))
def test_support_rule_is_warp_statements(name):
    """the support flags are warp_statement.unsupported_flags' at the node-frame positions"""
    c = C6.case(name)
    v = WST.voxel_positions(c["vol"].shape, c["voxel_size"])
    flags = WS.unsupported_flags(c["nodes"], c["node_w"], c["k"], W6.apply32(c["vol2node"], v))
    assert np.array_equal(flags == 0, c["ref"]["supported"].ravel())


@pytest.mark.parametrize("name", C6.MAIN)
def test_cases_are_not_vacuous(name):
    ref = C6.case(name)["ref"]
    upd = ref["updated"]
    assert upd.sum() >= 500
    assert (upd & (ref["tsdf"] < 1)).sum() >= 200
    assert ref["supported"].sum() >= 500 and (~ref["supported"]).sum() >= 500


@pytest.mark.parametrize("name", list(C6.CASES))
def test_undecided_share(name):
    """at most 2 % of the voxels the statement updates (a condition on the cases: with more, change the case)"""
    ref = C6.case(name)["ref"]
    undecided, updated = int((~ref["decided"]).sum()), int(ref["updated"].sum())
    print("%s: %d undecided, %d updated (%.3f %%), rho %.3g" % (name, undecided, updated, 100.0 * undecided / max(updated, 1), ref["rho"]))
    assert undecided <= 0.02 * updated


def test_cases_cover_the_matrix():
    vals = list(C6.CASES.values())
    assert {v[0] for v in vals} == {(32, 32, 32), (50, 38, 44), (9, 7, 14), (1, 2, 12)}
    assert {(v[1], v[2]) for v in vals} == {(300, 8), (63, 4), (2, 8), (1024, 8), (0, 8), (64, 3)}
    assert {v[3] for v in vals} == {"identity", "general"} and {v[4] for v in vals} == {W6.SKIP, W6.RIGID}
    assert {v[5] for v in vals} == {"empty", "junk"} and {v[6] for v in vals} == {"volume", "posed", "moved"}
    c = C6.case("big_moved")
    R = c["vol2node"][:9].reshape(3, 3).astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and 0.29 < np.arccos((np.trace(R) - 1) / 2) < 0.31
    assert np.abs(c["vol2node"][9:]).max() > 0.5 * c["edge"]
    posed = C6.case("main_posed_rigid_junk")
    assert np.abs(W6.compose(posed["node2cam"], posed["vol2node"]) - posed["vol2cam"]).max() < 1e-6
    assert np.abs(W6.compose(c["node2cam"], c["vol2node"]) - c["vol2cam"]).max() > 1e-2  # "moved": the camera is elsewhere


def test_the_recorded_deviation_holds_over_the_cases():
    """WARPED6_DEVIATION, re-measured: the float32 evaluation of steps 1-6 (operation by operation, the header's order) against
    the fp64 statement, relative to L, over every case"""
    dev = {name: C6.measured_deviation(name) for name in C6.CASES}
    for name, d in dev.items():
        print("%-24s %.3e" % (name, d))
    top = max(dev.values())
    print("largest: %.4e, recorded %.4e" % (top, W6.WARPED6_DEVIATION))
    assert top <= W6.WARPED6_DEVIATION < 1e-5
    assert top > W6.WARPED6_DEVIATION / 2


# ------------------------------------------------------------------------------------------ the C call's validation
@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.dfa_tsdf_integrate_warped6.argtypes = [vp, i, i, i, vp, i, i, i, vp, vp, f, i, vp, vp, f, f, f, f, vp, vp, vp, i, i, i, vp]
    L.dfa_last_error.restype = ctypes.c_char_p
    return L


def test_argument_validation_needs_no_gpu(lib):
    """every refusal comes before any HIP call, with DFA_ERR_INVALID (1) and a message"""
    vs = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
    ident = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    sheared = (ctypes.c_float * 12)(1, 0.01, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    scaled = (ctypes.c_float * 12)(1.01, 0, 0, 0, 1.01, 0, 0, 0, 1.01, 0, 0, 0)
    nan = (ctypes.c_float * 12)(float("nan"), 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    p = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first

    def call(dists=p, volume=p, dims=(8, 8, 8), image=(16, 8, 8), pos=p, dq=p, w=p, D=4, k=8, mode=0, v2n=ident, n2c=ident, voxel=vs):
        return lib.dfa_tsdf_integrate_warped6(dists, image[0], image[1], image[2], volume, dims[0], dims[1], dims[2], None, voxel, 0.1,
                                              64, v2n, n2c, 10.0, 10.0, 4.0, 4.0, pos, dq, w, D, k, mode, None)

    for kw, msg in ((dict(volume=None), b"bad volume"), (dict(dists=None), b"bad dists image"), (dict(dims=(8, 0, 8)), b"bad volume"),
                    (dict(dims=(-1, 8, 8)), b"bad volume"), (dict(image=(16, 0, 8)), b"bad dists image"),
                    (dict(image=(16, 8, -2)), b"bad dists image"), (dict(voxel=None), b"null parameter block"),
                    (dict(D=-1), b"negative node count"),
                    (dict(pos=None), b"nodes without"), (dict(dq=None), b"nodes without"), (dict(w=None), b"nodes without"),
                    (dict(k=0), b"k out of range 1..8"), (dict(k=9), b"k out of range 1..8"), (dict(k=16), b"k out of range 1..8"),
                    (dict(mode=2), b"unknown unsupported_mode"), (dict(mode=-1), b"unknown unsupported_mode"),
                    (dict(v2n=sheared), b"vol2node must be rigid"), (dict(v2n=scaled), b"vol2node must be rigid"),
                    (dict(v2n=nan), b"vol2node must be rigid")):
        assert call(**kw) == 1, kw
        err = lib.dfa_last_error()
        assert b"dfa_tsdf_integrate_warped6" in err and msg in err, (kw, err)
    # no nodes, no node arrays, SKIP mode: valid, and nothing to do — no HIP call either; with or without the transforms
    assert call(pos=None, dq=None, w=None, D=0) == 0
    assert call(pos=None, dq=None, w=None, D=0, v2n=None, n2c=None) == 0
