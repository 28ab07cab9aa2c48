"""CPU checks of the warped-integrate statement (tests/tsdf_warped_statement.py) and of its cases: it reduces to the rigid
statement where the warp is the identity, a voxel worked by hand, the cases are not vacuous and almost all of their voxels
are decided — and the C call checks its arguments before it touches the GPU."""
import ctypes

import numpy as np
import pytest

import tsdf_statement as TS
import tsdf_warped_cases as CS
import tsdf_warped_statement as WST
import warp_statement as WS
from extract_statement import pack, unpack

f32 = np.float32


@pytest.mark.parametrize("name", ["odd_grid_rigid", "no_nodes_rigid", "thin"])
def test_identity_warp_is_the_rigid_statement(name):
    """identity node transforms move no voxel (exactly, in fp64): with RIGID mode — or SKIP mode over the supported voxels — the
    call is tsdf_statement.integrate up to that statement's running sum of positions, i.e. on decided voxels"""
    c = CS.case(name)
    ref = c["ref"]
    rigid = TS.integrate(c["vol"], c["dists"], c["voxel_size"], c["trunc"], CS.MAX_WEIGHT, c["vol2cam"], *CS.INTR)
    where = ref["decided"] & (ref["supported"] if c["mode"] == WST.SKIP else True)
    assert where.sum() > 0
    changed = rigid != c["vol"]
    sat = (c["vol"] >> 16) == CS.MAX_WEIGHT  # (a saturated voxel may be updated to the very same bits)
    assert np.array_equal(changed[where & ~sat], (ref["vol"] != c["vol"])[where & ~sat])
    Fa, Wa = unpack(ref["vol"][where])
    Fb, Wb = unpack(rigid[where])
    assert np.array_equal(Wa, Wb)
    assert np.abs(Fa - Fb).max() <= WST.tsdf_tolerance(ref["rho"], c["trunc"])
    if c["mode"] == WST.SKIP:  # ... and no unsupported voxel moves
        assert np.array_equal(ref["vol"][~ref["supported"]], c["vol"][~ref["supported"]])


def test_one_voxel_by_hand():
    """A (1, 1, 2) volume of 0.5 m voxels, one node AT voxel z = 1 = (0, 0, 0.5) with radius 0.1 that translates by
    (0.125, 0, 0.25); vol2cam translates by (0, 0, 0.25); f = 10, c = 2.5 (no point on a texel boundary).
      voxel 1: quotient 0 -> supported, weight exp(0) = 1, blend = the node's transform: p = (0.125, 0, 0.75),
               vc = (0.125, 0, 1): coo = (10 * 0.125 + 2.5, 2.5) = (3.75, 2.5) -> texel (3, 2), Dp = 1;
               sdf = 1 - sqrt(1.015625) = -0.0077822, trunc 0.125 -> tsdf = -0.0622577;
               old (0.5, weight 1) -> (0.5 * 1 - 0.0622577) / 2 = 0.2188712, weight 2.
      voxel 0: |v - g| / w = 0.5 / 0.1 = 5 -> unsupported.  SKIP leaves it; RIGID takes vc = (0, 0, 0.25) -> coo = (2.5, 2.5), texel (2, 2),
               which is 0 -> skipped as well."""
    dists = np.zeros((5, 5), np.float16)
    dists[2, 3] = 1.0
    dists = dists.view(np.uint16)
    old = pack(np.array([0.25, 0.5], f32), np.array([7, 1])).reshape(2, 1, 1)
    nodes = np.array([[0, 0, 0.5]], f32)
    dq = WS.dq_from_euler(0, 0, 0, 0.125, 0, 0.25).astype(f32).reshape(1, 8)
    w = np.array([0.1], f32)
    vol2cam = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0.25]
    for mode in (WST.SKIP, WST.RIGID):
        r = WST.integrate(old, dists, [0.5] * 3, 0.125, 64, vol2cam, 10, 10, 2.5, 2.5, nodes, dq, w, 8, mode)
        assert r["supported"].ravel().tolist() == [False, True]
        assert r["updated"].ravel().tolist() == [False, True]
        assert r["decided"].all()
        assert r["vol"][0, 0, 0] == old[0, 0, 0]
        F, W = unpack(r["vol"][1, 0, 0])
        assert W == 2
        assert abs(float(F) - 0.2188712) <= 2.0 ** -13  # one fp16 step in [0.125, 0.25)
        assert abs(float(r["tsdf"][1, 0, 0]) + 0.0622577) < 1e-6


@pytest.mark.parametrize("name", list(CS.CASES))
def test_support_rule_is_warp_statements(name):
    """the statement keeps the support quotient (the decided set needs it): its flags are warp_statement.unsupported_flags'"""
    c = CS.case(name)
    v = WST.voxel_positions(c["vol"].shape, c["voxel_size"])
    flags = WS.unsupported_flags(c["nodes"], c["node_w"], c["k"], v)
    assert np.array_equal(flags == 0, c["ref"]["supported"].ravel())


@pytest.mark.parametrize("name", CS.MAIN)
def test_cases_are_not_vacuous(name):
    ref = CS.case(name)["ref"]
    upd = ref["updated"]
    assert upd.sum() >= 500
    assert (upd & (ref["tsdf"] < 1)).sum() >= 200
    assert ref["supported"].sum() >= 500 and (~ref["supported"]).sum() >= 500


@pytest.mark.parametrize("name", list(CS.CASES))
def test_undecided_share(name):
    """at most 2 % of the voxels the statement updates (a condition on the cases: with more, change the case)"""
    ref = CS.case(name)["ref"]
    undecided, updated = int((~ref["decided"]).sum()), int(ref["updated"].sum())
    print("%s: %d undecided, %d updated (%.3f %%), rho %.3g" % (name, undecided, updated, 100.0 * undecided / max(updated, 1), ref["rho"]))
    assert undecided <= 0.02 * updated


def test_cases_cover_every_shape_and_mode():
    vals = list(CS.CASES.values())
    assert {v[0] for v in vals} == {(32, 32, 32), (50, 38, 44), (9, 7, 14), (1, 2, 12)}
    assert {(v[1], v[2]) for v in vals} == {(300, 8), (63, 4), (2, 8), (1024, 16), (0, 8), (64, 4), (63, 16)}
    assert {v[3] for v in vals} == {"identity", "general"} and {v[4] for v in vals} == {WST.SKIP, WST.RIGID}
    assert {v[5] for v in vals} == {"empty", "junk"}
    junk = CS.case("main_rigid_junk")["vol"] >> 16
    assert {0, 1, CS.MAX_WEIGHT} <= set(np.unique(junk).tolist())
    zero = np.mean([(CS.case(n)["dists"] == 0).mean() for n in CS.MAIN])
    assert 0.03 < zero < 0.07


# ------------------------------------------------------------------------------------------ the C call's validation
@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.dfa_tsdf_integrate_warped.argtypes = [vp, i, i, i, vp, i, i, i, vp, vp, f, i, vp, f, f, f, f, vp, vp, vp, i, i, i, vp]
    L.dfa_last_error.restype = ctypes.c_char_p
    return L


def test_argument_validation_needs_no_gpu(lib):
    """every refusal comes before any HIP call, with DFA_ERR_INVALID (1) and a message"""
    vs = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
    aff = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    p = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first

    def call(dists=p, volume=p, dims=(8, 8, 8), image=(16, 8, 8), pos=p, dq=p, w=p, D=4, k=8, mode=0):
        return lib.dfa_tsdf_integrate_warped(dists, image[0], image[1], image[2], volume, dims[0], dims[1], dims[2], None, vs, 0.1,
                                             64, aff, 10.0, 10.0, 4.0, 4.0, pos, dq, w, D, k, mode, None)

    for kw, msg in ((dict(volume=None), b"bad volume"), (dict(dists=None), b"bad dists image"), (dict(dims=(8, 0, 8)), b"bad volume"),
                    (dict(dims=(-1, 8, 8)), b"bad volume"), (dict(image=(16, 0, 8)), b"bad dists image"),
                    (dict(image=(16, 8, -2)), b"bad dists image"), (dict(D=-1), b"negative node count"),
                    (dict(pos=None), b"nodes without"), (dict(dq=None), b"nodes without"), (dict(w=None), b"nodes without"),
                    (dict(k=0), b"k out of range"), (dict(k=17), b"k out of range"), (dict(mode=2), b"unknown unsupported_mode"),
                    (dict(mode=-1), b"unknown unsupported_mode")):
        assert call(**kw) == 1, kw
        err = lib.dfa_last_error()
        assert b"dfa_tsdf_integrate_warped" in err and msg in err, (kw, err)
    # no nodes, no node arrays, SKIP mode: valid, and nothing to do — no HIP call either
    assert call(pos=None, dq=None, w=None, D=0) == 0
