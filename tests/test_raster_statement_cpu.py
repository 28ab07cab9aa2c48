"""CPU tests of tests/raster_statement.py, the numpy statement tests/test_gpu_raster.py compares dfa_mesh_rasterize with:
the hand-written coverage of the top-left rule, the partition of a quad, rasterize32 against the fp64 ray-triangle check, and
the conditions the shared cases must meet for the GPU comparison to say something.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import raster_cases as RC
import raster_statement as RS


def _covered(name):
    return RS.coverage(RC.reference(name)[0])


def test_top_left_rule_on_the_hand_written_triangle():
    got = tuple("".join("#" if v >= 0 else "." for v in row) for row in _covered("a"))
    assert got == RC.COVERAGE_A, "\n".join(got)
    z, points, normals = RC.reference("a")
    hit = z != RS.MISS
    assert (RS.depth_bits(z)[hit] == np.float32(1).view(np.uint32)).all()  # the triangle lies in the plane z = 1
    assert np.array_equal(points[hit][:, :2], np.argwhere(hit)[:, ::-1].astype(np.float32))  # fx = 1, cx = 0: x = i, y = j
    assert np.isnan(points[~hit]).all() and np.isnan(normals[~hit]).all()
    assert np.array_equal(normals[hit], np.tile(np.float32([0, 0, -1, 0]), (hit.sum(), 1)))  # the face, towards the camera


@pytest.mark.parametrize("name", ["b_cw", "b_ccw"])
def test_two_triangles_partition_the_quad(name):
    c = RC.case(name)
    idx = c["indices"].reshape(-1, 3)
    count = np.zeros((c["rows"], c["cols"]), int)
    for t in range(2):  # each triangle alone: what it covers does not depend on the other
        count += RS.coverage(RS.rasterize32(c["vertices"], None, idx[t], *RC.args(c))[0]) >= 0
    inside = np.zeros_like(count)
    inside[3:9, 3:11] = 1  # rows 3 ... 8, columns 3 ... 10: the right and bottom edges own nothing
    assert np.array_equal(count, inside)
    both = _covered(name)
    assert np.array_equal(both >= 0, inside == 1) and set(np.unique(both)) == {-1, 0, 1}
    assert both[6, 7] in (0, 1)  # the centre on the diagonal belongs to one of them


def test_both_windings_cover_the_same_pixels():
    assert np.array_equal(_covered("b_cw") >= 0, _covered("b_ccw") >= 0)


def test_copies_and_depth_order():
    cov = _covered("c")
    assert set(np.unique(cov)) == {-1, 0, 2, 3}  # of the copies 0 and 1 the lower number wins everywhere
    c = RC.case("c")
    alone = [RS.coverage(RS.rasterize32(c["vertices"], None, c["indices"].reshape(-1, 3)[t], *RC.args(c))[0]) >= 0 for t in range(4)]
    assert np.array_equal(alone[0], alone[1]) and (alone[2] & alone[3]).sum() > 20
    assert (cov[alone[2] & alone[3]] == 3).all()  # the nearer of the two parallel triangles, although it comes later


def test_the_winner_changes_inside_a_box():
    cov = _covered("d")
    c = RC.case("d")
    alone = [RS.coverage(RS.rasterize32(c["vertices"], None, c["indices"].reshape(-1, 3)[t], *RC.args(c))[0]) >= 0 for t in range(2)]
    both = alone[0] & alone[1]
    assert (cov[both] == 0).sum() > 30 and (cov[both] == 1).sum() > 30


def test_skip_rules():
    cov = _covered("e")
    assert set(np.unique(cov)) == {-1, 0, 8, 9}  # the drawn triangle and the two that straddle the border
    drawn, _, _, _ = RS.setup(RC.case("e")["vertices"], RC.case("e")["indices"], *RC.args(RC.case("e"))[:-2])
    assert drawn.tolist() == [True, False, False, False, False, False, False, True, True, True]  # (7 is drawn: off the image)
    assert (cov[:, -1] == 8).any() and (cov[-1, :] == 8).any() and (cov[0, :] == 9).any() and (cov[:, 0] == 9).any()
    z, points, normals = RC.reference("f")
    assert (z == RS.MISS).all() and np.isnan(points).all() and np.isnan(normals).all()


def test_wide_and_small_triangles_share_case_g():
    cov = _covered("g")
    share = [(cov == t).mean() for t in (3, 40)]
    assert min(share) > 0.2 and sum(share) > 0.6, share
    assert len(set(np.unique(cov)) - {-1, 3, 40}) >= 5  # small triangles in front of the wide ones
    assert (_covered("h") == 0).all()


@pytest.mark.parametrize("name", ["c", "d", "i"])
def test_rasterize32_against_the_fp64_visibility(name):
    """hit or miss, and the depth within (|dz/du| + |dz/dv|) / 256 + 8 ulp, on every pixel that is no knife edge; at most
    2 % of the hit pixels are knife edges"""
    c = RC.case(name)
    z = RC.reference(name)[0]
    chk = RS.check64(c["vertices"], c["indices"], *RC.args(c))
    knife, wrong_side, too_far = RS.compare(z, chk)
    hit = (z != RS.MISS) | (chk["tri"] >= 0)
    share = (knife & hit).sum() / hit.sum()
    err = np.abs(RS.depth_bits(z).view(np.float32).astype(np.float64) - chk["z"])[(z != RS.MISS) & (chk["tri"] >= 0) & ~knife]
    print("%s: %d hit pixels, %.2f %% knife edges, %d hit / miss disagreements, %d depths over their bound, worst %.3g m"
          % (name, hit.sum(), 100 * share, wrong_side.sum(), too_far.sum(), err.max()))
    assert hit.sum() > 100 and share <= 0.02
    assert not wrong_side.any() and not too_far.any()


def test_conditions_of_the_sphere_cases():
    """a tenth of the pixels on each side of hit / miss (as render_scenes.check_conditions asks of the render scenes); normals
    of hits are unit vectors or NaN; the camera frame is the raycast's"""
    for name in ("i", "j"):
        z, points, normals = RC.reference(name)
        hit = z != RS.MISS
        assert 0.1 <= hit.mean() <= 0.9, (name, hit.mean())
        assert np.array_equal(np.isnan(points[..., 0]), ~hit)
        n = normals[hit]
        good = ~np.isnan(n[:, 0])
        assert good.mean() > 0.9 and np.abs(np.linalg.norm(n[good, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
        assert (n[good, 2] < 0).mean() > 0.95  # the TSDF gradient points out of the surface, towards the camera
    assert len(RC.case("i")["indices"]) // 3 > 1000


def test_argument_validation_needs_no_gpu():
    """arguments are checked before any HIP call: DFA_ERR_INVALID and the error string"""
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynfu_amd", "libdynfu_amd.so"))
    lib.dfa_last_error.restype = C.c_char_p
    f = lib.dfa_mesh_rasterize
    vp, i, fl = C.c_void_p, C.c_int, C.c_float
    f.argtypes = [vp, vp, i, vp, i, vp, fl, fl, fl, fl, fl, i, i, vp, vp, i, vp, i, vp]
    p = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused first)

    def call(vertices=p, N=3, indices=p, T=1, z_near=0.1, cols=16, rows=16, zbuffer=p, points=p, step=256):
        return f(vertices, None, N, indices, T, None, 1, 1, 0, 0, z_near, cols, rows, zbuffer, points, step, None, 0, None)

    assert call(zbuffer=None) == 1 and b"z-buffer" in lib.dfa_last_error()
    for kw in (dict(cols=0), dict(rows=-1)):
        assert call(**kw) == 1 and b"non-positive image size" in lib.dfa_last_error()
    for kw in (dict(cols=8193, step=8193 * 16), dict(rows=8193)):
        assert call(**kw) == 1 and b"8192" in lib.dfa_last_error()
    for zn in (0.0, -1.0, float("nan")):
        assert call(z_near=zn) == 1 and b"z_near" in lib.dfa_last_error()
    assert call(T=-1) == 1 and call(N=-1) == 1
    assert call(vertices=None) == 1 and b"null mesh" in lib.dfa_last_error()
    assert call(indices=None) == 1 and call(N=0) == 1
    assert call(step=16 * 16 - 16) == 1 and b"row step" in lib.dfa_last_error()
    assert call(points=C.c_void_p(0x1004)) == 1 and b"aligned" in lib.dfa_last_error()
    assert call(zbuffer=C.c_void_p(0x1004)) == 1 and b"aligned" in lib.dfa_last_error()
