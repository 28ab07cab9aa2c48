"""CPU checks of the depth pre-processing and the rigid ICP against a second, independent reading of the reference
(tests/img_statement.py, a numpy statement of imgproc.cu and proj_icp.cu):

- hand-computed answers on hand-made inputs, independent of both the statement and oracle/img_oracle.c, icp_oracle.c;
- the statement equals the C oracle bit for bit (depth, points and normals; undefined outputs are the reference's
  0x7fffffff NaN) on seeded images of 1x1, 37x53 and 8x130 pixels and on the synthetic frames;
- the ICP's matched pixels are the statement's, and the oracle's 27 sums agree with the statement's to 1e-9 of the
  largest: both add the same float32 products in float64, in different orders.
The HIP kernels are compared with the statement by the -m gpu tests of tests/test_gpu_img.py and test_gpu_icp.py."""
import numpy as np
import pytest

import img_statement as S
import oracle as O
from dynfu_amd import synth
from gpu_util_cpu import rot

SHAPES = [(1, 1), (37, 53), (8, 130), (2, 3), (9, 200)]
FILTERS = [(7, 4.5, 0.04), (3, 1.0, 0.2), (17, 6.0, 0.05), (4, 2.0, 0.03)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _depth(H, W, seed):
    rng = np.random.default_rng(seed)
    d = (1200 + 400 * np.sin(np.arange(W) / 11.0)[None, :] + 300 * np.cos(np.arange(H) / 7.0)[:, None]
         + rng.normal(0, 6, (H, W))).astype(np.uint16)
    d[rng.random((H, W)) < 0.05] = 0
    d[rng.random((H, W)) < 0.01] = 9000
    return d


def _intr(H, W):
    return 525.0 * W / 640, 520.0 * W / 640, W / 2 - 0.5, H / 2 - 0.5


# ------------------------------------------------------------------------------------------------ hand-made ----
def test_constant_depth_through_bilateral_pyramid_and_resize():
    H, W, c = 12, 10, 1234
    d = np.full((H, W), c, np.uint16)
    # bilateral: every pixel keeps its value, the last row and column included (their windows exclude themselves
    # but hold only equal values); a 1-pixel-wide image has an empty window: 0 / 0 -> 0
    for ksz, ss, sd in FILTERS:
        assert (S.bilateral(d, ksz, ss, sd) == c).all()
    assert S.bilateral(np.full((5, 1), c, np.uint16), 7, 4.5, 0.04).tolist() == [[0]] * 5
    assert S.bilateral(np.full((1, 1), c, np.uint16), 7, 4.5, 0.04).tolist() == [[0]]
    # pyramid: (rows/2, cols/2) of the constant
    assert S.depth_pyr(d, 0.04).shape == (6, 5) and (S.depth_pyr(d, 0.04) == c).all()
    # resize: the mean of each 2x2 block; a block with a zero gives 0
    n = np.zeros((H, W, 4), np.float32)
    n[..., 2] = -1
    d2 = d.copy()
    d2[3, 4] = 0
    D, N = S.resize_depth_normals(d2, n)
    assert D[1, 2] == 0 and np.isnan(N[1, 2]).all()
    keep = np.ones(D.shape, bool)
    keep[1, 2] = False
    assert (D[keep] == c).all() and (N[..., 2][keep] == -1).all()


def test_pyramid_window_is_the_5x5_block_around_2x_2y_without_the_last_row_and_column():
    H, W = 10, 10
    d = np.full((H, W), 1000, np.uint16)
    d[0, 0] = 1000 + 90  # within 3 sigma = 120 mm: averaged in
    d[3, 3] = 2000       # outside: not counted
    d[4, 4] = 1000 + 60  # inside the window of (y, x) = (1, 1): rows / columns 0 .. 4
    d[9, :] = 1100       # the last row: never in a window
    P = S.depth_pyr(d, 0.04)
    assert P[0, 0] == (1090 + 1000 * 8) // 9  # window rows / cols 0 .. 2 of the centre (0, 0)
    assert P[1, 1] == (1090 + 1060 + 1000 * 22) // 24
    assert P[4, 4] == 1000  # rows / cols 6 .. 8: row 9 excluded
    assert np.array_equal(P, O.depth_pyr(d, 0.04))


def test_bilateral_window_excludes_the_last_row_and_column():
    d = np.full((4, 4), 1000, np.uint16)
    d[3, :] = 1100  # the last row: outside every window
    d[:, 3] = 1100
    out = S.bilateral(d, 3, 1.0, 1.0)
    assert (out[:3, :3] == 1000).all() and (out[3, :] == 1000).all() and (out[:, 3] == 1000).all()
    assert np.array_equal(out, O.bilateral(d, 3, 1.0, 1.0))


def test_frame_against_itself_matches_every_valid_pixel_with_zero_residual():
    cfg = synth.CONFIGS["T0"]
    intr = synth.intrinsics(cfg)
    # a fronto-parallel plane: re-projection is exact, so every valid pixel finds itself
    d = np.full((cfg["height"], cfg["width"]), 1000, np.uint16)
    d[10:20, 30:50] = 0
    m, n = S.normals_mask_depth(d, *intr)
    ident = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
    for args in ((m, n, m, n), S.points_normals(d, *intr) * 2):
        sums, ok, rows = S.icp(*args, ident, intr)
        assert np.array_equal(ok, m != 0)
        assert (rows[..., 6] == 0).all() and sums[[6, 12, 17, 21, 24, 26]].tolist() == [0] * 6  # b = 0
        assert sums[25] == pytest.approx(ok.sum())  # n_z^2 summed: the plane's normal is (0, 0, -1)


# ------------------------------------------------------------------------------------ statement == oracle ----
@pytest.mark.parametrize("shape", SHAPES)
def test_bilateral_equals_oracle(shape):
    d = _depth(*shape, seed=shape[1])
    for ksz, ss, sd in FILTERS:
        assert np.array_equal(S.bilateral(d, ksz, ss, sd), O.bilateral(d, ksz, ss, sd)), (ksz, ss, sd)


def test_exp_neg_equals_oracle():
    x = -np.random.default_rng(0).uniform(0, 100, 2000).astype(np.float32)
    x = np.concatenate([x, np.float32([0, -0.0, -87.3, -87.4, -1e-30])])
    L = O._libimg()
    assert np.array_equal(bits(S.exp_neg(x)), bits([L.orc_exp_neg(float(v)) for v in x]))


@pytest.mark.parametrize("shape", SHAPES)
def test_truncate_pyramid_normals_resizers_equal_oracle(shape):
    d = _depth(*shape, seed=7)
    intr = _intr(*shape)
    assert np.array_equal(S.truncate_depth(d, 1.4), O.truncate_depth(d, 1.4))
    for sd in (0.04, 0.01):
        assert np.array_equal(S.depth_pyr(d, sd), O.depth_pyr(d, sd))
    m, n = S.normals_mask_depth(d, *intr)
    mo, no = O.normals_mask_depth(d, *intr)
    assert np.array_equal(m, mo) and np.array_equal(bits(n), bits(no))
    P, N = S.points_normals(d, *intr)
    Po, No = O.points_normals(d, *intr)
    assert np.array_equal(bits(P), bits(Po)) and np.array_equal(bits(N), bits(No))
    for a, b in zip(S.resize_depth_normals(m, n), O.resize_depth_normals(mo, no)):
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
    for a, b in zip(S.resize_points_normals(P, N), O.resize_points_normals(Po, No)):
        assert np.array_equal(bits(a), bits(b))


def test_undefined_outputs_are_the_reference_quiet_nan():
    """imgproc.cu writes numeric_limits<float>::quiet_NaN() = 0x7fffffff (temp_utils.hpp:21) for an undefined normal
    or point (:139, :196, :269, :323); the oracle once wrote C's NAN (0x7fc00000)"""
    d = _depth(9, 12, 3)
    intr = _intr(9, 12)
    _, n = O.normals_mask_depth(d, *intr)
    P, N = O.points_normals(d, *intr)
    assert (bits(n[-1, :, :3]) == 0x7FFFFFFF).all() and (bits(P[:, -1]) == 0x7FFFFFFF).all()
    assert (bits(N[:, -1]) == 0x7FFFFFFF).all()
    d2, n2 = O.resize_depth_normals(np.zeros((4, 4), np.uint16), n[:4, :4])
    v2, m2 = O.resize_points_normals(P[-2:, -2:], N[-2:, -2:])
    assert (bits(n2) == 0x7FFFFFFF).all() and (bits(v2[..., :3]) == 0x7FFFFFFF).all() and (v2[..., 3] == 0).all()


def _icp_inputs(name, level, variant):
    cfg = synth.CONFIGS[name]
    intr = synth.intrinsics(cfg)
    d0, d1 = synth.depth_frame(cfg, 0), synth.depth_frame(cfg, 4)
    if variant == "depth":
        m0, n0 = S.normals_mask_depth(d0, *intr)
        m1, n1 = S.normals_mask_depth(d1, *intr)
        if level:
            (m0, n0), (m1, n1) = S.resize_depth_normals(m0, n0), S.resize_depth_normals(m1, n1)
        args = (m1, n1, m0, n0)
    else:
        P0, N0 = S.points_normals(d0, *intr)
        P1, N1 = S.points_normals(d1, *intr)
        if level:
            (P0, N0), (P1, N1) = S.resize_points_normals(P0, N0), S.resize_points_normals(P1, N1)
        args = (P1, N1, P0, N0)
    div = 1 << level
    li = tuple(v / div for v in intr)
    return args, li


@pytest.mark.parametrize("variant", ["depth", "points"])
@pytest.mark.parametrize("level", [0, 1])
def test_icp_matches_and_sums_equal_oracle(variant, level):
    args, li = _icp_inputs("T0", level, variant)
    for axis, ang, t in (([0.2, 1.0, 0.1], 0.01, [0.004, -0.003, 0.006]), ([1, 0, 0.3], 0.05, [0.02, 0.01, -0.03])):
        aff = np.concatenate([rot(axis, ang).astype(np.float32).reshape(-1), np.array(t, np.float32)])
        sums, ok, _ = S.icp(*args, aff, li)
        ref, matched = O.icp_sums(*args, aff, li)
        assert ok.sum() == matched and matched > 0.3 * ok.size
        assert np.abs(sums - ref).max() <= 1e-9 * np.abs(ref).max()


def test_icp_sum_layout_is_the_upper_triangle_with_b():
    """StreamHelper::get (projective_icp.cpp:39-57) reads the 27 sums as A[i][j], j >= i, then b[i], row by row"""
    args, li = _icp_inputs("T0", 0, "depth")
    aff = np.concatenate([rot([0.2, 1.0, 0.1], 0.01).astype(np.float32).reshape(-1), np.array([0.004, -0.003, 0.006], np.float32)])
    sums, ok, rows = S.icp(*args, aff, li)
    r = rows[ok].astype(np.float64)
    q = 0
    for i in range(6):
        for j in range(i, 7):
            assert sums[q] == pytest.approx(np.dot(r[:, i], r[:, j]), rel=1e-6, abs=1e-9)
            q += 1
    ref, _ = O.icp_sums(*args, aff, li)
    A = np.zeros((6, 6))
    b = np.zeros(6)
    q = 0
    for i in range(6):
        for j in range(i, 7):
            if j == 6:
                b[i] = ref[q]
            else:
                A[i, j] = A[j, i] = ref[q]
            q += 1
    assert np.allclose(A, r[:, :6].T @ r[:, :6], rtol=1e-6, atol=1e-9) and np.allclose(b, r[:, :6].T @ r[:, 6], rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------- the ICP statement at the shapes of the GPU test ----
import functools  # noqa: E402

import icp_cases as K  # noqa: E402

CASE_IDS = [(name, variant) for name in K.CASES for variant in K.VARIANTS]


@functools.lru_cache(maxsize=None)
def _stated(name, variant):
    """per pose of the case: (affine, icp64's six results, the fused float32 statement's sums and mask)"""
    args, li = K.inputs(name, variant)
    out = []
    for pose in K.poses(name):
        aff = K.affine(pose)
        fused, okf, _ = S.icp(*args, aff, li, fused=True)
        out.append((aff, S.icp64(*args, aff, li), fused, okf))
    return out


@pytest.mark.parametrize("name,variant", CASE_IDS)
def test_icp_equals_oracle_at_the_ragged_and_large_shapes(name, variant):
    args, li = K.inputs(name, variant)
    best = 0.0
    for aff, (sums, ok, _, sum64, abs64, _), _, _ in _stated(name, variant):
        ref, matched = O.icp_sums(*args, aff, li)
        assert ok.sum() == matched
        assert np.abs(sums - ref).max() <= 1e-9 * np.abs(ref).max()
        assert (abs64 >= np.abs(sum64)).all()
        best = max(best, ok.mean())
    assert best >= K.CASES[name][4]


@pytest.mark.parametrize("name,variant", CASE_IDS)
def test_icp_cases_have_no_knife_edge_pixel(name, variant):
    """a condition on the inputs: at no pixel is a gate quantity within 4 float32 ulps of its threshold, so a contracted
    a*b + c cannot decide membership differently; the fused statement's mask is the same by construction"""
    for _, (_, ok, _, _, _, knife), _, okf in _stated(name, variant):
        assert knife == 0 and np.array_equal(ok, okf)


def test_knife_edge_pixels_are_counted():
    """one pixel with dist2 on the threshold, one with u one ulp under cols, one well inside every gate"""
    H, W = 8, 40
    P = np.full((H, W, 4), S.QNAN, np.float32)
    N = np.zeros((H, W, 4), np.float32)
    N[..., 2] = -1
    intr = (256.0, 256.0, 19.5, 3.5)

    def at(x, y, z=1.0):
        return [(x - 19.5) / 256 * z, (y - 3.5) / 256 * z, z, 0]
    P[2, 3], P[4, 5], P[6, 7] = at(3, 2), at(5, 4), at(7, 6)
    C = P.copy()
    P[2, 3, 2] = 1.125                                                      # dist2 == 0.125^2, on the threshold
    C[4, 5, 0] = np.nextafter(np.float32((W - 19.5) / 256), np.float32(0))  # u just under cols
    ident = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
    *_, knife = S.icp64(C, N, P, N, ident, intr, dist_thres=0.125)
    assert knife == 2


def test_icp_update_solves_the_unpacked_system():
    (aff, (sums, *_), _, _), *_ = _stated("640x480", "points")
    A, b = S.unpack_sums(sums)
    assert np.array_equal(A, A.T) and b.tolist() == sums[S.B_SUMS].tolist() and A[0, 1] == sums[1] and A[5, 5] == sums[25]
    x = np.linalg.solve(A, b)
    assert np.abs(A @ x - b).max() <= 64 * np.finfo(np.float64).eps * (np.abs(A) @ np.abs(x) + np.abs(b)).max()
    ok, nxt = S.icp_update(sums, aff)
    want_R = S.rodrigues(x[:3]) @ aff[:9].reshape(3, 3).astype(np.float64)
    want_t = S.rodrigues(x[:3]) @ aff[9:].astype(np.float64) + x[3:]
    assert ok and nxt.dtype == np.float32
    assert np.array_equal(nxt, np.concatenate([want_R.reshape(-1), want_t]).astype(np.float32))
    R = nxt[:9].reshape(3, 3).astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6  # still a rotation
    # zero right-hand side: the pose stays; Rodrigues below the reference's epsilon is the identity
    zero_b = sums.copy()
    zero_b[S.B_SUMS] = 0
    ok, same = S.icp_update(zero_b, aff)
    assert ok and np.array_equal(same, aff)
    assert np.array_equal(S.rodrigues([1e-17, 0, 0]), np.eye(3)) and S.rodrigues([0, 0, 1e-9])[0, 1] == -1e-9


def test_icp_update_refuses_singular_systems():
    aff = K.affine(K.NEAR)
    ok, same = S.icp_update(np.zeros(27), aff)
    assert not ok and np.array_equal(same, aff)
    rows = np.random.default_rng(3).normal(0, 1, (200, 7))
    rows[:, 5] = 0  # rank 5: a zero row and column
    sums = np.array([rows[:, i] @ rows[:, j] for i, j in S.SUM_PAIRS])
    assert not S.icp_update(sums, aff)[0]
    rows[:, 5] = rows[:, 4]  # rank 5 without a zero: two equal columns
    sums = np.array([np.float32(rows[:, i] @ rows[:, j]) for i, j in S.SUM_PAIRS], np.float64)
    assert not S.icp_update(sums, aff)[0]
    sums[0] = np.nan
    assert not S.icp_update(sums, aff)[0]


MATRIX_UNITS, MATRIX_WORST_AT, WALL_UNITS = 391.8, ("1x1", "depth"), 9203.3


def test_the_constants_of_the_per_sum_bar_are_four_times_the_measured_deviations():
    """c of |got[q] - sum64[q]| <= c 2^-24 abs64[q] is measured, not picked: the largest deviation from sum64 of the
    float32 statement and of its fused reading, in units of 2^-24 abs64[q], over every variant and pose of the cases of
    tests/icp_cases.py; c is 4 times that, rounded up to a power of two (the kernel adds 8 float additions per workgroup
    partial on top of either statement's roundings).

    Over the nine sizes of the shape matrix: MATRIX_UNITS = 391.8 (1x1, depth variant, TINY pose: one pixel, nothing
    averages; the largest of the other sizes is 269.5 at 8x130, points, MID pose, sum 21 = b[3]), hence K.C_BAR = 2048.  The nearly converged wall crop has a
    constant of its own: WALL_UNITS = 9203.3 (depth, sum 6 = b[0], float32 statement; its fused reading 18.9), hence
    K.C_BAR_CONVERGED = 65536: at a residual of 0.1 mm d - s cancels four digits, the same rounding of fl(R p) + t at every
    pixel of a flat wall, and abs64 of a b sum does not see it.  The two figures are asserted below to their first three
    digits."""
    worst = {False: (0.0, None), True: (0.0, None)}
    for name, variant in CASE_IDS:
        for _, (sums, _, _, sum64, abs64, _), fused, _ in _stated(name, variant):
            u = max(S.per_sum_units(sums, sum64, abs64).max(), S.per_sum_units(fused, sum64, abs64).max())
            print("%-11s %-6s %9.1f" % (name, variant, u))
            conv = name in K.CONVERGED_CASES
            if u > worst[conv][0]:
                worst[conv] = (u, (name, variant))
    print("largest deviations in units of 2^-24 abs64:", worst)
    assert worst[False][1] == MATRIX_WORST_AT and worst[False][0] == pytest.approx(MATRIX_UNITS, rel=5e-3)
    assert worst[True][1] == ("37x53-wall", "depth") and worst[True][0] == pytest.approx(WALL_UNITS, rel=5e-3)
    assert K.C_BAR == 2 ** int(np.ceil(np.log2(4 * worst[False][0]))) == 2048
    assert K.C_BAR_CONVERGED == 2 ** int(np.ceil(np.log2(4 * worst[True][0]))) == 65536


def test_the_per_sum_bar_catches_what_the_largest_sum_bar_misses():
    """Two mutations of the float32 rows of the ragged 37x53 wall case (nearly aligned, as in a level's last
    iterations), both in b, the vector that moves the camera: one 64-pixel wave (two 32-pixel rows of a tile) does not
    reach the six b sums; b's sign is flipped on the last image row.  Both pass max|d| <= 1e-5 max|sums| and fail the
    per-sum bar.  (Dropping the wave from all 27 sums also fails the old bar: 64 of 1961 pixels is 3 % of the largest
    sum too.  The old bar is blind where the residual is small against the normals' unit length.)"""
    (_, (sums, ok, rows, sum64, abs64, _), _, _), = _stated("37x53-wall", "points")
    c = K.c_of("37x53-wall")

    def old_bar(got):
        return np.abs(got - sum64).max() <= 1e-5 * np.abs(sum64).max()
    assert K.within_bar(sums, sum64, abs64, c) and old_bar(sums)
    wave = rows.copy()
    assert ok[8:10, 0:32].all()
    wave[8:10, 0:32, 6] = 0
    got = S.sums_of_rows(wave)
    assert not K.within_bar(got, sum64, abs64, c) and old_bar(got)
    wave[8:10, 0:32, :] = 0
    assert not K.within_bar(S.sums_of_rows(wave), sum64, abs64, c) and not old_bar(S.sums_of_rows(wave))
    flip = rows.copy()
    assert ok[-1].all()
    flip[-1, :, 6] *= -1
    got = S.sums_of_rows(flip)
    assert not K.within_bar(got, sum64, abs64, c) and old_bar(got)


@pytest.mark.parametrize("config,variant", list(K.POSE_BARS))
def test_pose_bar_is_four_times_the_float32_to_fp64_trajectory_gap(config, variant):
    """The {10, 5, 4} schedule on a rendered scene with a known camera motion (tests/icp_cases.py), once driven by the
    float32 statement's sums rounded to float32 and once by sum64, both through icp_update.  The largest pose-entry
    difference per level is the measured reference of the GPU-driven trajectory's bar, K.POSE_BARS = 4 x that (two
    digits, rounded up; recorded within a quarter, so that another BLAS may move the last digit).  Both trajectories
    recover the motion as tightly as tests/cpp/test_host_icp.cpp demands: rotation 3e-3, translation 5e-3."""
    a, b = K.iterate(config, variant, K.sums32), K.iterate(config, variant, K.sums64)
    gaps = K.level_gaps(a, b)
    print(config, variant, "gaps", gaps, "bars", K.POSE_BARS[config, variant])
    for gap, bar in zip(gaps, K.POSE_BARS[config, variant]):
        assert bar / 1.25 <= 4 * gap <= bar * 1.0001
    R, t = K.motion()
    for traj in (a, b):
        final = traj[-1][1].astype(np.float64)
        assert np.abs(final[:9].reshape(3, 3) - R).max() <= 3e-3 and np.abs(final[9:] - t).max() <= 5e-3
