"""-m gpu parity tests of the rigid-ICP seam (src/kfusion/cuda/proj_icp.cu) vs the oracle.

Bar: the set of matched pixels is identical (integer count), the 27 sums agree to 1e-5 relative to the largest
sum (the reference itself tree-reduces floats, so its sums depend on the reduction order; the HIP kernel adds
float wave totals and double partials, the oracle adds doubles in pixel order).  The same bar against the independent
numpy statement tests/img_statement.py, which cross-checks the oracle on the CPU (tests/test_img_statement_cpu.py,
same matched set, sums within 1e-9); neither is pinned to reference outputs (the reference has no ICP tests)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import bits, dev, host, rot  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _frames(name="T1"):
    cfg = synth.CONFIGS[name]
    intr = synth.intrinsics(cfg)
    d0, d1 = synth.depth_frame(cfg, 0), synth.depth_frame(cfg, 4)
    return cfg, intr, d0, d1


@pytest.mark.parametrize("variant", ["depth", "points"])
@pytest.mark.parametrize("level", [0, 1])
def test_icp_sums_match_the_oracle(A, variant, level):
    cfg, intr, d0, d1 = _frames()
    fx, fy, cx, cy = intr
    # the reference's inputs: masked depth + normals per pyramid level (kinfu.cpp:150-175)
    m0, n0 = O.normals_mask_depth(d0, *intr)
    m1, n1 = O.normals_mask_depth(d1, *intr)
    P0, N0 = O.points_normals(d0, *intr)
    P1, N1 = O.points_normals(d1, *intr)
    if level == 1:
        m0, n0 = O.resize_depth_normals(m0, n0)
        m1, n1 = O.resize_depth_normals(m1, n1)
        P0, N0 = O.resize_points_normals(P0, N0)
        P1, N1 = O.resize_points_normals(P1, N1)
    div = 1 << level
    li = (fx / div, fy / div, cx / div, cy / div)
    aff = np.concatenate([rot([0.2, 1.0, 0.1], 0.01).astype(np.float32).reshape(-1), np.array([0.004, -0.003, 0.006], np.float32)])
    if variant == "depth":
        args = (m1, n1, m0, n0)
    else:
        args = (P1, N1, P0, N0)
    ref, matched = O.icp_sums(*args, aff, li)
    sums, m = A.icp_sums(*(dev(a) for a in args), aff, *li)
    assert int(host(m)[0]) == matched and matched > 0.5 * m0.size
    assert np.abs(host(sums).astype(np.float64) - ref).max() <= 1e-5 * np.abs(ref).max()


def test_icp_sums_no_overlap_and_errors(A):
    import torch
    cfg, intr, d0, d1 = _frames("T0")
    m0, n0 = O.normals_mask_depth(d0, *intr)
    far = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.array([5.0, 0, 0], np.float32)])  # nothing projects
    sums, m = A.icp_sums(dev(m0), dev(n0), dev(m0), dev(n0), far, *intr)
    assert int(host(m)[0]) == 0 and not host(sums).any()
    ident = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
    sums, m = A.icp_sums(dev(m0), dev(n0), dev(m0), dev(n0), ident, *intr)
    h = host(sums)
    assert int(host(m)[0]) > 0.97 * int((m0 != 0).sum())  # a frame matches itself (the re-projected pixel may round to a neighbour)
    assert np.abs(h[[6, 12, 17, 21, 24, 26]]).max() <= 1e-3 * np.abs(h).max()  # b ~ 0: already aligned (up to the re-projection rounding)
    with pytest.raises(A.DynfuAmdError):
        A.icp_sums(dev(m0), dev(n0), dev(m0), dev(n0), ident, 0.0, 1.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------------------------
# HIP against the independent numpy statement (tests/img_statement.py): the statement forms the rows and products in
# float32 as proj_icp.cu does and sums them in float64.
import img_statement as St  # noqa: E402


@pytest.mark.parametrize("variant", ["depth", "points"])
@pytest.mark.parametrize("level", [0, 1])
def test_icp_sums_match_the_statement(A, variant, level):
    cfg, intr, d0, d1 = _frames()
    if variant == "depth":
        (m0, n0), (m1, n1) = St.normals_mask_depth(d0, *intr), St.normals_mask_depth(d1, *intr)
        if level:
            (m0, n0), (m1, n1) = St.resize_depth_normals(m0, n0), St.resize_depth_normals(m1, n1)
        args = (m1, n1, m0, n0)
    else:
        (P0, N0), (P1, N1) = St.points_normals(d0, *intr), St.points_normals(d1, *intr)
        if level:
            (P0, N0), (P1, N1) = St.resize_points_normals(P0, N0), St.resize_points_normals(P1, N1)
        args = (P1, N1, P0, N0)
    li = tuple(v / (1 << level) for v in intr)
    for axis, ang, t in (([0.2, 1.0, 0.1], 0.01, [0.004, -0.003, 0.006]), ([1.0, 0.0, 0.3], 0.04, [-0.02, 0.01, 0.03])):
        aff = np.concatenate([rot(axis, ang).astype(np.float32).reshape(-1), np.array(t, np.float32)])
        want, ok, _ = St.icp(*args, aff, li)
        sums, m = A.icp_sums(*(dev(a) for a in args), aff, *li)
        assert int(host(m)[0]) == int(ok.sum()) and ok.sum() > 0.3 * ok.size
        assert np.abs(host(sums).astype(np.float64) - want).max() <= 1e-5 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------------------------
# The kernel against the float64 statement (img_statement.icp64), sum by sum: |got[q] - sum64[q]| <= c 2^-24 abs64[q]
# with abs64[q] the sum of |row_i row_j| over the matched pixels and c = 2048, measured on the CPU as 4 times the
# largest deviation of the float32 statements over the nine sizes (391.8 units, tests/test_img_statement_cpu.py; the
# nearly converged wall crop has its own measured c = 65536, from 9203.3 units), and the matched count
# exactly (no case has a knife-edge pixel, checked there too).  The cases are tests/icp_cases.py.
import icp_cases as K  # noqa: E402


def _gpu(A, args, aff, li, **kw):
    sums, m = A.icp_sums(*(a if hasattr(a, "is_cuda") else dev(a) for a in args), aff, *li, **kw)
    return host(sums), int(host(m)[0])


@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("name", list(K.CASES))
def test_icp_sums_per_sum_bar_over_the_shape_matrix(A, name, variant):
    args, li = K.inputs(name, variant)
    for pose in K.poses(name):
        aff = K.affine(pose)
        want, ok, _, sum64, abs64, knife = St.icp64(*args, aff, li)
        got, m = _gpu(A, args, aff, li)
        print(name, variant, "matched", m, "units", St.per_sum_units(got, sum64, abs64).max())
        assert knife == 0 and m == int(ok.sum())
        assert K.within_bar(got, sum64, abs64, K.c_of(name))
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-5 * np.abs(want).max()


def _pitched(a, extra):
    """the same image in a CUDA tensor whose rows are `extra` pixels longer; padding NaN (float4 maps) / 0xFFFF (depth)"""
    H, W = a.shape[:2]
    wide = np.full((H, W + extra) + a.shape[2:], 0xFFFF if a.dtype == np.uint16 else np.nan, a.dtype)
    wide[:, :W] = a
    return dev(wide)[:, :W]


@pytest.mark.parametrize("variant", K.VARIANTS)
def test_icp_sums_with_four_different_row_pitches_are_bit_equal(A, variant):
    args, li = K.inputs("37x53", variant)
    aff = K.affine(K.NEAR)
    flat, m = _gpu(A, args, aff, li)
    views = [_pitched(a, e) for a, e in zip(args, (3, 8, 1, 5))]
    assert len({v.stride(0) * v.element_size() for v in views}) == 4 and not any(v.is_contiguous() for v in views)
    got, mp = _gpu(A, views, aff, li)
    assert mp == m and m > 0 and np.array_equal(bits(got), bits(flat))


IDENT = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
EH, EW, EINTR = 8, 40, (256.0, 256.0, 19.5, 3.5)  # s = p, and u, v exact in float32 with or without an fma
f32 = np.float32


def _ray(x, y, z=1.0):
    return [f32(x - 19.5) / f32(256) * f32(z), f32(y - 3.5) / f32(256) * f32(z), f32(z), 0]


def _edge_inputs(cur, prv, ncur=(0, 0, -1), nprv=(0, 0, -1), at=(5, 3), reads=None):
    """points-variant maps with one live pixel `at` = (x, y) holding `cur`; `prv` sits where it projects (`reads`)"""
    C = np.full((EH, EW, 4), St.QNAN, np.float32)
    P, NC, NP = C.copy(), C.copy(), C.copy()
    rx, ry = reads or at
    C[at[1], at[0]], P[ry, rx] = cur, prv
    NC[at[1], at[0], :3], NP[ry, rx, :3] = ncur, nprv
    return C, NC, P, NP


up = lambda v: np.nextafter(f32(v), f32(np.inf))  # noqa: E731
down = lambda v: np.nextafter(f32(v), f32(-np.inf))  # noqa: E731
EDGES = {
    # name: (inputs, dist_thres, angle_thres, matched pixels)
    "dist2 on the threshold": (_edge_inputs(_ray(5, 3), [_ray(5, 3)[0], _ray(5, 3)[1], 1.125, 0]), 0.125, 0.35, 1),
    "dist2 one float above": (_edge_inputs(_ray(5, 3), [_ray(5, 3)[0], _ray(5, 3)[1], up(1.125), 0]), 0.125, 0.35, 0),
    "cos on min_cosine = 1": (_edge_inputs(_ray(5, 3), _ray(5, 3)), 0.125, 0.0, 1),
    "cos one float under 1": (_edge_inputs(_ray(5, 3), _ray(5, 3), nprv=(0, 0, -down(1))), 0.125, 0.0, 0),
    "perpendicular normals under 1.6 rad": (_edge_inputs(_ray(5, 3), _ray(5, 3), nprv=(1, 0, 0)), 0.125, 1.6, 1),
    "s.z zero": (_edge_inputs([0.01, 0.01, 0, 0], _ray(5, 3)), 0.125, 0.35, 0),
    "s.z negative": (_edge_inputs([0.01, 0.01, -1, 0], _ray(5, 3)), 0.125, 0.35, 0),
    "u on cols": (_edge_inputs(_ray(EW, 3), _ray(EW - 1, 3), reads=(EW - 1, 3)), 0.125, 0.35, 0),
    "u one float under cols": (_edge_inputs([down(down(_ray(EW, 3)[0])), _ray(EW, 3)[1], 1, 0], _ray(EW - 1, 3), reads=(EW - 1, 3)), 0.125, 0.35, 1),
    # (u = -0.0 cannot come out of fma(fx, x / z, cx) with cx > 0: the exact cancellation rounds to +0)
    "u zero": (_edge_inputs(_ray(0, 3), _ray(0, 3), at=(0, 3)), 0.125, 0.35, 1),
    "v on rows": (_edge_inputs(_ray(5, EH), _ray(5, EH - 1), reads=(5, EH - 1)), 0.125, 0.35, 0),
    "v one float under rows": (_edge_inputs([_ray(5, EH)[0], down(_ray(5, EH)[1]), 1, 0], _ray(5, EH - 1), reads=(5, EH - 1)), 0.125, 0.35, 1),
    "v zero": (_edge_inputs(_ray(5, 0), _ray(5, 0), at=(5, 0)), 0.125, 0.35, 1),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_icp_gate_edges_points_variant(A, edge):
    args, dist, ang, matched = EDGES[edge]
    want, ok, _, sum64, abs64, _ = St.icp64(*args, IDENT, EINTR, dist_thres=dist, angle_thres=ang)
    assert int(ok.sum()) == matched, "the statement itself"
    got, m = _gpu(A, args, IDENT, EINTR, dist_thres=dist, angle_thres=ang)
    assert m == matched and np.array_equal(got.astype(np.float64), want)  # one pixel: float32 products, nothing to round


def test_icp_gate_edges_depth_variant(A):
    """whole millimetres along one ray: 124 mm apart is kept; 125 mm is dropped, because the re-projected d also lies
    125 mm (u - cx) / f to the side and no pixel sits on the axis of a half-integer cx, so dist2 = 0.125^2 exactly is out of
    this variant's reach.  With them the image's last column and row (u = cols - 1, v = rows - 1 project inside).
    Then a translation of exactly one pixel at z = 1 m (1 / 256 m along x, along y): the last column / row lands on
    u == cols / v == rows and is dropped, its neighbour lands on the last column / row and is kept."""
    N = np.zeros((EH, EW, 4), np.float32)
    N[..., 2] = -1
    for gap, matched in ((124, 3), (125, 2)):
        D0, D1 = np.zeros((EH, EW), np.uint16), np.zeros((EH, EW), np.uint16)
        for x, y in ((5, 3), (EW - 1, 2), (7, EH - 1)):
            D0[y, x] = D1[y, x] = 1000
        D0[3, 5] = 1000 + gap
        want, ok, _, sum64, abs64, _ = St.icp64(D1, N, D0, N, IDENT, EINTR, dist_thres=0.125)
        got, m = _gpu(A, (D1, N, D0, N), IDENT, EINTR, dist_thres=0.125)
        assert int(ok.sum()) == matched == m and K.within_bar(got, sum64, abs64)
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-5 * np.abs(want).max()
    for t, live, kept in (((1 / 256, 0, 0), ((EW - 1, 2), (EW - 2, 2)), (EW - 2, 2)), ((0, 1 / 256, 0), ((5, EH - 1), (5, EH - 2)), (5, EH - 2))):
        D0, D1 = np.zeros((EH, EW), np.uint16), np.zeros((EH, EW), np.uint16)
        for x, y in live:
            D1[y, x] = 1000
        D0[live[0][1], live[0][0]] = 1000  # where the kept neighbour lands
        aff = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.array(t, np.float32)])
        want, ok, _, sum64, abs64, _ = St.icp64(D1, N, D0, N, aff, EINTR, dist_thres=0.125)
        assert ok.sum() == 1 and ok[kept[1], kept[0]], "the statement itself"
        got, m = _gpu(A, (D1, N, D0, N), aff, EINTR, dist_thres=0.125)
        assert m == 1 and K.within_bar(got, sum64, abs64)
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("which", ["nprev", "ncurr"])
def test_icp_nan_normal_on_a_valid_pair_is_counted_and_poisons_the_sums(A, which):
    """!(|cos| < min_cosine) keeps a NaN cosine, as the reference's `cosine < min_cosine` return does (proj_icp.cu:66-68,
    :94-96).  A NaN nprev is in the row: every sum is NaN.  A NaN ncurr only enters the gate: the sums stay finite."""
    args, li = K.inputs("37x53", "points")
    args = [a.copy() for a in args]
    aff = K.affine(K.NEAR)
    _, ok, *_ = St.icp64(*args, aff, li)
    y, x = np.argwhere(ok)[ok.sum() // 2]
    if which == "ncurr":
        args[1][y, x, :3] = np.nan
    else:
        T = St._icp_terms(*args, aff, li, 0.1, 0.3490658503988659)
        args[3][T["iw"][y, x], T["iu"][y, x], :3] = np.nan
    want, ok2, _, sum64, abs64, _ = St.icp64(*args, aff, li)
    got, m = _gpu(A, args, aff, li)
    assert ok2[y, x] and m == int(ok2.sum())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any() == (which == "nprev")
    assert K.within_bar(got, sum64, abs64)
    args[0][y, x] = np.nan  # the vertex too: the pixel is gone, the sums are finite
    if which == "nprev":
        args[2][T["iw"][y, x], T["iu"][y, x]] = np.nan
    want, ok3, _, sum64, abs64, _ = St.icp64(*args, aff, li)
    got, m = _gpu(A, args, aff, li)
    assert m == int(ok3.sum()) < int(ok2.sum()) and np.isfinite(got).all() and K.within_bar(got, sum64, abs64)


def test_icp_sums_without_a_matched_counter_are_bit_equal(A):
    """the C++ adaptor passes matched = NULL (host/src/projective_icp.cpp)"""
    import ctypes as C
    import torch
    from dynfu_amd import _lib
    args, li = K.inputs("37x53", "points")
    aff = K.affine(K.NEAR)
    counted, m = _gpu(A, args, aff, li)
    t = [dev(a) for a in args]
    sums = torch.full((27,), float("nan"), dtype=torch.float32, device="cuda")
    rc = _lib.load().dfa_icp_sums(0, C.c_void_p(t[0].data_ptr()), 53 * 16, C.c_void_p(t[1].data_ptr()), 53 * 16,
                                  C.c_void_p(t[2].data_ptr()), 53 * 16, C.c_void_p(t[3].data_ptr()), 53 * 16, 53, 37,
                                  _lib._aff12(aff), *[float(v) for v in li], 0.1, 0.3490658503988659,
                                  C.c_void_p(sums.data_ptr()), None, _lib._stream())
    torch.cuda.synchronize()
    assert rc == 0 and m > 0 and np.array_equal(bits(host(sums)), bits(counted))


def test_icp_scratch_grown_shrunk_and_grown_again_on_one_stream(A):
    import torch
    big, small = K.inputs("1280x720", "depth"), K.inputs("37x53", "depth")
    aff = K.affine(K.NEAR)
    with torch.cuda.stream(torch.cuda.Stream()):
        first = [_gpu(A, a, aff, li) for a, li in (big, small, big)]
        again = [_gpu(A, a, aff, li) for a, li in (big, small, big)]
    for (s0, m0), (s1, m1) in zip(first, again):
        assert m0 == m1 > 0 and np.array_equal(bits(s0), bits(s1))
    assert np.array_equal(bits(first[0][0]), bits(first[2][0]))


def test_icp_on_two_streams_from_one_thread(A):
    """each (device, stream) has its own partial-sum scratch: alternating launches on two streams do not mix them"""
    import torch
    cases = [K.inputs("640x480", "points"), K.inputs("37x53", "points")]
    aff = K.affine(K.NEAR)
    tens = [([dev(a) for a in args], li) for args, li in cases]
    alone = [_gpu(A, t, aff, li) for t, li in tens]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = [[], []]
    for _ in range(10):
        for k in (0, 1):
            with torch.cuda.stream(streams[k]):
                out[k].append(A.icp_sums(*tens[k][0], aff, *tens[k][1]))
    torch.cuda.synchronize()
    for k in (0, 1):
        for sums, m in out[k]:
            assert int(host(m)[0]) == alone[k][1] and np.array_equal(bits(host(sums)), bits(alone[k][0]))


@pytest.mark.parametrize("config,variant", list(K.POSE_BARS))
def test_icp_whole_schedule_follows_the_fp64_trajectory(A, config, variant):
    """{10, 5, 4} iterations over three levels from the identity: the kernel's sums and the statement's sum64 each drive
    St.icp_update.  After every iteration the kernel's matched count is the statement's at the same pose (or within the
    statement's knife-edge count there) and the two poses agree to K.POSE_BARS, 4 times the float32-to-fp64 gap measured on
    the CPU; the final pose recovers the rendered camera motion to 3e-3 / 5e-3 (tests/cpp/test_host_icp.cpp)."""
    pyr = K.pyramids(config, variant)
    on_gpu = {lv: [dev(a) for a in args] for lv, (args, _) in enumerate(pyr)}
    level_of = {id(args): lv for lv, (args, _) in enumerate(pyr)}
    counts = []

    def kernel_sums(args, li, aff):
        sums, m = A.icp_sums(*on_gpu[level_of[id(args)]], aff, *li, **K.GATES)
        _, ok, _, _, _, knife = St.icp64(*args, aff, li, **K.GATES)
        counts.append((int(host(m)[0]), int(ok.sum()), knife))
        return host(sums).astype(np.float64)
    got = K.iterate(config, variant, kernel_sums)
    want = K.iterate(config, variant, K.sums64)
    for it, (m, n, knife) in enumerate(counts):
        assert abs(m - n) <= knife, (it, m, n, knife)
    gaps = K.level_gaps(got, want)
    print(config, variant, "gaps", gaps, "bars", K.POSE_BARS[config, variant])
    for (lv, x), (_, y) in zip(got, want):
        assert np.abs(x.astype(np.float64) - y).max() <= K.POSE_BARS[config, variant][lv], (lv, gaps)
    R, t = K.motion()
    final = got[-1][1].astype(np.float64)
    assert np.abs(final[:9].reshape(3, 3) - R).max() <= 3e-3 and np.abs(final[9:] - t).max() <= 5e-3
