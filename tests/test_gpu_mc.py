"""-m gpu parity tests of the marching-cubes seam: HIP kernels (through the C ABI) vs the CPU oracle.

Bar: BIT-EXACT — vertex count, order (ascending linear voxel index) and the float bits of every
point, with the library's default case tables and with the reference's own tables
(tests/golden/ref_mc_tables.bin).  The oracle is unpinned (the reference has
no marching-cubes test), see oracle/mc_oracle.c."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
import reference_data  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402
from mc_util import blob_volume, default_tables, pack  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _tables(which):
    return default_tables() if which == "default" else reference_data.mc_tables()


def _run(A, vol, cell, tri, nv, cap):
    pts, total = A.marching_cubes(dev(vol), cell, dev(tri), dev(nv), cap)
    total = int(host(total)[0])
    return host(pts)[: min(total, cap)], total


@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("dims", [(64, 64, 64), (128, 128, 128), (50, 38, 44), (256, 24, 40), (260, 9, 7), (2, 2, 2),
                                  (67, 5, 130)])
def test_marching_cubes_bit_exact(A, dims, which):
    tri, nv = _tables(which)
    vol = blob_volume(dims, seed=sum(dims))
    cell = np.array([3.0 / dims[0], 2.5 / dims[1], 3.5 / dims[2]], np.float32)
    ref, total, _ = O.marching_cubes(vol, cell, tri, nv)
    got, gtotal = _run(A, vol, cell, tri, nv, max(total, 1))
    assert gtotal == total
    assert np.array_equal(bits(got), bits(ref))


def test_marching_cubes_of_an_integrated_depth_frame(A):
    """the producer/consumer chain of DynFusion::operator(): integrate a depth frame, extract the mesh"""
    import torch
    cfg = synth.CONFIGS["T1"]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    depth = synth.depth_frame(cfg, 0)
    dists = torch.empty(depth.shape, dtype=torch.uint16, device="cuda")
    A.compute_dists(dev(depth), dists, fx, fy, cx, cy)
    dim = cfg["dim"]
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)
    tri, nv = default_tables()
    hv = host(vol).view(np.uint32)
    ref, total, occ = O.marching_cubes(hv, voxel, tri, nv)
    assert total > 10000 and occ > 3000
    pts, gtotal = A.marching_cubes(vol, voxel, dev(tri), dev(nv), total)
    assert int(host(gtotal)[0]) == total
    assert np.array_equal(bits(host(pts)), bits(ref))
    # the mesh is the depth surface: vertices (volume frame) -> camera frame lie on the sphere / plane
    p = ref[:, :3] + np.array(synth.VOLUME_POSE_T, np.float32)
    r = np.linalg.norm(p - synth.SPHERE_C, axis=1)
    on_sphere = np.abs(r - synth.SPHERE_R) < 0.03
    on_plane = np.abs(p[:, 2] - synth.PLANE_Z) < 0.03
    assert (on_sphere | on_plane).mean() > 0.97  # the rest: depth discontinuity at the silhouette


def test_marching_cubes_capacity_count_only_and_errors(A):
    import torch
    tri, nv = default_tables()
    vol = blob_volume((48, 40, 36), seed=5)
    cell = np.array([0.01, 0.01, 0.01], np.float32)
    ref, total, _ = O.marching_cubes(vol, cell, tri, nv)
    # count only
    _, t0 = A.marching_cubes(dev(vol), cell, dev(tri), dev(nv), 0)
    assert int(host(t0)[0]) == total
    # truncated: the first `cap` vertices, nothing written beyond
    cap = total // 3 + 1
    pts = torch.full((cap + 8, 4), -7.0, dtype=torch.float32, device="cuda")
    tot = torch.zeros(1, dtype=torch.int32, device="cuda")
    from dynfu_amd import _lib
    _lib._check(_lib.load().dfa_marching_cubes(_lib._dev(dev(vol)), 48, 40, 36, _lib._farr(cell, 3), _lib._dev(dev(tri)),
                                               _lib._dev(dev(nv)), _lib._dev(pts), cap, _lib._dev(tot), _lib._stream()))
    assert int(host(tot)[0]) == total
    assert np.array_equal(bits(host(pts)[:cap]), bits(ref[:cap])) and np.all(host(pts)[cap:] == -7.0)
    # empty volume, all-outside volume
    zero = np.zeros((8, 8, 8), np.uint32)
    assert int(host(A.marching_cubes(dev(zero), cell, dev(tri), dev(nv), 10)[1])[0]) == 0
    pos = pack(np.full((8, 8, 8), 0.25), np.ones((8, 8, 8), np.uint32))
    assert int(host(A.marching_cubes(dev(pos), cell, dev(tri), dev(nv), 10)[1])[0]) == 0
    with pytest.raises(A.DynfuAmdError):
        A.marching_cubes(dev(vol), cell, None, dev(nv), 10)


@pytest.mark.parametrize("dims,delta", [((64, 64, 64), 0.5), ((50, 38, 44), 0.75), ((128, 128, 128), 0.5)])
def test_vertex_normals_bit_exact(A, dims, delta):
    """dfa_tsdf_vertex_normals vs the oracle's compute_normal on the vertices marching cubes emits,
    plus points whose gradient stencil leaves the volume (NaN on both sides)"""
    tri, nv = default_tables()
    vol = blob_volume(dims, seed=7, holes=False)
    cell = np.array([3.0 / dims[0], 2.5 / dims[1], 3.5 / dims[2]], np.float32)
    pts, total, _ = O.marching_cubes(vol, cell, tri, nv)
    assert total > 100
    extra = np.array([[0, 0, 0, 1], [cell[0] * (dims[0] - 1), 0.5, 0.5, 1], [-1, 0.5, 0.5, 1]], np.float32)
    pts = np.concatenate([pts, extra]).astype(np.float32)
    ref = O.tsdf_vertex_normals(vol, cell, delta, pts)
    got = host(A.tsdf_vertex_normals(dev(vol), cell, delta, dev(pts)))
    assert np.isnan(ref[-3:, 0]).all()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(got)[ok], bits(ref)[ok])
    assert host(A.tsdf_vertex_normals(dev(vol), cell, delta, dev(pts[:0]))).shape == (0, 4)


def _boxes(hv):
    """the map the sweep must at least produce, per box of 32 x 2 x 8 voxels (x, y, z): (holds a voxel with a weight, holds
    a voxel with a weight and a negative distance)"""
    Z, Y, X = hv.shape
    w = (hv >> 16) != 0
    neg = w & ((hv & 0x8000) != 0) & ((hv & 0x7fff) != 0)

    def boxes(b):
        pad = np.zeros(((Z + 7) // 8 * 8, (Y + 1) // 2 * 2, (X + 31) // 32 * 32), bool)
        pad[:Z, :Y, :X] = b
        return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 2, 2, pad.shape[2] // 32, 32).any(axis=(1, 3, 5))

    return boxes(w), boxes(neg)


@pytest.mark.parametrize("name,dims", [("T1", None), ("T0", None), ("T1", (100, 77, 90)), ("C2", None)])
def test_occupancy_map_and_marching_cubes_without_the_empty_voxels(A, name, dims):
    """dfa_tsdf_clear_integrate_occ / dfa_tsdf_integrate_occ / dfa_tsdf_clear_occ keep a byte per box of 32 x 2 x 8 voxels;
    dfa_marching_cubes_occ reads it instead of the empty voxels (the reference's OccupiedVoxels pass reads all of them,
    src/kfusion/cuda/marching_cubes.cu:77-142).  The volume is the one the plain entry points write (bit for bit), the map
    covers every voxel with a weight and is sparse, the mesh is the plain entry point's and the oracle's, bit for bit —
    fused sweep, accumulating sweep over three frames, ragged dimensions, BASELINE size."""
    import torch
    cfg = synth.CONFIGS[name]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    X, Y, Z = dims or (cfg["dim"],) * 3
    if dims:
        voxel = tuple(float(synth.VOLUME_SIZE / d) for d in dims)
    tri, nv = default_tables()
    dists = []
    for f in range(3):
        d = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
        A.compute_dists(dev(synth.depth_frame(cfg, f)), d, fx, fy, cx, cy)
        dists.append(d)
    vol = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda")
    plain = torch.empty_like(vol)
    occ = A.tsdf_occupancy(vol)
    assert tuple(occ.shape) == ((Z + 7) // 8, (Y + 1) // 2, (X + 31) // 32)
    occ.fill_(7)  # the fused sweep must write every byte

    def check(cap=None):
        hv = host(vol).view(np.uint32)
        assert np.array_equal(hv, host(plain).view(np.uint32))
        m, full = (host(occ) & 1) != 0, (host(occ) & 2) != 0
        need, need_neg = _boxes(hv)
        assert not (need & ~m).any() and not (need_neg & ~full).any()  # supersets of the boxes with weights / negative distances
        assert m.sum() < 3 * max(1, need.sum()) and not (full & ~m).any()  # ... and not much more
        # (boxes of 32 x 2 x 8 voxels against the frustum / a band of ~5 voxels around the surface: coarse at 64^3 and
        # 128^3, where most boxes hold something; at 512^3 a third of the volume has weights and a tenth may be negative)
        if X >= 512:
            assert m.mean() < 0.4 and full.mean() < 0.2, (m.mean(), full.mean())
        ref_pts, ref_total = A.marching_cubes(plain, voxel, dev(tri), dev(nv), cap or 1)
        total = int(host(ref_total)[0])
        ref_pts, _ = A.marching_cubes(plain, voxel, dev(tri), dev(nv), total)
        pts, got = A.marching_cubes(vol, voxel, dev(tri), dev(nv), total, occupancy=occ)
        assert int(host(got)[0]) == total > 1000
        assert np.array_equal(bits(host(pts)), bits(host(ref_pts)))
        return hv, total, host(pts)

    A.tsdf_clear_integrate(plain, dists[0], voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)
    A.tsdf_clear_integrate(vol, dists[0], voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, occupancy=occ)
    assert set(np.unique(host(occ))) <= {0, 1, 3}
    hv, total, pts = check()
    if X * Y * Z <= 128 ** 3:  # the CPU statement of marching cubes beside it
        ref, rtotal, _ = O.marching_cubes(hv, np.asarray(voxel, np.float32), tri, nv)
        assert rtotal == total and np.array_equal(bits(pts), bits(ref))
    # the accumulating sweep: two more frames into the same volume; the map only grows
    before = host(occ) != 0
    for f in (1, 2):
        A.tsdf_integrate(plain, dists[f], voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)
        A.tsdf_integrate(vol, dists[f], voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, occupancy=occ)
    assert not (before & ~(host(occ) != 0)).any()
    check()
    # clear: volume and map
    A.tsdf_clear(vol, occupancy=occ)
    assert not host(occ).any() and not host(vol).any()
    pts, got = A.marching_cubes(vol, voxel, dev(tri), dev(nv), 16, occupancy=occ)
    assert int(host(got)[0]) == 0
    # a map of ones is the plain sweep
    A.tsdf_clear_integrate(vol, dists[1], voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)
    A.tsdf_clear_integrate(plain, dists[1], voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)
    occ.fill_(3)
    _, t1 = A.marching_cubes(vol, voxel, dev(tri), dev(nv), 1, occupancy=occ)
    _, t0 = A.marching_cubes(plain, voxel, dev(tri), dev(nv), 1)
    assert int(host(t1)[0]) == int(host(t0)[0]) > 1000


@pytest.mark.parametrize("name,dims", [("T1", None), ("T1", (100, 77, 90)), ("C2", None), ("C4", None)])
def test_fused_sweep_over_a_known_occupancy_map_leaves_the_same_volume_and_map(A, name, dims):
    """dfa_tsdf_clear_integrate_known_occ: with a map that describes the volume on entry, boxes of zeros that stay zeros are
    not stored again.  Frame after frame with a moving camera — behind a clear, behind fused sweeps, behind accumulating
    sweeps — the volume and the map are those of dfa_tsdf_clear_integrate_occ (and so of the plain fused sweep, and at the
    small sizes of the oracle), bit for bit; the documented failure with a map that does NOT describe the volume is there
    too (old content survives where the map says "zeros")."""
    import torch
    cfg = synth.CONFIGS[name]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    X, Y, Z = dims or (cfg["dim"],) * 3
    if dims:
        voxel = tuple(float(synth.VOLUME_SIZE / d) for d in dims)
    dists = []
    for f in range(4):
        d = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
        A.compute_dists(dev(synth.depth_frame(cfg, f)), d, fx, fy, cx, cy)
        dists.append(d)

    def pose(f):  # the camera a little to the side and back every frame: other boxes come into the frustum
        m = np.array(vol2cam, np.float32).copy()
        m[9] += 0.04 * f
        m[11] += 0.03 * f
        return m

    vol = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda").random_(0, 2 ** 31 - 1)
    ref = torch.empty_like(vol)
    occ, occ_ref = A.tsdf_occupancy(vol), A.tsdf_occupancy(vol)
    args = (voxel, trunc, synth.MAX_WEIGHT)

    def same():  # (on the device: 1024^3 is 4 GiB a volume)
        assert torch.equal(vol, ref) and torch.equal(occ, occ_ref)

    A.tsdf_clear(vol, occupancy=occ)  # from here on the map describes the volume
    occ_first = None
    for f in range(4):
        A.tsdf_clear_integrate(vol, dists[f], *args, pose(f), fx, fy, cx, cy, occupancy=occ, occupancy_known=True)
        A.tsdf_clear_integrate(ref, dists[f], *args, pose(f), fx, fy, cx, cy, occupancy=occ_ref)
        same()
        if f == 0:
            occ_first = occ.clone()
    if X >= 1024:
        # The one place where "old content survives" would show, against the ORACLE (the comparison above is with the plain
        # HIP sweep): the 32 slices with the most boxes that frame 0 wrote and frame 3 — the camera has moved — left alone
        # because their byte said zeros... which they are only if frames 1-3 put the zeros back when the boxes fell out of
        # the frustum.  orc_tsdf_integrate_slab (tsdf_volume.cu:11-22 clear + :43-96) on zeros = what a cleared volume
        # holds after frame 3.
        gone = ((occ_first != 0) & (occ == 0)).sum(dim=(1, 2))  # per layer of 8 slices
        kept = (occ != 0).sum(dim=(1, 2))
        win = gone.unfold(0, 4, 1).sum(1)                        # per window of four layers
        win_kept = kept.unfold(0, 4, 1).sum(1)
        win = torch.where(win_kept > 1000, win, torch.zeros_like(win))  # (a window frame 3 also writes in: not an empty slab)
        assert int(win.max()) > 1000, int(win.max())             # (thousands of boxes left the frustum)
        z0 = 8 * int(win.argmax())
        slab = np.zeros((32, Y, X), np.uint32)
        O.tsdf_integrate_slab(slab, z0, host(dists[3]), np.asarray(voxel, np.float32), trunc, synth.MAX_WEIGHT, pose(3), fx, fy, cx, cy,
                              threads=8)
        assert np.array_equal(host(vol[z0:z0 + 32]).view(np.uint32), slab), z0
        assert (slab >> 16 != 0).any()  # (not an empty slab: part of it is inside the frustum of frame 3)
    skipped = float((occ == 0).float().mean())
    if X >= 512:
        assert skipped > 0.6  # most of the volume is not written at all
    if X * Y * Z <= 128 ** 3:
        dn = host(dists[3])
        want = np.zeros((Z, Y, X), np.uint32)
        O.tsdf_integrate(want, dn, np.asarray(voxel, np.float32), trunc, synth.MAX_WEIGHT, pose(3), fx, fy, cx, cy)
        assert np.array_equal(host(vol).view(np.uint32), want)
    # behind accumulating sweeps (the map only grows there) ...
    for f in (1, 2):
        A.tsdf_integrate(vol, dists[f], *args, pose(f), fx, fy, cx, cy, occupancy=occ)
        A.tsdf_integrate(ref, dists[f], *args, pose(f), fx, fy, cx, cy, occupancy=occ_ref)
    A.tsdf_clear_integrate(vol, dists[0], *args, pose(0), fx, fy, cx, cy, occupancy=occ, occupancy_known=True)
    A.tsdf_clear_integrate(ref, dists[0], *args, pose(0), fx, fy, cx, cy, occupancy=occ_ref)
    same()
    # ... and what the contract warns of: a map of zeros over a volume that is not
    vol.fill_(0x00070001)  # (weight 7: nothing one frame writes)
    occ.zero_()
    A.tsdf_clear_integrate(vol, dists[0], *args, pose(0), fx, fy, cx, cy, occupancy=occ, occupancy_known=True)
    left = vol == 0x00070001
    assert bool(left.any()) and not bool((left & (ref != 0)).any())  # only where the frame writes zeros
    A.tsdf_clear_integrate(vol, dists[0], *args, pose(0), fx, fy, cx, cy, occupancy=occ)  # the sweep without the promise repairs it
    same()


# ------------------------------------------------------------------------------------------------------------------------
# Against tests/mc_statement.py: the numpy statement of the reference's marching cubes (not the oracle's C, which shares
# the kernels' author and operation order), and its table-free fp64 checker.  Inputs that reach what the kernels are
# sized for (tests/test_mc_statement_cpu.py asserts that they do), and the sizes the benchmark runs.
import mc_statement as MS  # noqa: E402
from mc_util import checkerboard_volume, sign_noise_volume, special_values_volume  # noqa: E402

NOISE_DIMS = (512, 24, 24)   # vec4 path, two 256-cube segments per row, two z chunks
RAGGED_DIMS = (130, 11, 9)   # X % 4 != 0: the scalar path, three 64-cube segments per row


def _cell(dims):
    return np.array([3.0 / dims[0], 2.5 / dims[1], 3.5 / dims[2]], np.float32)


def _new_volume(kind, dims):
    return {"noise": lambda: sign_noise_volume(dims, 0), "checkerboard": lambda: checkerboard_volume(dims),
            "special": lambda: special_values_volume(dims, 0)}[kind]()


def _same_bits(got, ref):
    """NaN positions first, then the bits elsewhere (as test_vertex_normals_bit_exact does)"""
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(got)[ok], bits(ref)[ok])


@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("dims", [NOISE_DIMS, RAGGED_DIMS])
@pytest.mark.parametrize("kind", ["noise", "checkerboard", "special"])
def test_dense_ambiguous_and_special_volumes_equal_the_statement(A, kind, dims, which):
    """all 254 cases, 20 triangles in a lane's four cubes, segments of 2 600 and 3 072 vertices; fp16 denormals, +-0,
    +-65504, +-inf and NaN as distances (the statement defines the bits: NaN < 0 is false, inf gives t = 0 or NaN)"""
    tri, nv = _tables(which)
    vol, cell = _new_volume(kind, dims), _cell(dims)
    ref, total = MS.marching_cubes(vol, cell, tri, nv)
    got, gtotal = _run(A, vol, cell, tri, nv, max(total, 1))
    assert gtotal == total > 100
    _same_bits(got, ref)
    if kind == "noise":  # the geometry itself, with no table and no order: the kernel's output
        MS.check_voxel_order(MS.check_mesh_fp64(got, vol, cell), dims)


def test_volume_pointer_that_is_not_16_byte_aligned(A):
    """X % 4 == 0 but the volume starts 4 bytes into a buffer: the scalar path, chosen by the pointer"""
    import torch
    tri, nv = reference_data.mc_tables()
    dims = NOISE_DIMS
    vol, cell = sign_noise_volume(dims, 1), _cell(dims)
    buf = torch.zeros(vol.size + 1, dtype=torch.int32, device="cuda")
    buf[1:] = dev(vol).reshape(-1)
    view = buf[1:].view(vol.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ref, total = MS.marching_cubes(vol, cell, tri, nv)
    pts, gtotal = A.marching_cubes(view, cell, dev(tri), dev(nv), total)
    assert int(host(gtotal)[0]) == total
    assert np.array_equal(bits(host(pts)), bits(ref))


def test_segment_count_that_is_an_exact_multiple_of_the_scan_chunk(A):
    """(256, 64, 128): one segment per row, 64 * 128 = 8 192 segments = exactly one scan chunk — the total is written by
    the thread whose last entry is the array's last (`first + PER == n`)"""
    tri, nv = default_tables()
    for dims in [(256, 64, 128), (256, 128, 128)]:
        assert (dims[1] * dims[2]) % 8192 == 0
        vol, cell = blob_volume(dims, seed=3), _cell(dims)
        ref, total = MS.marching_cubes(vol, cell, tri, nv)
        got, gtotal = _run(A, vol, cell, tri, nv, total)
        assert gtotal == total > 10000
        assert np.array_equal(bits(got), bits(ref))


def test_capacity_that_ends_inside_a_heavy_segment(A):
    """the first `cap` vertices and nothing beyond, where cap falls in the middle of the noise volume's fullest 256-cube
    segment"""
    import torch
    from dynfu_amd import _lib
    tri, nv = reference_data.mc_tables()
    dims = NOISE_DIMS
    X, Y, Z = dims
    vol, cell = sign_noise_volume(dims, 0), _cell(dims)
    ref, total = MS.marching_cubes(vol, cell, tri, nv)
    n = MS.cube_counts(vol, nv)
    pad = np.zeros(n.shape[:2] + (512,), np.int64)
    pad[:, :, :X - 1] = n
    segs = pad.reshape(Z - 1, Y - 1, 2, 256).sum(-1)  # the vec4 path's segments, in output order
    flat = segs.reshape(-1)
    s = int(flat.argmax())
    assert flat[s] >= 2000
    cap = int(flat[:s].sum() + flat[s] // 2 + 1)
    pts = torch.full((cap + 64, 4), -7.0, dtype=torch.float32, device="cuda")
    tot = torch.zeros(1, dtype=torch.int32, device="cuda")
    dvol, dtri, dnv = dev(vol), dev(tri), dev(nv)  # (held until the call has run: a temporary's memory may be handed out again)
    _lib._check(_lib.load().dfa_marching_cubes(_lib._dev(dvol), X, Y, Z, _lib._farr(cell, 3), _lib._dev(dtri), _lib._dev(dnv),
                                               _lib._dev(pts), cap, _lib._dev(tot), _lib._stream()))
    assert int(host(tot)[0]) == total
    assert np.array_equal(bits(host(pts)[:cap]), bits(ref[:cap]))
    assert np.all(host(pts)[cap:] == -7.0)


def _integrated_volume(A, name):
    import torch
    cfg = synth.CONFIGS[name]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    dim = cfg["dim"]
    d = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
    A.compute_dists(dev(synth.depth_frame(cfg, 0)), d, fx, fy, cx, cy)
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    occ = A.tsdf_occupancy(vol)
    A.tsdf_clear_integrate(vol, d, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, occupancy=occ)
    return vol, occ, np.asarray(voxel, np.float32)


def test_c2_size_equals_the_statement_slab_by_slab(A):
    """512^3 (benchmark config C2: two segments per row, 64 scan chunks, z chunks of 32 slices): a synthetic depth frame
    integrated, extracted by the plain entry point and with the occupancy map — total and bits against the statement run
    slab by slab over the whole volume, and the geometry against the fp64 checker"""
    tri, nv = default_tables()
    vol, occ, cell = _integrated_volume(A, "C2")
    _, t = A.marching_cubes(vol, cell, dev(tri), dev(nv), 1)
    total = int(host(t)[0])
    assert total > 100000
    pts, t0 = A.marching_cubes(vol, cell, dev(tri), dev(nv), total)
    pts_occ, t1 = A.marching_cubes(vol, cell, dev(tri), dev(nv), total, occupancy=occ)
    assert int(host(t0)[0]) == int(host(t1)[0]) == total
    got, got_occ = host(pts), host(pts_occ)
    hv = host(vol).view(np.uint32)
    Z, slab, off = hv.shape[0], 16, 0
    for z in range(0, Z - 1, slab):
        c = MS.count(hv, nv, z, z + slab)
        if c:
            ref = MS.vertices(hv, cell, tri, nv, z, z + slab)
            assert len(ref) == c
            assert np.array_equal(bits(got[off:off + c]), bits(ref)), z
            assert np.array_equal(bits(got_occ[off:off + c]), bits(ref)), z
        off += c
    assert off == total
    MS.check_voxel_order(MS.check_mesh_fp64(got, hv, cell), hv.shape[::-1])


def test_c4_size_count_of_every_slab_and_the_fullest_slabs_in_full(A):
    """1024^3 (benchmark config C4: four segments per row, 512 scan chunks, z chunks of 256 slices).  The statement's
    count-only pass runs over ALL 64 slabs of 16 slices, fetched from the device a slab at a time: it gives the total and
    every slab's offset in the output.  The vertices are compared in full on the first non-empty slab, the last non-empty
    one and the fullest one, plus the next fullest until the compared slabs hold at least 10 % of all vertices."""
    tri, nv = default_tables()
    vol, occ, cell = _integrated_volume(A, "C4")
    _, t = A.marching_cubes(vol, cell, dev(tri), dev(nv), 1)
    total = int(host(t)[0])
    assert total > 400000
    pts, t0 = A.marching_cubes(vol, cell, dev(tri), dev(nv), total, occupancy=occ)
    assert int(host(t0)[0]) == total
    del occ
    Z, slab = vol.shape[0], 16
    starts = list(range(0, Z - 1, slab))
    fetch = lambda z: host(vol[z:min(z + slab, Z - 1) + 1]).view(np.uint32)
    counts = np.array([MS.count(fetch(z), nv, z, z + slab, z_base=z, Z=Z) for z in starts])
    assert counts.sum() == total  # the counted total is the kernel's
    offs = np.cumsum(counts) - counts
    nonempty = np.flatnonzero(counts)
    by_size = np.argsort(-counts, kind="stable")
    chosen = [int(nonempty[0]), int(nonempty[-1]), int(by_size[0])]
    for s in by_size[1:]:
        if counts[sorted(set(chosen))].sum() >= 0.1 * total:
            break
        chosen.append(int(s))
    chosen = sorted(set(chosen))
    assert counts[chosen].sum() >= 0.1 * total
    print("1024^3: %d vertices, %d of %d slabs non-empty, %d slabs compared in full (%d vertices, %.1f %%)"
          % (total, len(nonempty), len(starts), len(chosen), counts[chosen].sum(), 100.0 * counts[chosen].sum() / total))
    for s in chosen:
        z = starts[s]
        ref = MS.vertices(fetch(z), cell, tri, nv, z, z + slab, z_base=z, Z=Z)
        got = host(pts[int(offs[s]):int(offs[s] + counts[s])])
        assert len(ref) == counts[s] and np.array_equal(bits(got), bits(ref)), z
    # the plain entry point's output is the same array (on the device)
    import torch
    del ref, got
    plain, t1 = A.marching_cubes(vol, cell, dev(tri), dev(nv), total)
    assert int(host(t1)[0]) == total and torch.equal(plain, pts)
