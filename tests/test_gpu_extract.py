"""-m gpu parity tests of the point-cloud extraction (dfa_tsdf_extract_cloud / _occ / dfa_tsdf_extract_normals):
HIP kernels through the C ABI against the numpy statement of tests/extract_statement.py (the reference's FullScan6 and
ExtractNormals, src/kfusion/cuda/tsdf_volume.cu:423-680, with the output contract of include/dynfu_amd.h).

Bar: BIT-EXACT — point count, order (ascending voxel index, then +x +y +z) and the float bits of every point and normal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import extract_statement as S  # noqa: E402
import oracle as O  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import aff12, bits, dev, host, rot  # noqa: E402

ID12 = aff12(np.eye(3), [0, 0, 0])
POSED = aff12(rot([0.3, -0.8, 0.5], 0.7), [-1.25, 0.75, 0.5])


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def random_volume(dims, seed, p_neg=0.05):
    """packed (Z, Y, X) volume: random fp16 distances (exact +-1 and +-0 included), a share of zero weights"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    F = rng.uniform(0.0, 1.0, (Z, Y, X)).astype(np.float32)
    F = np.where(rng.random((Z, Y, X)) < p_neg, -F, F)
    special = rng.random((Z, Y, X))
    F = np.where(special < 0.03, np.float32(1), F)
    F = np.where((special >= 0.03) & (special < 0.05), np.float32(-1), F)
    F = np.where((special >= 0.05) & (special < 0.06), np.float32(0), F)
    F = np.where((special >= 0.06) & (special < 0.07), np.float32(-0.0), F)
    W = np.where(rng.random((Z, Y, X)) < 0.1, 0, rng.integers(1, 65536, (Z, Y, X))).astype(np.uint32)
    return S.pack(F, W)


def extract(A, vol, voxel, aff, cap=None, occupancy=None):
    if cap is None:
        _, total = A.tsdf_extract_cloud(vol, voxel, aff, 0, occupancy=occupancy)
        cap = max(int(host(total)[0]), 1)
    pts, total = A.tsdf_extract_cloud(vol, voxel, aff, cap, occupancy=occupancy)
    total = int(host(total)[0])
    return host(pts)[: min(total, cap)], total


def assert_cloud_matches_statement(hv, voxel, aff, got, slab=None):
    """got: the kernel's points; the statement's slab by slab (a 512^3 volume at once would take gigabytes)"""
    Z = hv.shape[0]
    slab = slab or Z
    at = 0
    for z in range(0, Z, slab):
        want = S.extract_cloud(hv, voxel, aff, z, z + slab)
        assert np.array_equal(bits(got[at:at + len(want)]), bits(want)), "slab %d" % z
        at += len(want)
    assert at == len(got)


@pytest.mark.parametrize("dims,p_neg", [((37, 29, 23), 0.05), ((65, 2, 9), 0.3), ((4, 3, 2), 0.5), ((1, 1, 1), 0.5),
                                        ((128, 128, 128), 0.5), ((256, 256, 256), 0.05), ((260, 9, 7), 0.5)])
@pytest.mark.parametrize("pose", ["identity", "posed"])
def test_extract_cloud_random_volumes_bit_exact(A, dims, p_neg, pose):
    hv = random_volume(dims, seed=sum(dims), p_neg=p_neg)
    voxel = np.array([3.0 / dims[0], 2.5 / dims[1], 3.5 / dims[2]], np.float32)
    aff = ID12 if pose == "identity" else POSED
    got, total = extract(A, dev(hv), voxel, aff)
    assert total == len(got)
    if dims[2] > 1 and p_neg == 0.5:
        assert total > 0
    assert_cloud_matches_statement(hv, voxel, aff, got, slab=32)


def test_extract_cloud_every_edge_crossing_and_unaligned_volume(A):
    """a checkerboard of signs: 3 points per voxel, 768 per 256-voxel row segment (three LDS windows of the emit); the
    same volume at an address that is not 16-byte aligned (the one-voxel-per-lane form)"""
    import torch
    X, Y, Z = 256, 6, 5
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    F = np.where((x + y + z) % 2 == 0, np.float32(0.25), np.float32(-0.5))
    hv = S.pack(F, np.ones_like(F, np.uint32))
    voxel = np.full(3, 0.01, np.float32)
    got, total = extract(A, dev(hv), voxel, POSED)
    assert total == (Z - 1) * ((X - 1) * Y + X * (Y - 1) + X * Y)  # every source voxel, every edge it has
    assert_cloud_matches_statement(hv, voxel, POSED, got)
    flat = torch.from_numpy(hv.view(np.int32).reshape(-1)).cuda()
    big = torch.empty(flat.numel() + 1, dtype=torch.int32, device="cuda")
    big[1:] = flat
    unaligned = big[1:].view(Z, Y, X)
    assert unaligned.data_ptr() % 16 != 0
    got2, total2 = extract(A, unaligned, voxel, POSED)
    assert total2 == total and np.array_equal(bits(got2), bits(got))


def _fused_volume(A, name, frames=(0,), cam_shift=None, occupancy=False):
    import torch
    cfg = synth.CONFIGS[name]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    dim = cfg["dim"]
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    occ = A.tsdf_occupancy(vol) if occupancy else None
    for i, f in enumerate(frames):
        d = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
        A.compute_dists(dev(synth.depth_frame(cfg, f)), d, fx, fy, cx, cy)
        v2c = vol2cam.copy()
        if cam_shift is not None:  # the camera moved: vol2cam = pose translated by -shift
            v2c[9:] -= np.float32(i) * np.asarray(cam_shift, np.float32)
        if i == 0:
            A.tsdf_clear_integrate(vol, d, voxel, trunc, synth.MAX_WEIGHT, v2c, fx, fy, cx, cy, occupancy=occ)
        else:
            A.tsdf_integrate(vol, d, voxel, trunc, synth.MAX_WEIGHT, v2c, fx, fy, cx, cy, occupancy=occ)
    return vol, occ, voxel, vol2cam


@pytest.mark.parametrize("name,pose", [("T0", "identity"), ("T0", "posed"), ("T1", "volume"), ("C2", "posed")])
def test_extract_cloud_of_fused_frames_bit_exact(A, name, pose):
    vol, _, voxel, vol2cam = _fused_volume(A, name)
    aff = {"identity": ID12, "posed": POSED, "volume": vol2cam}[pose]
    got, total = extract(A, vol, voxel, aff)
    assert total > 1000
    assert_cloud_matches_statement(host(vol).view(np.uint32), voxel, aff, got, slab=32)
    if pose == "volume":  # the cloud is the depth surface, in the camera (= world) frame
        p = got[:, :3].astype(np.float64)
        on_sphere = np.abs(np.linalg.norm(p - synth.SPHERE_C, axis=1) - synth.SPHERE_R) < 0.03
        on_plane = np.abs(p[:, 2] - synth.PLANE_Z) < 0.03
        assert (on_sphere | on_plane).mean() > 0.97


def test_extract_cloud_contract(A):
    """total; a capacity below it writes exactly the first points and nothing after them; count-only; the same bits every
    call; two volumes extracted on two streams at once each get their own answer"""
    import torch
    dims = (96, 40, 33)
    hv = random_volume(dims, seed=11, p_neg=0.2)
    voxel = np.full(3, 0.02, np.float32)
    vol = dev(hv)
    want = S.extract_cloud(hv, voxel, POSED)
    n = len(want)
    assert n > 10000
    _, total = A.tsdf_extract_cloud(vol, voxel, POSED, 0)  # count only
    assert int(host(total)[0]) == n
    for cap in (1, 63, 64, 1000, n - 1, n, n + 100):
        pts = torch.full((cap + 64, 4), -7.0, dtype=torch.float32, device="cuda")  # sentinels after the capacity
        tot = torch.zeros((1,), dtype=torch.int32, device="cuda")
        L = A._lib
        A._lib._check(L.load().dfa_tsdf_extract_cloud(L._dev(vol), dims[0], dims[1], dims[2], L._farr(voxel, 3),
                                                      L._aff12(POSED), L._dev(pts), cap, L._dev(tot), L._stream()))
        h = host(pts)
        assert int(host(tot)[0]) == n
        k = min(cap, n)
        assert np.array_equal(bits(h[:k]), bits(want[:k]))
        assert (h[k:] == -7.0).all(), cap
    a, _ = extract(A, vol, voxel, POSED, cap=n)
    b, _ = extract(A, vol, voxel, POSED, cap=n)
    assert np.array_equal(bits(a), bits(b))
    # two streams
    hv2 = random_volume((128, 64, 48), seed=12, p_neg=0.3)
    vol2 = dev(hv2)
    want2 = S.extract_cloud(hv2, voxel, ID12)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            r1 = A.tsdf_extract_cloud(vol, voxel, POSED, n + 5)
        with torch.cuda.stream(s2):
            r2 = A.tsdf_extract_cloud(vol2, voxel, ID12, len(want2) + 5)
        outs.append((r1, r2))
    torch.cuda.synchronize()
    for (p1, t1), (p2, t2) in outs:
        assert int(host(t1)[0]) == n and int(host(t2)[0]) == len(want2)
        assert np.array_equal(bits(host(p1)[:n]), bits(want)) and np.array_equal(bits(host(p2)[:len(want2)]), bits(want2))


def _exact_map(hv):
    """the tightest map the contract allows: bit 0 where a box holds a weight, bit 1 where it holds a negative distance"""
    Z, Y, X = hv.shape
    F, W = S.unpack(hv)

    def boxes(b):
        pad = np.zeros(((Z + 7) // 8 * 8, (Y + 1) // 2 * 2, (X + 31) // 32 * 32), bool)
        pad[:Z, :Y, :X] = b
        return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 2, 2, pad.shape[2] // 32, 32).any(axis=(1, 3, 5))

    return (boxes(W != 0).astype(np.uint8) | (boxes(F < 0).astype(np.uint8) << 1)).astype(np.uint8)


def test_extract_cloud_occ_with_the_tightest_map(A):
    """crossings between boxes: the negative voxel in the +x / +y / +z neighbour box of a source whose own box has no
    negative distance — the conservative rule reads the source box for its neighbours' bit 1"""
    dims = (96, 20, 40)
    X, Y, Z = dims
    F = np.full((Z, Y, X), 0.5, np.float32)
    W = np.zeros((Z, Y, X), np.uint32)
    for (x, y, z) in [(31, 5, 4), (40, 1, 9), (50, 10, 7), (63, 19, 23), (64, 3, 31)]:
        W[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = 1
    W[:, :, 95] = 0
    for (x, y, z) in [(32, 5, 4), (40, 2, 9), (50, 10, 8), (64, 19, 24), (65, 3, 32)]:  # across a box face
        F[z, y, x], W[z, y, x] = -0.5, 1
    hv = S.pack(F, W)
    voxel = np.full(3, 0.01, np.float32)
    want = S.extract_cloud(hv, voxel, POSED)
    occ = _exact_map(hv)
    got, total = extract(A, dev(hv), voxel, POSED, occupancy=dev(occ))
    assert total == len(want) > 20
    assert np.array_equal(bits(got), bits(want))
    # random volumes under their tightest maps
    for seed, d in ((21, (37, 29, 23)), (22, (128, 64, 40)), (23, (260, 9, 17))):
        hv = random_volume(d, seed, p_neg=0.01)
        hv[:, :, : d[0] // 2] = 0  # empty boxes that the map lets the sweep skip
        want = S.extract_cloud(hv, voxel, ID12)
        got, total = extract(A, dev(hv), voxel, ID12, occupancy=dev(_exact_map(hv)))
        assert total == len(want) and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_extract_cloud_occ_equals_plain_on_fused_volumes(A, name):
    """maps left by the fused sweep, then by the accumulating sweep over more frames from a moving camera"""
    vol, occ, voxel, vol2cam = _fused_volume(A, name, occupancy=True)
    for step in range(2):
        plain, total = extract(A, vol, voxel, POSED)
        got, gtotal = extract(A, vol, voxel, POSED, cap=total, occupancy=occ)
        assert gtotal == total > 10000
        assert np.array_equal(bits(got), bits(plain))
        if step == 0:
            del vol, occ
            vol, occ, voxel, vol2cam = _fused_volume(A, name, frames=(0, 3, 6), cam_shift=(0.03, -0.02, 0.05),
                                                     occupancy=True)


def assert_same_normals(got, want):
    """NaN exactly where the statement has NaN (whatever its payload), the same bits everywhere else"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(np.where(nan, 0, got)), bits(np.where(nan, 0, want)))


def _posed_cloud(A, name, aff):
    vol, _, voxel, vol2cam = _fused_volume(A, name)
    pts, _ = extract(A, vol, voxel, aff)
    return vol, voxel, pts


@pytest.mark.parametrize("pose", ["identity", "posed"])
def test_extract_normals_of_the_fetched_cloud_bit_exact(A, pose):
    import torch
    aff = ID12 if pose == "identity" else POSED
    rinv = np.linalg.inv(aff[:9].reshape(3, 3).astype(np.float64)).astype(np.float32)
    vol, voxel, pts = _posed_cloud(A, "T1", aff)
    hv = host(vol).view(np.uint32)
    got = host(A.tsdf_extract_normals(vol, voxel, aff, synth.GRADIENT_DELTA_FACTOR, torch.from_numpy(pts).cuda(), Rinv=rinv))
    want = S.extract_normals(hv, voxel, aff, rinv, synth.GRADIENT_DELTA_FACTOR, pts)
    assert_same_normals(got, want)
    assert np.isfinite(got[:, 0]).mean() > 0.9
    if pose == "identity":  # R = I: R n = n, so in range the raycaster's normal (the CPU oracle of vertex normals)
        ok = np.isfinite(want[:, 0])
        ref = O.tsdf_vertex_normals(hv, voxel, synth.GRADIENT_DELTA_FACTOR, pts)
        assert np.array_equal(bits(got[ok]), bits(np.asarray(ref, np.float32).reshape(-1, 4)[ok]))


def test_extract_normals_hand_placed_points(A):
    """points out of range, exactly on the voxels g = 1, 2, dim - 3 and dim - 2 of every axis, round-half-even ties
    between them, and NaN / huge coordinates"""
    import torch
    dims = (40, 36, 44)
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    F = np.clip(((x - 20.3) * 0.6 + (y - 17.1) * 0.3 - (z - 21.7) * 0.5) * 0.05, -1, 1).astype(np.float32)
    hv = S.pack(F, np.ones_like(F, np.uint32))
    voxel = np.array([0.02, 0.025, 0.015], np.float32)
    coords = []
    for axis, dim in enumerate(dims):
        for g in (-3.0, 0.0, 1.0, 1.5, 2.0, 2.5, 3.5, dim - 3.5, dim - 3.0, dim - 2.5, dim - 2.0, dim - 1.5, dim - 1.0, dim + 4.0):
            c = [X / 2 + 0.3, Y / 2 - 0.2, Z / 2 + 0.1]
            c[axis] = g
            coords.append(c)
    coords += [[np.nan, 5, 5], [1e30, 5, 5], [-1e30, 5, 5], [np.inf, 5, 5]]
    vox = np.array(coords, np.float32)
    for aff in (ID12, POSED):
        R, t = aff[:9].reshape(3, 3), aff[9:]
        rinv = np.linalg.inv(R.astype(np.float64)).astype(np.float32)
        world = (vox * voxel) @ R.T + t
        pts = np.concatenate([world, np.zeros((len(world), 1))], 1).astype(np.float32)
        got = host(A.tsdf_extract_normals(dev(hv), voxel, aff, 0.5, torch.from_numpy(pts).cuda(), Rinv=rinv))
        want = S.extract_normals(hv, voxel, aff, rinv, 0.5, pts)
        assert_same_normals(got, want)
        assert 10 < np.isfinite(want[:, 0]).sum() < len(want) - 10


def test_extract_errors_are_loud(A):
    import torch
    vol = torch.zeros((4, 4, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(A.DynfuAmdError):
        A.tsdf_extract_cloud(vol, [0.1] * 3, ID12, -1)
    with pytest.raises(A.DynfuAmdError):
        A.tsdf_extract_normals(vol, [0.1] * 3, ID12, 0.0, torch.zeros((4, 4), device="cuda"))
    pts, total = A.tsdf_extract_cloud(vol, [0.1] * 3, ID12, 8)  # an empty volume: no points
    assert int(host(total)[0]) == 0
