"""-m gpu: the internal scratch of the C ABI (csrc/device_memory.hpp) across growth.  Every entry point that keeps a
grow-only buffer per (device, stream) is called small -> larger -> the same small again on ONE stream, and each of the
three results is compared, bit for bit, with the same call on a stream that has never been used (whose scratch is
allocated at exactly that call's size).  A buffer that kept a stale capacity, a stale pointer inside a view, or a block
shorter than its policy says shows as a difference (or as a fault) in the second or third call.

All outputs compared here have a defined order and were reproducible where the test was written: no entry point needed
a weaker statement than equality."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import render_scenes as RS  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import aff12, dev, host  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


_HIP = []
_STREAMS = []


def _fresh_stream():
    """a stream straight from the runtime (torch.cuda.Stream() hands out a pool of 32 that other tests have used)"""
    import torch
    if not _HIP:
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _HIP.append(ctypes.CDLL(path))
    h = ctypes.c_void_p()
    assert _HIP[0].hipStreamCreateWithFlags(ctypes.byref(h), 1) == 0 and h.value  # 1 = hipStreamNonBlocking
    _STREAMS.append(h)
    return torch.cuda.ExternalStream(h.value)


@pytest.fixture(scope="module", autouse=True)
def _destroy_streams():
    yield
    import torch
    torch.cuda.synchronize()
    for h in _STREAMS:
        _HIP[0].hipStreamDestroy(h)
    del _STREAMS[:]


def _run(stream, call, args):
    import torch
    with torch.cuda.stream(stream):
        return [a.copy() for a in call(*args)]


def _grown_equals_fresh(call, small, large):
    """call(*args) -> list of numpy arrays (the defined part of the output only)"""
    import torch
    torch.cuda.synchronize()  # the inputs were made on the default stream
    one = _fresh_stream()
    got = [_run(one, call, a) for a in (small, large, small)]
    want = [_run(_fresh_stream(), call, a) for a in (small, large, small)]
    for step, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) > 0
        for x, y in zip(g, w):
            assert x.dtype == y.dtype and x.shape == y.shape and x.size > 0, step
            assert x.tobytes() == y.tobytes(), step
    assert any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(got[0], got[1])), "small and large are one case"
    return got


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    return dev(rng.uniform(-1, 1, (n, 3)).astype(np.float32))


def test_knn_node_grid(A):
    q = _cloud(4096, 1)

    def args(D):  # (want_grid: every node set of 1 024 or more is searched through the grid)
        return _cloud(D, D), dev(np.full(D, 0.1, np.float32)), q, 4

    def call(*a):
        idx, w = A.knn(*a)
        return [host(idx), host(w)]

    _grown_equals_fresh(call, args(1024), args(2048))


@pytest.mark.parametrize("small,large", [(4096, 12000), (16384, 40000)], ids=["node_grid", "point_grid"])
def test_correspond(A, small, large):
    live = _cloud(3000, 2)

    def args(n):
        return _cloud(n, n), _cloud(n, n + 1), live

    def call(*a):
        return [host(t) for t in A.correspond(*a)]

    _grown_equals_fresh(call, args(small), args(large))


@pytest.fixture(scope="module")
def spheres(A):
    """dim -> (volume, voxel size): the fused sphere of tests/render_scenes.py at 32^3 and 64^3"""
    import torch
    cfg = synth.CONFIGS["T0"]
    intr = synth.intrinsics(cfg)
    depth = dev(synth.depth_frame(cfg, 0))
    dists = torch.empty_like(depth)
    A.compute_dists(depth, dists, *intr)
    out = {}
    for dim in (32, 64):
        voxel, trunc, _, _, _ = synth.volume_params(dict(cfg, dim=dim))
        vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
        A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, RS.integration_poses("turned")[0], *intr)
        out[dim] = (vol, voxel)
    return out


@pytest.fixture(scope="module")
def tables(A):
    tri, nv = A.mc_default_tables()
    return dev(tri), dev(nv)


CAP = 1 << 18  # points of one extraction: far above what a 64^3 sphere yields (asserted)


def test_marching_cubes(A, spheres, tables):
    def call(vol, voxel):
        pts, total = A.marching_cubes(vol, voxel, *tables, CAP)
        n = int(host(total)[0])
        assert 0 < n <= CAP
        return [host(total), host(pts)[:n]]

    _grown_equals_fresh(call, spheres[32], spheres[64])


def test_marching_cubes_indexed(A, spheres, tables):
    def call(vol, voxel):
        verts, idx, totals = A.marching_cubes_indexed(vol, voxel, *tables, CAP, CAP)
        nv, ni = (int(v) for v in host(totals))
        assert 0 < nv <= CAP and 0 < ni <= CAP
        return [host(totals), host(verts)[:nv], host(idx)[:ni]]

    _grown_equals_fresh(call, spheres[32], spheres[64])


def test_tsdf_extract_cloud(A, spheres):
    pose = aff12(np.eye(3), synth.VOLUME_POSE_T)

    def call(vol, voxel):
        pts, total = A.tsdf_extract_cloud(vol, voxel, pose, CAP)
        n = int(host(total)[0])
        assert 0 < n <= CAP
        return [host(total), host(pts)[:n]]

    _grown_equals_fresh(call, spheres[32], spheres[64])


def _warp_nodes(D):
    """D nodes on the sphere of the `spheres` volumes (volume frame, metres) with small general transforms"""
    import warp_statement as WS
    rng = np.random.default_rng(D)
    n = rng.standard_normal((D, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    pos = synth.SPHERE_C - np.array(synth.VOLUME_POSE_T) + synth.SPHERE_R * n
    dq = WS.dq_from_euler(*rng.uniform(-0.1, 0.1, (3, D)), *rng.uniform(-0.03, 0.03, (3, D))).reshape(D, 8)
    return tuple(dev(a.astype(np.float32)) for a in (pos, dq, rng.uniform(0.2, 0.5, D)))


@pytest.fixture(scope="module")
def warped(A, spheres):
    """(call, args): the next 64 x 48 depth frame fused into a copy of the dim^3 sphere through D nodes, k = 4, with a fresh
    occupancy map -> the volume words and the map; six = dfa_tsdf_integrate_warped6 with an identity vol2node"""
    import torch
    cfg = _image_cfg(64, 48)
    intr = synth.intrinsics(cfg)
    dists = torch.empty((48, 64), dtype=torch.uint16, device="cuda")
    A.compute_dists(dev(synth.depth_frame(cfg, 1)), dists, *intr)
    identity = aff12(np.eye(3), [0, 0, 0])

    def args(dim, D):  # (64 nodes and more are searched through the node grid)
        return (spheres[dim][0],) + _warp_nodes(D)

    def call(six, start, nodes, dq, w):
        dim = start.shape[0]
        voxel, trunc, vol2cam, _, _ = synth.volume_params(dict(dim=dim))
        vol = start.clone()
        occ = A.tsdf_occupancy(vol)
        if six:
            A.tsdf_integrate_warped6(vol, dists, voxel, trunc, synth.MAX_WEIGHT, identity, vol2cam, *intr, nodes, dq, w, 4, occupancy=occ)
        else:
            A.tsdf_integrate_warped(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, *intr, nodes, dq, w, 4, occupancy=occ)
        h, o = host(vol, np.uint32), host(occ)
        assert (h != host(start, np.uint32)).any() and o.any()
        return [h, o]

    return call, args


@pytest.mark.parametrize("six", [False, True], ids=["tsdf_integrate_warped", "tsdf_integrate_warped6"])
def test_tsdf_integrate_warped(warped, six):
    call, args = warped
    _grown_equals_fresh(lambda *a: call(six, *a), args(32, 64), args(64, 256))


def test_node_grid_shared_by_knn_and_tsdf_integrate_warped(A, warped):
    """one GridScratch per stream whichever entry point builds it: knn (1 024 nodes, the smallest set 256 queries send to
    the grid), the warped sweep over 64 nodes, the same knn again"""
    call, args = warped
    knn = ("knn", _cloud(1024, 1024), dev(np.full(1024, 0.1, np.float32)), _cloud(256, 3), 4)

    def either(kind, *a):
        if kind == "warped":
            return call(False, *a)
        idx, w = A.knn(*a)
        return [host(idx), host(w)]

    _grown_equals_fresh(either, knn, ("warped",) + args(32, 64))


def test_compact_points(A):
    def args(n):
        rng = np.random.default_rng(n)
        return _cloud(n, n), dev((rng.random(n) < 0.4).astype(np.uint8))

    def call(*a):
        return [host(t) for t in A.compact_points(*a)]

    _grown_equals_fresh(call, args(1000), args(200000))


def _image_cfg(width, height):
    return dict(synth.CONFIGS["T0"], width=width, height=height, focal=131.25 * width / 160)


def test_icp_sums(A):
    def args(width, height):
        cfg = _image_cfg(width, height)
        intr = synth.intrinsics(cfg)
        curr, ncurr = A.compute_points_normals(dev(synth.depth_frame(cfg, 1)), *intr)
        prev, nprev = A.compute_points_normals(dev(synth.depth_frame(cfg, 0)), *intr)
        return (curr, ncurr, prev, nprev, aff12(np.eye(3), [0, 0, 0])) + tuple(intr)

    def call(*a):
        sums, matched = A.icp_sums(*a)
        assert int(host(matched)[0]) > 0
        return [host(sums), host(matched)]

    _grown_equals_fresh(call, args(80, 60), args(320, 240))


def test_tsdf_clear_integrate(A):
    import torch
    voxel, trunc, vol2cam, _, _ = synth.volume_params(dict(dim=32))

    def args(width, height):
        cfg = _image_cfg(width, height)
        intr = synth.intrinsics(cfg)
        depth = dev(synth.depth_frame(cfg, 0))
        dists = torch.empty_like(depth)
        A.compute_dists(depth, dists, *intr)
        return (dists,) + tuple(intr)

    def call(dists, *intr):
        vol = torch.empty((32, 32, 32), dtype=torch.int32, device="cuda")
        A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, *intr)
        h = host(vol)
        assert (h != 0).any()
        return [h]

    _grown_equals_fresh(call, args(80, 60), args(320, 240))
