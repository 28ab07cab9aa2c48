"""-m gpu parity tests of dfa_marching_cubes_indexed_min_weight (csrc/mc.hip) against tests/mc_min_weight_statement.py.

Bar: BIT-EXACT — both totals, every vertex's float bits in key order, every index — against the statement (the indexed
statement on a weight-zeroed copy of the volume) AND against dfa_marching_cubes_indexed run on that copy on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mc_indexed_statement as IS  # noqa: E402
import mc_min_weight_statement as FS  # noqa: E402
import reference_data  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402
from mc_util import default_tables, sign_noise_volume, special_values_volume  # noqa: E402

# ragged X (voxel-by-voxel loads), below one segment, one segment and four voxels, two segments
DIMS = [(2, 2, 2), (40, 9, 7), (70, 33, 41), (260, 9, 7), (512, 24, 24)]
FLOORS = [1, 2, 3]


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _tables(which):
    return default_tables() if which == "default" else reference_data.mc_tables()


def _cell(dims):
    return np.array([3.0 / dims[0], 2.5 / dims[1], 3.5 / dims[2]], np.float32)


def _volume(dims, kind="noise"):
    """distances of mc_util's volumes, weights drawn from {0, 1, 2, 3, 65535}; then, on every other row, a weight-1 voxel at
    the first and last voxel of every 256-voxel segment (x = 0 and x = X - 1 among them) between voxels of weight 65535: the
    floor decides there about the cubes across a segment's seam and at the volume's faces"""
    X, Y, Z = dims
    base = sign_noise_volume(dims, 0) if kind == "noise" else special_values_volume(dims, 0)
    vol = FS.with_weights(base, seed=sum(dims))
    w = (vol >> 16).astype(np.uint32)
    zz, yy = np.meshgrid(np.arange(Z), np.arange(Y), indexing="ij")
    rows = (zz + yy) % 2 == 0
    edge_x = sorted({x for x in (0, 255, 256, 511, X - 1) if 0 <= x < X})
    for x in edge_x:
        for nb in (x - 1, x + 1):
            if 0 <= nb < X and nb not in edge_x:
                w[:, :, nb] = np.where(rows, 65535, w[:, :, nb])
    for x in edge_x:
        w[:, :, x] = np.where(rows, 1, w[:, :, x])
    return ((vol & np.uint32(0xFFFF)) | (w << 16)).astype(np.uint32)


def _same_bits(got, ref):
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(got)[ok], bits(ref)[ok])


def _run(A, dvol, cell, dtri, dnv, m, occupancy=None):
    """count, then extract into buffers of exactly the totals"""
    _, _, t = A.marching_cubes_indexed(dvol, cell, dtri, dnv, 0, 0, occupancy=occupancy, min_weight=m)
    nvert, nidx = (int(v) for v in host(t))
    verts, idx, t2 = A.marching_cubes_indexed(dvol, cell, dtri, dnv, nvert, nidx, occupancy=occupancy, min_weight=m)
    assert [int(v) for v in host(t2)] == [nvert, nidx]
    return host(verts)[:nvert], host(idx)[:nidx], nvert, nidx


def _floored(A, dvol, cell, dtri, dnv, m, occupancy=None):
    """the new symbol whatever m is (the Python binding routes min_weight = 1 to the plain call)"""
    import torch
    from dynfu_amd import _lib
    Z, Y, X = dvol.shape

    def call(cap_v, cap_i):
        verts = torch.empty((max(cap_v, 1), 4), dtype=torch.float32, device="cuda")
        idx = torch.empty((max(cap_i, 1),), dtype=torch.int32, device="cuda")
        tot = torch.zeros(2, dtype=torch.int32, device="cuda")
        _lib._check(_lib.load().dfa_marching_cubes_indexed_min_weight(
            _lib._dev(dvol), None if occupancy is None else _lib._dev(occupancy), X, Y, Z, _lib._farr(cell, 3), _lib._dev(dtri),
            _lib._dev(dnv), m, _lib._dev(verts) if cap_v else None, cap_v, _lib._dev(idx) if cap_i else None, cap_i,
            _lib._dev(tot), _lib._stream()))
        return verts, idx, [int(v) for v in host(tot)]

    _, _, (nvert, nidx) = call(0, 0)
    verts, idx, tot = call(nvert, nidx)
    assert tot == [nvert, nidx]
    return host(verts)[:nvert], host(idx)[:nidx], nvert, nidx


@pytest.fixture(scope="module")
def volumes():
    return {d: _volume(d) for d in DIMS}


@pytest.mark.parametrize("m", FLOORS)
@pytest.mark.parametrize("dims", DIMS)
def test_floored_mesh_equals_the_statement_and_the_plain_call_on_the_zeroed_copy(A, volumes, dims, m):
    tri, nv = reference_data.mc_tables()
    vol, cell = volumes[dims], _cell(dims)
    X = dims[0]
    w = vol >> 16
    assert set(np.unique(w).tolist()) <= set(FS.WEIGHTS.tolist())
    for x in {0, X - 1} | {x for x in (255, 256, 511) if x < X}:
        assert (w[:, :, x] == 1).any()
    ref_v, ref_i, _ = FS.indexed_min_weight(vol, cell, tri, nv, m)
    dvol, dtri, dnv = dev(vol), dev(tri), dev(nv)
    got_v, got_i, nvert, nidx = _floored(A, dvol, cell, dtri, dnv, m)
    print("%s m=%d: %d vertices, %d indices" % (dims, m, nvert, nidx))
    assert (nvert, nidx) == (len(ref_v), len(ref_i))
    if dims != (2, 2, 2):
        assert nvert > 100
    _same_bits(got_v, ref_v)
    assert np.array_equal(got_i, ref_i)
    # the plain call on the zeroed copy, on the device
    cp_v, cp_i, nv2, ni2 = _run(A, dev(FS.zeroed(vol, m)), cell, dtri, dnv, 1)
    assert (nv2, ni2) == (nvert, nidx)
    assert np.array_equal(bits(cp_v), bits(got_v)) and np.array_equal(cp_i, got_i)
    # the floor matters on these volumes: the unfloored mesh is another one
    if m > 1 and dims != (2, 2, 2):
        assert len(IS.indexed(vol, cell, tri, nv)[1]) > nidx
    # through the Python binding
    py_v, py_i, _, _ = _run(A, dvol, cell, dtri, dnv, m)
    assert np.array_equal(bits(py_v), bits(got_v)) and np.array_equal(py_i, got_i)


@pytest.mark.parametrize("m", FLOORS)
@pytest.mark.parametrize("dims,kind", [((70, 33, 41), "special"), ((260, 9, 7), "noise")])
def test_with_the_default_case_table(A, dims, kind, m):
    tri, nv = default_tables()
    vol, cell = _volume(dims, kind), _cell(dims)
    ref_v, ref_i, _ = FS.indexed_min_weight(vol, cell, tri, nv, m)
    got_v, got_i, nvert, nidx = _floored(A, dev(vol), cell, dev(tri), dev(nv), m)
    assert (nvert, nidx) == (len(ref_v), len(ref_i)) and nvert > 100
    _same_bits(got_v, ref_v)
    assert np.array_equal(got_i, ref_i)


@pytest.mark.parametrize("dims", [(70, 33, 41), (512, 24, 24)])
def test_floor_one_is_the_plain_call(A, volumes, dims):
    tri, nv = reference_data.mc_tables()
    vol, cell = volumes[dims], _cell(dims)
    dvol, dtri, dnv = dev(vol), dev(tri), dev(nv)
    a_v, a_i, nvert, nidx = _floored(A, dvol, cell, dtri, dnv, 1)
    b_v, b_i, nv2, ni2 = _run(A, dvol, cell, dtri, dnv, 1)
    assert (nvert, nidx) == (nv2, ni2) and nvert > 100
    assert np.array_equal(bits(a_v), bits(b_v)) and np.array_equal(a_i, b_i)


def test_with_the_occupancy_map_of_a_volume_fused_twice(A):
    """two depth frames into one volume, the map kept by both sweeps: weights 1 and 2 coexist; identical output with and
    without the map at every floor, and the statement's"""
    import torch
    cfg = synth.CONFIGS["T1"]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    _, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    X, Y, Z = 100, 77, 90
    voxel = tuple(float(synth.VOLUME_SIZE / d) for d in (X, Y, Z))
    vol = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda")
    occ = A.tsdf_occupancy(vol)
    d = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
    A.compute_dists(dev(synth.depth_frame(cfg, 0)), d, fx, fy, cx, cy)
    A.tsdf_clear_integrate(vol, d, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, occupancy=occ)
    # the second frame sees the left part of the image only: the rest of the surface keeps weight 1
    depth1 = np.array(synth.depth_frame(cfg, 1))
    depth1[:, depth1.shape[1] // 2:] = 0
    A.compute_dists(dev(depth1), d, fx, fy, cx, cy)
    A.tsdf_integrate(vol, d, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, occupancy=occ)
    hvol = host(vol).view(np.uint32)
    w = hvol >> 16
    assert (w == 1).sum() > 1000 and (w == 2).sum() > 1000 and w.max() == 2
    assert 0 < float((occ != 0).float().mean()) < 1
    tri, nv = default_tables()
    dtri, dnv = dev(tri), dev(nv)
    cell = np.asarray(voxel, np.float32)
    counts = []
    for m in (1, 2, 3):
        plain_v, plain_i, nvert, nidx = _floored(A, vol, cell, dtri, dnv, m)
        occ_v, occ_i, nvert2, nidx2 = _floored(A, vol, cell, dtri, dnv, m, occupancy=occ)
        assert (nvert, nidx) == (nvert2, nidx2)
        assert np.array_equal(bits(occ_v), bits(plain_v)) and np.array_equal(occ_i, plain_i)
        ref_v, ref_i, _ = FS.indexed_min_weight(hvol, cell, tri, nv, m)
        assert np.array_equal(bits(plain_v), bits(ref_v)) and np.array_equal(plain_i, ref_i)
        counts.append(nvert)
    print("fused twice: vertices at floors 1, 2, 3:", counts)
    assert counts[0] > counts[1] > 1000 and counts[2] == 0


def test_capacities_count_only_and_canaries(A):
    import torch
    from dynfu_amd import _lib
    tri, nv = reference_data.mc_tables()
    dims, m = (260, 20, 12), 2
    X, Y, Z = dims
    vol, cell = _volume(dims), _cell(dims)
    ref_v, ref_i, _ = FS.indexed_min_weight(vol, cell, tri, nv, m)
    nvert, nidx = len(ref_v), len(ref_i)
    assert nvert > 100
    dvol, dtri, dnv = dev(vol), dev(tri), dev(nv)
    _, _, t = A.marching_cubes_indexed(dvol, cell, dtri, dnv, 0, 0, min_weight=m)  # count only
    assert [int(v) for v in host(t)] == [nvert, nidx]

    def call(cap_v, cap_i, floor=m, volume=dvol):
        verts = torch.full((cap_v + 16, 4), -7.0, dtype=torch.float32, device="cuda")
        idx = torch.full((cap_i + 64,), -7, dtype=torch.int32, device="cuda")
        tot = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        _lib._check(_lib.load().dfa_marching_cubes_indexed_min_weight(
            _lib._dev(volume), None, X, Y, Z, _lib._farr(cell, 3), _lib._dev(dtri), _lib._dev(dnv), floor, _lib._dev(verts),
            cap_v, _lib._dev(idx), cap_i, _lib._dev(tot), _lib._stream()))
        return host(verts), host(idx), [int(v) for v in host(tot)]

    def checked(cap_v, cap_i):
        v, i, tot = call(cap_v, cap_i)
        assert tot == [nvert, nidx]                                       # always exact
        assert np.all(v[cap_v:] == -7.0) and np.all(i[cap_i:] == -7)      # nothing past either buffer
        return v[:cap_v], i[:cap_i]

    v, i = checked(nvert, nidx)
    assert np.array_equal(bits(v), bits(ref_v)) and np.array_equal(i, ref_i)
    checked(nvert - 1, nidx)
    checked(nvert, nidx - 1)
    checked(nvert // 2, nidx // 3)
    v, i = checked(nvert + 5, nidx + 7)
    assert np.array_equal(bits(v[:nvert]), bits(ref_v)) and np.array_equal(i[:nidx], ref_i)
    # no voxel reaches the floor: totals (0, 0), nothing written
    low = dev(((vol & np.uint32(0xFFFF)) | (np.minimum(vol >> 16, 3) << 16)).astype(np.uint32))
    v, i, tot = call(8, 8, floor=4, volume=low)
    assert tot == [0, 0] and np.all(v == -7.0) and np.all(i == -7)
    # the floor's range
    for bad in (0, 65536, -1):
        with pytest.raises(A.DynfuAmdError, match="min_weight"):
            A.marching_cubes_indexed(dvol, cell, dtri, dnv, 4, 4, min_weight=bad)
    _, _, t = A.marching_cubes_indexed(dvol, cell, dtri, dnv, 0, 0, min_weight=65535)
    assert [int(v) for v in host(t)] == [len(x) for x in FS.indexed_min_weight(vol, cell, tri, nv, 65535)[:2]]
