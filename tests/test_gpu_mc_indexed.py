"""-m gpu parity tests of dfa_marching_cubes_indexed (csrc/mc.hip) against tests/mc_indexed_statement.py.

Bar: BIT-EXACT — both totals, every vertex's float bits in key order, every index — with the library's default case tables
and the reference's (tests/golden/ref_mc_tables.bin); the index list has the length and the triangle order of
dfa_marching_cubes' soup from the same call site; the expansion vertices[indices] passes the table-free fp64 checker."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mc_indexed_statement as IS  # noqa: E402
import mc_statement as MS  # noqa: E402
import reference_data  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402
from mc_util import (blob_volume, checkerboard_volume, default_tables, sign_noise_volume,  # noqa: E402
                     special_values_volume)

RAGGED = (70, 33, 41)      # X % 4 != 0: voxel-by-voxel loads, one ragged segment per row
SMALL = (40, 9, 7)         # below one segment
TWO_SEGMENTS = (512, 24, 24)
BIG = (256, 256, 256)


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def _tables(which):
    return default_tables() if which == "default" else reference_data.mc_tables()


def _cell(dims):
    return np.array([3.0 / dims[0], 2.5 / dims[1], 3.5 / dims[2]], np.float32)


def _volume(kind, dims):
    return {"blob": lambda: blob_volume(dims, seed=sum(dims)), "noise": lambda: sign_noise_volume(dims, 0),
            "checkerboard": lambda: checkerboard_volume(dims), "special": lambda: special_values_volume(dims, 0)}[kind]()


def _same_bits(got, ref):
    """NaN positions first, then the bits elsewhere (as tests/test_gpu_mc.py does for the special distances)"""
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(got)[ok], bits(ref)[ok])


def _run(A, dvol, cell, dtri, dnv, occupancy=None):
    """count, then extract into buffers of exactly the totals"""
    _, _, t = A.marching_cubes_indexed(dvol, cell, dtri, dnv, 0, 0, occupancy=occupancy)
    nvert, nidx = (int(v) for v in host(t))
    verts, idx, t2 = A.marching_cubes_indexed(dvol, cell, dtri, dnv, nvert, nidx, occupancy=occupancy)
    assert [int(v) for v in host(t2)] == [nvert, nidx]
    return host(verts)[:nvert], host(idx)[:nidx], nvert, nidx


CASES = [("blob", RAGGED), ("noise", RAGGED), ("checkerboard", RAGGED), ("special", RAGGED),
         ("blob", SMALL), ("noise", SMALL), ("special", (64, 48, 40)), ("blob", (2, 2, 2)), ("noise", (260, 9, 7)),
         ("noise", TWO_SEGMENTS), ("checkerboard", TWO_SEGMENTS), ("special", TWO_SEGMENTS), ("blob", BIG)]


@pytest.mark.parametrize("kind,dims,which", [(k, d, w) for k, d in CASES for w in ("default", "reference")
                                             if d != BIG or w == "reference"])  # (one 256^3 volume)
def test_indexed_mesh_equals_the_statement(A, kind, dims, which):
    tri, nv = _tables(which)
    vol, cell = _volume(kind, dims), _cell(dims)
    ref_v, ref_i, keys = IS.indexed(vol, cell, tri, nv)
    dvol, dtri, dnv = dev(vol), dev(tri), dev(nv)
    got_v, got_i, nvert, nidx = _run(A, dvol, cell, dtri, dnv)
    print("%s %s: %d vertices, %d indices" % (kind, dims, nvert, nidx))
    assert (nvert, nidx) == (len(ref_v), len(ref_i))
    if dims != (2, 2, 2):
        assert nvert > 100
    _same_bits(got_v, ref_v)
    assert np.array_equal(got_i, ref_i)
    # the soup from the same call site: same length, same triangle order — soup vertex i lies on the edge of vertex indices[i]
    pts, total = A.marching_cubes(dvol, cell, dtri, dnv, max(nidx, 1))
    assert int(host(total)[0]) == nidx
    soup = host(pts)[:nidx]
    ekeys, low_to_high = IS.soup_edges(vol, tri, nv)
    assert np.array_equal(keys[got_i], ekeys)
    expanded = got_v[got_i]
    both = low_to_high & ~np.isnan(soup).any(axis=1)
    assert np.array_equal(bits(expanded[both]), bits(soup[both]))
    if nidx:
        MS.check_mesh_fp64(expanded, vol, cell, allow_nonfinite=(kind == "special"))
    # a second run: identical bits
    again_v, again_i, _, _ = _run(A, dvol, cell, dtri, dnv)
    assert np.array_equal(bits(again_v), bits(got_v)) and np.array_equal(again_i, got_i)


def test_volume_pointer_that_is_not_16_byte_aligned(A):
    """X % 4 == 0 but the volume starts 4 bytes into a buffer: loads voxel by voxel, chosen by the pointer"""
    import torch
    tri, nv = reference_data.mc_tables()
    dims = (256, 12, 10)
    vol, cell = sign_noise_volume(dims, 1), _cell(dims)
    buf = torch.zeros(vol.size + 1, dtype=torch.int32, device="cuda")
    buf[1:] = dev(vol).reshape(-1)
    view = buf[1:].view(vol.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ref_v, ref_i, _ = IS.indexed(vol, cell, tri, nv)
    got_v, got_i, _, _ = _run(A, view, cell, dev(tri), dev(nv))
    assert np.array_equal(bits(got_v), bits(ref_v)) and np.array_equal(got_i, ref_i)


@pytest.mark.parametrize("name,dims", [("T1", None), ("T1", (100, 77, 90))])
def test_with_the_occupancy_map_of_an_integrated_depth_frame(A, name, dims):
    """the map dfa_tsdf_clear_integrate_occ keeps: identical output with and without it, and the statement's"""
    import torch
    cfg = synth.CONFIGS[name]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    X, Y, Z = dims or (cfg["dim"],) * 3
    if dims:
        voxel = tuple(float(synth.VOLUME_SIZE / d) for d in dims)
    d = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
    A.compute_dists(dev(synth.depth_frame(cfg, 0)), d, fx, fy, cx, cy)
    vol = torch.empty((Z, Y, X), dtype=torch.int32, device="cuda")
    occ = A.tsdf_occupancy(vol)
    A.tsdf_clear_integrate(vol, d, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, occupancy=occ)
    assert 0 < float((occ != 0).float().mean()) < 1  # (a map that lets the sweep skip something)
    tri, nv = default_tables()
    dtri, dnv = dev(tri), dev(nv)
    cell = np.asarray(voxel, np.float32)
    plain_v, plain_i, nvert, nidx = _run(A, vol, cell, dtri, dnv)
    occ_v, occ_i, nvert2, nidx2 = _run(A, vol, cell, dtri, dnv, occupancy=occ)
    assert (nvert, nidx) == (nvert2, nidx2) and nvert > 1000
    assert np.array_equal(bits(occ_v), bits(plain_v)) and np.array_equal(occ_i, plain_i)
    ref_v, ref_i, _ = IS.indexed(host(vol).view(np.uint32), cell, tri, nv)
    assert np.array_equal(bits(plain_v), bits(ref_v)) and np.array_equal(plain_i, ref_i)
    _, total = A.marching_cubes(vol, cell, dtri, dnv, 1, occupancy=occ)
    assert int(host(total)[0]) == nidx
    print("%s %s: %d soup vertices -> %d vertices (%.2f x)" % (name, (X, Y, Z), nidx, nvert, nidx / nvert))


def test_capacities_count_only_and_canaries(A):
    import torch
    from dynfu_amd import _lib
    tri, nv = reference_data.mc_tables()
    dims = (260, 20, 12)
    X, Y, Z = dims
    vol, cell = sign_noise_volume(dims, 2), _cell(dims)
    ref_v, ref_i, _ = IS.indexed(vol, cell, tri, nv)
    nvert, nidx = len(ref_v), len(ref_i)
    dvol, dtri, dnv = dev(vol), dev(tri), dev(nv)
    # count only: NULL buffers, zero capacities
    _, _, t = A.marching_cubes_indexed(dvol, cell, dtri, dnv, 0, 0)
    assert [int(v) for v in host(t)] == [nvert, nidx]

    def call(cap_v, cap_i):
        verts = torch.full((cap_v + 16, 4), -7.0, dtype=torch.float32, device="cuda")
        idx = torch.full((cap_i + 64,), -7, dtype=torch.int32, device="cuda")
        tot = torch.zeros(2, dtype=torch.int32, device="cuda")
        _lib._check(_lib.load().dfa_marching_cubes_indexed(
            _lib._dev(dvol), None, X, Y, Z, _lib._farr(cell, 3), _lib._dev(dtri), _lib._dev(dnv), _lib._dev(verts), cap_v,
            _lib._dev(idx), cap_i, _lib._dev(tot), _lib._stream()))
        assert [int(v) for v in host(tot)] == [nvert, nidx]       # always exact
        assert np.all(host(verts)[cap_v:] == -7.0) and np.all(host(idx)[cap_i:] == -7)  # nothing past either buffer
        return host(verts)[:cap_v], host(idx)[:cap_i]

    v, i = call(nvert, nidx)  # exact capacities: the mesh
    assert np.array_equal(bits(v), bits(ref_v)) and np.array_equal(i, ref_i)
    call(nvert - 1, nidx)     # each capacity one short of its total: contents unspecified, canaries and totals hold
    call(nvert, nidx - 1)
    call(nvert // 2, nidx // 3)
    v, i = call(nvert + 5, nidx + 7)  # roomy
    assert np.array_equal(bits(v[:nvert]), bits(ref_v)) and np.array_equal(i[:nidx], ref_i)
    # no surface: empty volume, all-outside volume
    zero = np.zeros((8, 8, 8), np.uint32)
    assert [int(x) for x in host(A.marching_cubes_indexed(dev(zero), cell, dtri, dnv, 4, 4)[2])] == [0, 0]
    with pytest.raises(A.DynfuAmdError):
        A.marching_cubes_indexed(dvol, cell, None, dnv, 4, 4)
