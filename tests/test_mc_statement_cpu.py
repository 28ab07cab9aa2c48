"""CPU tests of tests/mc_statement.py (the numpy statement of marching cubes the -m gpu tests compare csrc/mc.hip with)
and of the inputs tests/mc_util.py adds for them.  No GPU."""
import numpy as np
import pytest

import mc_statement as S
import oracle as O
import reference_data
from mc_util import (SPECIAL_HALVES, blob_volume, checkerboard_volume, default_tables, pack, sign_noise_volume,
                     special_values_volume)

bits = S.bits
BLOB_DIMS = [(64, 64, 64), (128, 128, 128), (50, 38, 44), (256, 24, 40), (260, 9, 7), (2, 2, 2), (67, 5, 130)]
NOISE_DIMS = (512, 24, 24)
RAGGED_DIMS = (130, 11, 9)


def _tables(which):
    return default_tables() if which == "default" else reference_data.mc_tables()


def _cell(dims):
    return np.array([3.0 / dims[0], 2.5 / dims[1], 3.5 / dims[2]], np.float32)


def _same_bits(got, ref):
    """NaN positions first, then the bits elsewhere"""
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(got)[ok], bits(ref)[ok])


def _volume(kind, dims):
    if kind == "noise":
        return sign_noise_volume(dims, 0)
    if kind == "checkerboard":
        return checkerboard_volume(dims)
    return special_values_volume(dims, 0)


@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("dims", BLOB_DIMS)
def test_statement_equals_the_oracle_on_the_blob_volumes(dims, which):
    tri, nv = _tables(which)
    vol = blob_volume(dims, seed=sum(dims))
    ref, total, _ = O.marching_cubes(vol, _cell(dims), tri, nv)
    got, n = S.marching_cubes(vol, _cell(dims), tri, nv)
    assert n == total and np.array_equal(bits(got), bits(ref))
    assert S.count(vol, nv) == total


@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("dims", [NOISE_DIMS, RAGGED_DIMS])
@pytest.mark.parametrize("kind", ["noise", "checkerboard", "special"])
def test_statement_equals_the_oracle_on_the_new_volumes(kind, dims, which):
    tri, nv = _tables(which)
    vol = _volume(kind, dims)
    ref, total, _ = O.marching_cubes(vol, _cell(dims), tri, nv)
    got, n = S.marching_cubes(vol, _cell(dims), tri, nv, slab=5)
    assert n == total > 100
    _same_bits(got, ref)
    if kind == "special":
        assert np.isnan(ref).any() and not np.isnan(ref).all()  # inf / inf and NaN distances reach the output
    # the integer-only count, whole and slab by slab, and the integer-only case decision
    assert S.count(vol, nv) == total
    assert sum(S.count(vol, nv, z, z + 3) for z in range(0, dims[2], 3)) == total
    assert np.array_equal(S.cube_cases(vol, integer=True), S.cube_cases(vol))


def test_slabs_concatenate_to_the_whole_also_from_partial_volumes():
    tri, nv = reference_data.mc_tables()
    dims = (50, 38, 44)
    vol, cell = blob_volume(dims, seed=1), _cell(dims)
    whole, n = S.marching_cubes(vol, cell, tri, nv, slab=dims[2])
    for cuts in ([0, 1, 2, 20, 43, 44], [0, 17, 50]):
        parts = [S.vertices(vol, cell, tri, nv, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole))
        # ... handed only the slices a slab needs (z0 .. z1), as a volume fetched slab by slab is
        parts = [S.vertices(vol[a:min(b, dims[2] - 1) + 1], cell, tri, nv, a, b, z_base=a, Z=dims[2])
                 for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole))
        assert sum(S.count(vol[a:min(b, dims[2] - 1) + 1], nv, a, b, z_base=a, Z=dims[2])
                   for a, b in zip(cuts[:-1], cuts[1:])) == n
    assert len(S.vertices(vol, cell, tri, nv, 43, 60)) == 0  # the last slice starts no cube


def test_the_noise_volume_reaches_what_the_kernels_are_sized_for():
    """a change to the generator cannot silently make the GPU test easy: all 254 non-trivial cases, a lane group (four
    consecutive cubes, x % 4 == 0) with 20 triangles — the limit of the count sweep's 5-bit sum —, a 256-cube row segment
    with at least 2 000 vertices"""
    _, nv = reference_data.mc_tables()
    vol = sign_noise_volume(NOISE_DIMS, 0)
    cases = S.cube_cases(vol)
    present = np.unique(cases)
    assert len(set(present.tolist()) - {0, 255}) == 254
    n = S.cube_counts(vol, nv)
    pad = np.zeros(n.shape[:2] + (512,), np.int64)
    pad[:, :, :n.shape[2]] = n
    lanes = pad.reshape(n.shape[0], n.shape[1], 128, 4).sum(-1) // 3
    assert lanes.max() >= 20
    segs = pad.reshape(n.shape[0], n.shape[1], 2, 256).sum(-1)
    assert segs.max() >= 2000
    assert n.sum() > 2_000_000
    # the checkerboard: every cube one of the two densest cases, 3 072 vertices in a full segment
    cb = S.cube_cases(checkerboard_volume(NOISE_DIMS))
    assert set(np.unique(cb).tolist()) == {0x5A, 0xA5} and nv[0x5A] == nv[0xA5] == 12
    # the special values: every pattern is there, beside a voxel of the other sign class
    sp = special_values_volume(NOISE_DIMS, 0)
    held = set(np.unique(sp[(sp >> 16) != 0] & 0xFFFF).tolist())
    assert set(SPECIAL_HALVES.tolist()) <= held


@pytest.mark.parametrize("kind,dims", [("noise", (50, 38, 44)), ("checkerboard", (33, 20, 12)), ("blob", (64, 64, 64)),
                                       ("noise", NOISE_DIMS)])
def test_check_mesh_fp64_passes_on_the_statement_and_the_oracle(kind, dims):
    tri, nv = reference_data.mc_tables()
    vol = blob_volume(dims, seed=2) if kind == "blob" else _volume(kind, dims)
    cell = _cell(dims)
    pts, n = S.marching_cubes(vol, cell, tri, nv)
    assert n > 1000
    edge = S.check_mesh_fp64(pts, vol, cell)
    assert S.check_mesh_fp64.worst_ulps < 4.0
    S.check_voxel_order(edge, dims)
    S.check_mesh_fp64(O.marching_cubes(vol, cell, *default_tables())[0], vol, cell)  # the other table, the other code


def test_check_mesh_fp64_negative_controls():
    tri, nv = reference_data.mc_tables()
    dims = (50, 38, 44)
    vol, cell = blob_volume(dims, seed=2), _cell(dims)
    pts, n = S.marching_cubes(vol, cell, tri, nv)
    edge = S.check_mesh_fp64(pts, vol, cell)
    S.check_voxel_order(edge, dims)
    # one vertex moved by 1e-4 of a cell along its edge (across it the coordinate would simply stop being a lattice one)
    for i in (0, n // 2, n - 1):
        moved = pts.copy()
        a = edge[i, 0]
        moved[i, a] += np.float32(1e-4) * cell[a]
        assert moved[i, a] != pts[i, a]
        with pytest.raises(S.MeshError):
            S.check_mesh_fp64(moved, vol, cell)
    # two vertices swapped across cubes: every vertex still lies on its edge, the order (and the bits) are wrong
    swapped = pts.copy()
    swapped[[3, n - 4]] = swapped[[n - 4, 3]]
    with pytest.raises(S.MeshError):
        S.check_voxel_order(S.check_mesh_fp64(swapped, vol, cell), dims)
    assert not np.array_equal(bits(swapped), bits(O.marching_cubes(vol, cell, tri, nv)[0]))
    # a table row with its winding and length unchanged but one edge id replaced by an edge the case does not cross
    cases = S.cube_cases(vol)
    counts = np.bincount(cases.reshape(-1), minlength=256)
    counts[[0, 255]] = 0
    c = int(counts.argmax())
    uncrossed = [e for e, (p, q) in enumerate(S.EDGE) if ((c >> p) & 1) == ((c >> q) & 1)]
    bad_tri = tri.copy()
    bad_tri[c, 1] = uncrossed[0]
    bad, nb = S.marching_cubes(vol, cell, bad_tri, nv)
    assert nb == n
    with pytest.raises(S.MeshError):
        S.check_mesh_fp64(bad, vol, cell)
    # a vertex on an edge whose end has no weight
    holes = vol.copy()
    x, y, z = edge[n // 3, 1:4]
    holes[z, y, x] &= np.uint32(0xFFFF)
    with pytest.raises(S.MeshError):
        S.check_mesh_fp64(pts, holes, cell)


@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("corner", range(8))
@pytest.mark.parametrize("inverted", [False, True])
def test_one_cube_with_one_corner_apart(corner, inverted, which):
    """2 x 2 x 2 voxels = one cube.  One corner at -0.25 among +0.75 (case 1 << corner) or at +0.25 among -0.75 (its
    complement): a triangle around that corner, a quarter of the way along each of its three edges — every number below
    is exact in binary, so the expected points are written down, not computed by the statement's formula."""
    tri, nv = _tables(which)
    cell = np.array([1.0, 2.0, 4.0], np.float32)
    f = np.full((2, 2, 2), -0.75 if inverted else 0.75)
    dx, dy, dz = S.CORNER[corner]
    f[dz, dy, dx] = 0.25 if inverted else -0.25
    vol = pack(f, np.ones((2, 2, 2), np.uint32))
    case = (255 - (1 << corner)) if inverted else (1 << corner)
    assert S.cube_cases(vol).tolist() == [[[case]]]
    got, n = S.marching_cubes(vol, cell, tri, nv)
    assert n == 3 and nv[case] == 3
    centre = lambda k: (np.asarray(S.CORNER[k]) + 0.5) * cell  # (0.5 or 1.5) * (1, 2, 4)
    expect = []
    for e in tri[case, :3]:
        p, q = S.EDGE[e]
        assert corner in (p, q)
        other = q if p == corner else p
        expect.append(list(centre(corner) + 0.25 * (centre(other) - centre(corner))) + [1.0])
    assert sorted(tri[case, :3].tolist()) == sorted(e for e, pq in enumerate(S.EDGE.tolist()) if corner in pq)
    assert np.array_equal(got, np.array(expect, np.float32))
    assert np.array_equal(bits(got), bits(O.marching_cubes(vol, cell, tri, nv)[0]))
    # no weight at one corner: nothing
    vol[1, 1, 1] &= np.uint32(0xFFFF)
    assert S.marching_cubes(vol, cell, tri, nv)[1] == 0 and S.count(vol, nv) == 0


def test_case_decision_on_special_distances():
    """NaN < 0 is false, -0 < 0 is false, a negative denormal and -inf are negative"""
    halves = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x83FF, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0xFBFF], np.uint32)
    want = np.array([0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1], bool)
    assert np.array_equal(S.half_to_float(halves) < 0, want) and np.array_equal(S.negative_int(halves), want)
    # all 65 536 patterns
    every = np.arange(65536, dtype=np.uint32)
    assert np.array_equal(S.negative_int(every), S.half_to_float(every) < 0)
