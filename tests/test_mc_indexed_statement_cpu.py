"""CPU tests of tests/mc_indexed_statement.py (the numpy statement the -m gpu tests compare dfa_marching_cubes_indexed
with) and of the precondition the contract puts on the case table.  No GPU."""
import numpy as np
import pytest

import mc_indexed_statement as IS
import mc_statement as MS
import reference_data
from mc_util import blob_volume, checkerboard_volume, default_tables, sign_noise_volume, special_values_volume

bits = MS.bits

VOLUMES = {"blob": lambda: blob_volume((64, 64, 64), seed=0), "noise": lambda: sign_noise_volume((24, 24, 24), 0),
           "checkerboard": lambda: checkerboard_volume((33, 20, 12)), "special": lambda: special_values_volume((48, 48, 48), 0)}


def _tables(which):
    return default_tables() if which == "default" else reference_data.mc_tables()


def _cell(vol):
    Z, Y, X = vol.shape
    return np.array([3.0 / X, 2.5 / Y, 3.5 / Z], np.float32)


@pytest.mark.parametrize("which", ["default", "reference"])
def test_every_case_of_the_table_references_exactly_its_crossed_edges(which):
    """the precondition of include/dynfu_amd.h: then the vertex set (sign and weight rule) is the set of edges the emitted
    triangles reference"""
    tri, nv = _tables(which)
    tri = np.asarray(tri).reshape(256, 16)
    per_case = MS.vertices_per_case(nv)
    for cs in range(256):
        crossed = {e for e, (p, q) in enumerate(MS.EDGE) if ((cs >> p) & 1) != ((cs >> q) & 1)}
        row = tri[cs, :per_case[cs]]
        assert ((row >= 0) & (row < 12)).all(), cs
        assert set(row.tolist()) == crossed, (cs, sorted(set(row.tolist())), sorted(crossed))
        assert (tri[cs, per_case[cs]:] == -1).all() and nv[cs] == per_case[cs], cs  # (nothing hidden behind the count)


@pytest.mark.parametrize("which", ["default", "reference"])
@pytest.mark.parametrize("kind", sorted(VOLUMES))
def test_indexed_statement_against_the_soup_statement_and_fp64(kind, which):
    tri, nv = _tables(which)
    vol = VOLUMES[kind]()
    cell = _cell(vol)
    verts, idx, keys = IS.indexed(vol, cell, tri, nv)
    soup, n = MS.marching_cubes(vol, cell, tri, nv)
    assert len(idx) == n > 1000                                  # one index per soup vertex
    assert (np.diff(keys) > 0).all()                             # strictly ascending: no vertex twice
    assert idx.min() >= 0 and idx.max() < len(verts)
    # the sign and weight rule gives exactly the edges the triangles reference
    ekeys, low_to_high = IS.soup_edges(vol, tri, nv)
    assert np.array_equal(np.unique(ekeys), keys)
    assert np.array_equal(keys[idx], ekeys)
    # the expansion: the soup's bits wherever the soup interpolates from low to high, the fp64 crossing everywhere
    expanded = verts[idx]
    assert low_to_high.any() and not low_to_high.all()
    both = ~np.isnan(soup[low_to_high]).any(axis=1)
    assert np.array_equal(np.isnan(expanded[low_to_high]), np.isnan(soup[low_to_high]))
    assert np.array_equal(bits(expanded[low_to_high][both]), bits(soup[low_to_high][both]))
    # (NaN coordinates — an infinite or NaN distance, special values only — cannot name an edge: the checker skips them)
    edge = MS.check_mesh_fp64(expanded, vol, cell, allow_nonfinite=(kind == "special"))
    assert MS.check_mesh_fp64.worst_ulps < 4.0
    if kind != "special":
        Z, Y, X = vol.shape
        found = 3 * ((edge[:, 3] * Y + edge[:, 2]) * X + edge[:, 1]) + edge[:, 0]
        on_a_voxel = edge[:, 4] != 0  # (a vertex on a voxel centre lies on several edges: the checker names one of them)
        assert np.array_equal(found[~on_a_voxel], ekeys[~on_a_voxel])


def test_soup_to_unique_ratio_of_the_blob():
    """what the indexed mesh saves: the three volumes measured gave 4.53 to 5.88 soup vertices per distinct edge"""
    tri, nv = reference_data.mc_tables()
    vol = VOLUMES["blob"]()
    verts, idx, _ = IS.indexed(vol, _cell(vol), tri, nv)
    ratio = len(idx) / len(verts)
    print("blob 64^3: %d soup vertices, %d distinct edges, ratio %.2f" % (len(idx), len(verts), ratio))
    assert 4.0 <= ratio <= 6.5


def test_copies_of_a_shared_vertex_are_not_bit_equal_in_the_soup():
    """why the welding has to happen in the extraction: some copies differ in bits from the indexed vertex"""
    tri, nv = reference_data.mc_tables()
    vol = VOLUMES["blob"]()
    cell = _cell(vol)
    verts, idx, _ = IS.indexed(vol, cell, tri, nv)
    soup, _ = MS.marching_cubes(vol, cell, tri, nv)
    differ = (bits(verts[idx]) != bits(soup)).any(axis=1)
    assert 0 < differ.sum() < len(soup) // 20
    assert np.abs(verts[idx].astype(np.float64) - soup.astype(np.float64)).max() < 1e-6


def test_volumes_below_one_segment_and_without_a_surface():
    tri, nv = default_tables()
    for dims in [(2, 2, 2), (3, 2, 5)]:
        vol = sign_noise_volume(dims, 3)
        verts, idx, keys = IS.indexed(vol, _cell(vol), tri, nv)
        soup, n = MS.marching_cubes(vol, _cell(vol), tri, nv)
        assert len(idx) == n and np.array_equal(np.unique(IS.soup_edges(vol, tri, nv)[0]), keys)
    verts, idx, keys = IS.indexed(np.zeros((4, 4, 4), np.uint32), (1, 1, 1), tri, nv)
    assert len(verts) == len(idx) == 0


def test_argument_validation_needs_no_gpu():
    """arguments are checked before any HIP call: DFA_ERR_INVALID and the error string, as the neighbouring entry points"""
    import ctypes as C
    import os
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynfu_amd", "libdynfu_amd.so"))
    lib.dfa_last_error.restype = C.c_char_p
    f = lib.dfa_marching_cubes_indexed
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                  C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    cell = (C.c_float * 3)(1, 1, 1)
    p = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused first)
    assert f(None, None, 8, 8, 8, cell, p, p, None, 0, None, 0, p, None) == 1 and b"bad volume" in lib.dfa_last_error()
    for dims in [(1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8)]:
        assert f(p, None, *dims, cell, p, p, None, 0, None, 0, p, None) == 1 and b"bad volume" in lib.dfa_last_error()
    assert f(p, None, 8, 8, 8, cell, p, p, p, -1, None, 0, p, None) == 1 and b"vertex buffer" in lib.dfa_last_error()
    assert f(p, None, 8, 8, 8, cell, p, p, None, 0, p, -1, p, None) == 1 and b"index buffer" in lib.dfa_last_error()
    assert f(p, None, 8, 8, 8, cell, p, p, None, 4, None, 0, p, None) == 1  # a capacity without a buffer
    assert f(p, None, 8, 8, 8, cell, p, p, None, 0, None, 4, p, None) == 1
    assert f(p, None, 8, 8, 8, cell, None, p, None, 0, None, 0, p, None) == 1 and b"case tables" in lib.dfa_last_error()
    assert f(p, None, 8, 8, 8, cell, p, p, None, 0, None, 0, None, None) == 1 and b"totals" in lib.dfa_last_error()
