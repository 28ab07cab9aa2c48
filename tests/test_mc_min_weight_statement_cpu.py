"""CPU tests of tests/mc_min_weight_statement.py: the statement by the contract's equivalence (the indexed statement on a
weight-zeroed copy) agrees with the floor rule stated directly, and min_weight = 1 is the indexed statement.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import mc_indexed_statement as IS
import mc_min_weight_statement as FS
import mc_statement as MS
import reference_data
from mc_util import blob_volume, default_tables, sign_noise_volume, special_values_volume

bits = MS.bits

VOLUMES = {"blob": lambda: blob_volume((30, 26, 22), seed=0, holes=False, trunc=0.3),
           "noise": lambda: sign_noise_volume((21, 14, 12), 0),
           "special": lambda: special_values_volume((30, 26, 22), 0)}
FLOORS = [1, 2, 3, 65535]


def _cell(vol):
    Z, Y, X = vol.shape
    return np.array([3.0 / X, 2.5 / Y, 3.5 / Z], np.float32)


@pytest.fixture(scope="module")
def volumes():
    """the distances of mc_util's volumes with weights drawn from {0, 1, 2, 3, 65535}"""
    return {k: FS.with_weights(make(), seed=i + 1) for i, (k, make) in enumerate(sorted(VOLUMES.items()))}


def _same(a, b):
    (va, ia, ka), (vb, ib, kb) = a, b
    assert np.array_equal(ka, kb) and np.array_equal(ia, ib)
    assert va.shape == vb.shape and np.array_equal(np.isnan(va), np.isnan(vb))
    assert np.array_equal(bits(va)[~np.isnan(va)], bits(vb)[~np.isnan(vb)])


@pytest.mark.parametrize("m", FLOORS)
@pytest.mark.parametrize("kind", sorted(VOLUMES))
def test_the_two_statements_agree(volumes, kind, m):
    tri, nv = reference_data.mc_tables() if kind == "noise" else default_tables()
    vol = volumes[kind]
    assert set(np.unique(vol >> 16).tolist()) == set(FS.WEIGHTS.tolist())
    cell = _cell(vol)
    by_copy = FS.indexed_min_weight(vol, cell, tri, nv, m)
    by_rule = FS.indexed_by_rule(vol, cell, tri, nv, m)
    _same(by_copy, by_rule)
    print("%s m=%d: %d vertices, %d indices" % (kind, m, len(by_copy[0]), len(by_copy[1])))
    if kind == "noise":
        assert len(by_copy[0]) > 100 and len(by_copy[1]) > 100
    assert by_copy[1].min(initial=0) >= 0  # every index names a vertex


@pytest.mark.parametrize("kind", sorted(VOLUMES))
def test_floor_one_is_the_indexed_statement(volumes, kind):
    tri, nv = default_tables()
    vol = volumes[kind]
    assert np.array_equal(FS.zeroed(vol, 1), vol)
    _same(FS.indexed_min_weight(vol, _cell(vol), tri, nv, 1), IS.indexed(vol, _cell(vol), tri, nv))
    _same(FS.indexed_by_rule(vol, _cell(vol), tri, nv, 1), IS.indexed(vol, _cell(vol), tri, nv))


def test_a_higher_floor_never_adds_a_cube_and_the_floor_matters(volumes):
    """the floors differ on these volumes (a statement that ignored the floor would pass nothing else here), and the
    zeroed copy keeps every distance"""
    vol = volumes["noise"]
    tri, nv = default_tables()
    n = [len(FS.indexed_min_weight(vol, _cell(vol), tri, nv, m)[1]) for m in FLOORS]
    assert n[0] > n[1] > n[2] > n[3] >= 0
    for m in FLOORS:
        z = FS.zeroed(vol, m)
        assert np.array_equal(z & 0xFFFF, vol & 0xFFFF)
        assert np.array_equal(z >> 16, np.where((vol >> 16) >= m, vol >> 16, 0))
        assert not (FS.valid_cubes(vol, m) & ~FS.valid_cubes(vol, 1)).any()


def test_min_weight_validation_needs_no_gpu():
    """0 and 65536 are refused before any HIP call, with a reason; so is what the plain call refuses"""
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynfu_amd", "libdynfu_amd.so"))
    lib.dfa_last_error.restype = C.c_char_p
    f = lib.dfa_marching_cubes_indexed_min_weight
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    cell = (C.c_float * 3)(1, 1, 1)
    p = C.c_void_p(0x1000)  # (never dereferenced: every call below is refused first)
    for m in (0, 65536, -1):
        assert f(p, None, 8, 8, 8, cell, p, p, m, None, 0, None, 0, p, None) == 1
        assert b"dfa_marching_cubes_indexed_min_weight" in lib.dfa_last_error() and b"min_weight" in lib.dfa_last_error()
    assert f(None, None, 8, 8, 8, cell, p, p, 2, None, 0, None, 0, p, None) == 1 and b"bad volume" in lib.dfa_last_error()
    assert f(p, None, 8, 8, 8, cell, p, p, 2, None, 0, None, 0, None, None) == 1 and b"totals" in lib.dfa_last_error()
