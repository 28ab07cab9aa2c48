"""CPU checks of the point-cloud extraction (dfa_tsdf_extract_cloud / _occ / dfa_tsdf_extract_normals): the library
exports the entry points, their argument checks run before any HIP call, and the numpy statement the GPU parity tests
compare against (tests/extract_statement.py) gives the hand-computed answers on hand-made volumes."""
import ctypes
import math

import numpy as np
import pytest

import extract_statement as S

DFA_ERR_INVALID = 1
NEW = ("dfa_tsdf_extract_cloud", "dfa_tsdf_extract_cloud_occ", "dfa_tsdf_extract_normals")
ID12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.dfa_last_error.restype = ctypes.c_char_p
    L.dfa_tsdf_extract_cloud.argtypes = [vp, i, i, i, vp, vp, vp, i, vp, vp]
    L.dfa_tsdf_extract_cloud_occ.argtypes = [vp, vp, i, i, i, vp, vp, vp, i, vp, vp]
    L.dfa_tsdf_extract_normals.argtypes = [vp, i, i, i, vp, vp, vp, f, vp, i, vp, vp]
    return L


def test_entry_points_exported_and_bound(lib):
    from dynfu_amd import _lib
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in _lib.SYMBOLS, n


def _arr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# fake device addresses: validation must refuse these calls before anything dereferences them
VOL, OCC, OUT, TOT, PTS, NRM = (ctypes.c_void_p(0x10000 * k) for k in range(1, 7))


def _invalid(lib, rc, words):
    assert rc == DFA_ERR_INVALID
    assert words.encode() in lib.dfa_last_error()


def test_extract_cloud_argument_validation(lib):
    vs, aff = np.full(3, 0.01, np.float32), ID12.copy()
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 0, 8, 8, _arr(vs), _arr(aff), OUT, 16, TOT, None), "bad volume")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 8, -1, 8, _arr(vs), _arr(aff), OUT, 16, TOT, None), "bad volume")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(None, 8, 8, 8, _arr(vs), _arr(aff), OUT, 16, TOT, None), "bad volume")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 8, 8, 8, None, _arr(aff), OUT, 16, TOT, None), "null voxel_size")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 8, 8, 8, _arr(vs), None, OUT, 16, TOT, None), "vol2world")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 8, 8, 8, _arr(vs), _arr(aff), OUT, -1, TOT, None), "bad output buffer")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 8, 8, 8, _arr(vs), _arr(aff), None, 16, TOT, None), "bad output buffer")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 8, 8, 8, _arr(vs), _arr(aff), ctypes.c_void_p(0x10004), 16, TOT, None),
             "16-byte aligned")
    _invalid(lib, lib.dfa_tsdf_extract_cloud(VOL, 1 << 14, 1 << 14, 1 << 14, _arr(vs), _arr(aff), OUT, 16, TOT, None),
             "volume too large")
    _invalid(lib, lib.dfa_tsdf_extract_cloud_occ(VOL, None, 8, 8, 8, _arr(vs), _arr(aff), OUT, 16, TOT, None),
             "null occupancy map")
    _invalid(lib, lib.dfa_tsdf_extract_cloud_occ(None, OCC, 8, 8, 8, _arr(vs), _arr(aff), OUT, 16, TOT, None), "bad volume")
    _invalid(lib, lib.dfa_tsdf_extract_cloud_occ(VOL, OCC, 8, 8, 8, _arr(vs), _arr(aff), None, 4, TOT, None),
             "bad output buffer")


def test_extract_normals_argument_validation(lib):
    vs, aff, ri = np.full(3, 0.01, np.float32), ID12.copy(), np.eye(3, dtype=np.float32)
    _invalid(lib, lib.dfa_tsdf_extract_normals(None, 8, 8, 8, _arr(vs), _arr(aff), _arr(ri), 0.5, PTS, 4, NRM, None),
             "bad volume")
    _invalid(lib, lib.dfa_tsdf_extract_normals(VOL, 8, 0, 8, _arr(vs), _arr(aff), _arr(ri), 0.5, PTS, 4, NRM, None),
             "bad volume")
    _invalid(lib, lib.dfa_tsdf_extract_normals(VOL, 8, 8, 8, _arr(vs), _arr(aff), None, 0.5, PTS, 4, NRM, None), "Rinv")
    _invalid(lib, lib.dfa_tsdf_extract_normals(VOL, 8, 8, 8, _arr(vs), _arr(aff), _arr(ri), 0.5, None, 4, NRM, None),
             "null points")
    _invalid(lib, lib.dfa_tsdf_extract_normals(VOL, 8, 8, 8, _arr(vs), _arr(aff), _arr(ri), 0.5, PTS, -1, NRM, None),
             "null points")
    _invalid(lib, lib.dfa_tsdf_extract_normals(VOL, 8, 8, 8, _arr(vs), _arr(aff), _arr(ri), 0.0, PTS, 4, NRM, None),
             "must be positive")
    _invalid(lib, lib.dfa_tsdf_extract_normals(VOL, 8, 8, 8, _arr(vs), _arr(aff), _arr(ri), 0.5, ctypes.c_void_p(0x10008), 4,
                                               NRM, None), "16-byte aligned")


# ------------------------------------------------------------------------------------- the statement
def _vol(X, Y, Z, F=0.5, W=1):
    return S.pack(np.full((Z, Y, X), F, np.float32), np.full((Z, Y, X), W, np.uint32))


def _set(vol, x, y, z, F, W=1):
    vol[z, y, x] = S.pack(np.float32(F), np.uint32(W))


def _cloud(vol, aff=ID12):
    return S.extract_cloud(vol, np.ones(3, np.float32), aff)


def test_one_crossing_per_axis():
    vol = _vol(3, 3, 3)
    _set(vol, 1, 1, 1, -0.5)  # |F| = |Fn|: every crossing is an exact midpoint
    got = _cloud(vol)
    want = [  # source voxel (linear order), then dx, dy, dz
        (1.5, 1.5, 1.0),  # (1,1,0) +z
        (1.5, 1.0, 1.5),  # (1,0,1) +y
        (1.0, 1.5, 1.5),  # (0,1,1) +x
        (2.0, 1.5, 1.5), (1.5, 2.0, 1.5), (1.5, 1.5, 2.0),  # (1,1,1) +x +y +z
    ]
    assert np.array_equal(got, np.array([w + (0.0,) for w in want], np.float32))


def test_interpolation_weights_the_two_distances():
    vol = _vol(3, 3, 3, W=0)
    _set(vol, 0, 0, 0, 0.25), _set(vol, 1, 0, 0, -0.75)
    got = _cloud(vol)
    assert got.shape == (1, 4)
    # (0.5 * 0.75 + 1.5 * 0.25) / (0.25 + 0.75) = 0.75
    assert np.array_equal(got[0], np.array([0.75, 0.5, 0.5, 0.0], np.float32))


def test_plus_one_zero_weight_and_negative_zero_emit_nothing():
    base = _vol(3, 3, 3)
    _set(base, 1, 1, 1, -0.5)
    n0 = len(_cloud(base))
    v = base.copy()
    _set(v, 2, 1, 1, 1.0)  # a +1 neighbour: the +x point of (1,1,1) goes
    assert len(_cloud(v)) == n0 - 1
    v = base.copy()
    _set(v, 0, 1, 1, 1.0)  # a +1 source emits nothing either
    assert len(_cloud(v)) == n0 - 1
    v = base.copy()
    _set(v, 1, 2, 1, 0.5, W=0)  # a weightless neighbour: the +y point of (1,1,1) goes
    assert len(_cloud(v)) == n0 - 1
    v = base.copy()
    _set(v, 1, 1, 1, -0.5, W=0)  # the weightless negative voxel: no crossing at all
    assert len(_cloud(v)) == 0
    v = base.copy()
    _set(v, 1, 1, 1, -0.0)  # -0.0 is neither > 0 nor < 0
    assert S.unpack(v[1, 1, 1])[0] == 0 and np.signbit(S.unpack(v[1, 1, 1])[0])
    assert len(_cloud(v)) == 0


def test_boundary_voxels():
    # x = X - 1: no +x edge
    v = _vol(4, 3, 3)
    _set(v, 3, 1, 1, -0.5)
    got = _cloud(v)[:, :3].tolist()
    assert got == [[3.5, 1.5, 1.0], [3.5, 1.0, 1.5], [3.0, 1.5, 1.5], [3.5, 2.0, 1.5], [3.5, 1.5, 2.0]]
    # y = Y - 1: no +y edge
    v = _vol(3, 3, 3)
    _set(v, 1, 2, 1, -0.5)
    got = _cloud(v)[:, :3].tolist()
    assert got == [[1.5, 2.5, 1.0], [1.5, 2.0, 1.5], [1.0, 2.5, 1.5], [2.0, 2.5, 1.5], [1.5, 2.5, 2.0]]
    # z = Z - 1: the last slice produces nothing, not even its x / y crossings
    v = _vol(3, 3, 3)
    _set(v, 1, 1, 2, -0.5)
    assert _cloud(v)[:, :3].tolist() == [[1.5, 1.5, 2.0]]
    # slabs concatenate to the whole cloud
    rng = np.random.default_rng(3)
    v = S.pack(rng.choice([-0.5, 0.25, 1.0, -0.0], (5, 4, 5)), rng.integers(0, 2, (5, 4, 5)))
    whole = _cloud(v)
    parts = np.concatenate([S.extract_cloud(v, np.ones(3, np.float32), ID12, z, z + 2) for z in range(0, 5, 2)])
    assert len(whole) > 0 and np.array_equal(whole.view(np.uint32), parts.view(np.uint32))


def test_pose_maps_the_points():
    v = _vol(3, 3, 3)
    _set(v, 1, 1, 1, -0.5)
    aff = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, 10, 20, 30], np.float32)  # 90 degrees about z, then t
    p = _cloud(v)
    q = _cloud(v, aff)
    assert np.array_equal(q[:, 0], -p[:, 1] + 10) and np.array_equal(q[:, 1], p[:, 0] + 20)
    assert np.array_equal(q[:, 2], p[:, 2] + 30) and np.all(q[:, 3] == 0)


def test_fma32_rounds_once():
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a float32 tie; 2^-80 decides it, but is lost when the float64 sum rounds first
    a = np.float32(1 + 2.0 ** -12)
    assert S.fma32(a, a, np.float32(2.0 ** -80)) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert S.fma32(a, a, np.float32(-(2.0 ** -80))) == np.float32(1 + 2.0 ** -11)
    assert S.fma32(a, a, np.float32(0)) == np.float32(1 + 2.0 ** -11)  # the tie itself: to even
    assert S.fma32(np.float32(3), np.float32(5), np.float32(7)) == 22
    assert math.isnan(S.fma32(np.float32(np.nan), np.float32(1), np.float32(1)))


def test_normals_statement():
    X = 9
    x = np.arange(X, dtype=np.float32)
    F = np.broadcast_to(np.clip((x - 4.0) * 0.125, -1, 1), (X, X, X))  # distance grows along +x
    vol = S.pack(F, np.ones((X, X, X), np.uint32))
    vs = np.ones(3, np.float32)
    pts = np.array([[gx, 4, 4, 0] for gx in (0.5, 1.0, 1.5, 2.0, 2.5, 4.25, 5.5, 6.0, 6.5, 7.0)], np.float32)
    nrm = S.extract_normals(vol, vs, ID12, np.eye(3), 0.5, pts)
    # nearest voxel (round half to even) 0, 1, 2, 2, 2, 4, 6, 6, 6, 7; a normal only for 1 < g < X - 2 = 7
    finite = [False, False, True, True, True, True, True, True, True, False]
    assert (np.isfinite(nrm[:, 0]) == np.array(finite)).all()
    assert np.array_equal(nrm[np.array(finite)], np.tile(np.float32([1, 0, 0, 0]), (sum(finite), 1)))
    assert np.isnan(nrm[~np.array(finite), :3]).all() and (nrm[:, 3] == 0).all()
    # a rotated volume: the same gradient, rotated, after the point is taken back into the volume frame
    aff = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, 1, 2, 3], np.float32)
    R = aff[:9].reshape(3, 3)
    world = np.concatenate([pts[:, :3] @ R.T + aff[9:], pts[:, 3:]], 1).astype(np.float32)
    nr = S.extract_normals(vol, vs, aff, R.T, 0.5, world)
    assert (np.isfinite(nr[:, 0]) == np.array(finite)).all()
    assert np.array_equal(nr[np.array(finite)], np.tile(np.float32([0, 1, 0, 0]), (sum(finite), 1)))
