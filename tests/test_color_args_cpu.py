"""dfa_tsdf_integrate_warped6_color and dfa_color_sample check their arguments before they touch the GPU: the three refusals
of the coloured call's own arguments (colors == NULL, image == NULL, max_color_weight outside 1..255) come first, then the
plain call's, each DFA_ERR_INVALID (1) with its text in dfa_last_error()."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (torch's bundled HIP runtime must be the one the library binds to)
    from dynfu_amd import build as B
    L = ctypes.CDLL(B.build())
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.dfa_tsdf_integrate_warped6_color.argtypes = [vp, i, i, i, vp, i, vp, vp, i, i, i, vp, vp, f, i, i, vp, vp, f, f, f, f, vp, vp, vp,
                                                   i, i, i, vp, vp]
    L.dfa_color_sample.argtypes = [vp, i, i, i, vp, vp, i, i, vp, vp, vp]
    L.dfa_last_error.restype = ctypes.c_char_p
    return L


P = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused first
VS = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
IDENT = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)


def fused(lib, image=P, image_step=32, volume=P, colors=P, cap=255, dims=(8, 8, 8), k=8, mode=0, D=4, pos=P, v2n=IDENT, dists=P):
    return lib.dfa_tsdf_integrate_warped6_color(dists, 16, 8, 8, image, image_step, volume, colors, dims[0], dims[1], dims[2], None, VS,
                                                0.1, 64, cap, v2n, IDENT, 10.0, 10.0, 4.0, 4.0, pos, P, P, D, k, mode, None, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(colors=None), b"null colour volume"),
    (dict(image=None), b"null colour image"),
    (dict(cap=0), b"max_color_weight outside 1..255"),
    (dict(cap=256), b"max_color_weight outside 1..255"),
    (dict(cap=-3), b"max_color_weight outside 1..255"),
    # ... each of them with and without a TSDF volume, and ahead of the plain call's own refusals
    (dict(colors=None, volume=None), b"null colour volume"),
    (dict(image=None, volume=None, k=0), b"null colour image"),
    (dict(cap=0, dims=(0, 8, 8)), b"max_color_weight outside 1..255"),
])
def test_the_three_refusals(lib, kw, msg):
    assert fused(lib, **kw) == 1, kw
    err = lib.dfa_last_error()
    assert b"dfa_tsdf_integrate_warped6_color" in err and msg in err, (kw, err)


@pytest.mark.parametrize("kw, msg", [
    (dict(dims=(8, 0, 8)), b"bad volume"), (dict(dists=None), b"bad dists image"), (dict(k=9), b"k out of range 1..8"),
    (dict(mode=2), b"unknown unsupported_mode"), (dict(pos=None), b"nodes without"), (dict(D=-1), b"negative node count"),
    (dict(image_step=31), b"image row step smaller than a pixel row"), (dict(image_step=34), b"image rows must be 4-byte aligned"),
    (dict(image=ctypes.c_void_p(0x1002)), b"image rows must be 4-byte aligned"),
    (dict(v2n=(ctypes.c_float * 12)(1, 0.01, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)), b"vol2node must be rigid"),
])
def test_the_plain_calls_refusals_follow(lib, kw, msg):
    for volume in (P, None):  # (colours only: the geometry is checked on the colour volume)
        assert fused(lib, volume=volume, **kw) == 1, kw
        err = lib.dfa_last_error()
        assert b"dfa_tsdf_integrate_warped6_color" in err and msg in err, (kw, err)


def test_nothing_to_do_is_no_hip_call(lib):
    """no nodes, SKIP mode: valid, every voxel is left alone — with and without a TSDF volume"""
    for volume in (P, None):
        assert lib.dfa_tsdf_integrate_warped6_color(P, 16, 8, 8, P, 32, volume, P, 8, 8, 8, None, VS, 0.1, 64, 255, None, None, 10.0, 10.0,
                                                    4.0, 4.0, None, None, None, 0, 8, 0, None, None) == 0


def test_color_sample_arguments(lib):
    def call(colors=P, dims=(8, 8, 8), voxel=VS, verts=P, stride=3, N=5, out=P):
        return lib.dfa_color_sample(colors, dims[0], dims[1], dims[2], voxel, verts, stride, N, None, out, None)

    for kw, msg in ((dict(colors=None), b"bad colour volume"), (dict(dims=(8, 8, 0)), b"bad colour volume"),
                    (dict(voxel=None), b"voxel size must be positive"),
                    (dict(voxel=(ctypes.c_float * 3)(0.1, 0.0, 0.1)), b"voxel size must be positive"),
                    (dict(stride=2), b"stride must be 3 or 4"), (dict(stride=5), b"stride must be 3 or 4"),
                    (dict(N=-1), b"null vertices / out"), (dict(verts=None), b"null vertices / out"), (dict(out=None), b"null vertices / out"),
                    (dict(out=ctypes.c_void_p(0x1001)), b"out must be 4-byte aligned")):
        assert call(**kw) == 1, kw
        err = lib.dfa_last_error()
        assert b"dfa_color_sample" in err and msg in err, (kw, err)
    assert call(N=0, verts=None, out=None) == 0  # N == 0 succeeds, without a launch
