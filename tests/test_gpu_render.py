"""The render kernels (dynfu_amd/csrc/render.hip) against tests/render_statement.py, byte for byte — the bytes of a
pitched row beyond its last pixel included: they must be left as the caller filled them.

Scenes and cameras: tests/render_scenes.py (the synthetic sphere of dynfu_amd/synth.py, cameras that see surface AND
background).  Every compared image is checked for its inputs first (render_scenes.check_conditions: at least a tenth of
the pixels on each side of the hit / miss branch, specular bases strictly between 0 and 1), so that a pass cannot be
empty; tests/test_render_statement_cpu.py checks the same conditions without a GPU.  The 1 x 1 images are the one
exception by construction: one is a hit and one a miss."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import render_scenes as RS  # noqa: E402
import render_statement as R  # noqa: E402
import tsdf_statement as S  # noqa: E402
from dynfu_amd import synth  # noqa: E402
from gpu_util import dev, host  # noqa: E402

FILL = 0xA5
VGA_256 = dict(synth.CONFIGS["C1"])
HD_256 = dict(synth.CONFIGS["C1"], width=1280, height=720, focal=1050.0)  # C4's camera on a 256^3 volume
VGA_512 = dict(synth.CONFIGS["C2"])
CFGS = {"256-vga": VGA_256, "256-720p": HD_256, "512-vga": VGA_512}


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


_VOLUMES = {}


def _volume(A, cfg_name, cam):
    """the scene fused on the GPU (the existing sweeps), kept for the module"""
    import torch
    key = (cfg_name, cam)
    if key not in _VOLUMES:
        if len(_VOLUMES) >= 2:  # (a 512^3 volume is 512 MiB: keep at most two alive)
            _VOLUMES.pop(next(iter(_VOLUMES)))
        cfg = CFGS[cfg_name]
        intr = synth.intrinsics(cfg)
        voxel, trunc, _, _, _ = synth.volume_params(cfg)
        dim, W, H = cfg["dim"], cfg["width"], cfg["height"]
        dists = torch.empty((H, W), dtype=torch.uint16, device="cuda")
        A.compute_dists(dev(synth.depth_frame(cfg, 0)), dists, *intr)
        v = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
        for i, v2c in enumerate(RS.integration_poses(cam)):
            (A.tsdf_clear_integrate if i == 0 else A.tsdf_integrate)(v, dists, voxel, trunc, synth.MAX_WEIGHT, v2c, *intr)
        _VOLUMES[key] = (v, voxel, trunc, intr, W, H)
    return _VOLUMES[key]


def _raycast(A, cfg_name, cam):
    """point and normal maps of the existing GPU raycast (device tensors)"""
    import torch
    v, voxel, trunc, intr, W, H = _volume(A, cfg_name, cam)
    c2v, ri = RS.camera(cam)
    pts = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    nrm = torch.zeros_like(pts)
    A.tsdf_raycast_points(v, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, pts, nrm)
    return pts, nrm


def _image(rows, cols, pad=0):
    """a pitched device image filled with a marker: (whole buffer, the (rows, cols, 4) view the kernels get)"""
    import torch
    buf = torch.full((rows, cols + pad, 4), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[:, :cols]


def _expect(img, pad=0):
    """the statement's image inside the marker-filled buffer"""
    rows, cols = img.shape[:2]
    want = np.full((rows, cols + pad, 4), FILL, np.uint8)
    want[:, :cols] = img
    return want


def _same(buf, img, pad=0):
    got, want = host(buf), _expect(img, pad)
    assert got.shape == want.shape
    assert np.array_equal(got, want), "%d of %d bytes differ" % (int((got != want).sum()), want.size)


def _shade_vs_statement(A, pts, nrm, light, pad):
    """the two kernels that read float4 maps, against the statement"""
    P, N = host(pts), host(nrm)
    rows, cols = P.shape[:2]
    buf, view = _image(rows, cols, pad)
    A.render_image_points(pts, nrm, light, view)
    _same(buf, R.render_image_points(P, N, light), pad)
    buf, view = _image(rows, cols, pad)
    A.render_tangent_colors(nrm, view)
    _same(buf, R.render_tangent_colors(N), pad)


# ------------------------------------------------------------------------------- shade kernels == statement ----
@pytest.mark.parametrize("light", RS.LIGHTS, ids=["origin", "off-axis"])
@pytest.mark.parametrize("cfg_name", ["256-vga", "256-720p"])
def test_shade_kernels_equal_statement(A, cfg_name, light):
    pts, nrm = _raycast(A, cfg_name, "turned")
    RS.check_conditions(host(pts), host(nrm), light)
    _shade_vs_statement(A, pts, nrm, light, pad=0)
    _shade_vs_statement(A, pts, nrm, light, pad=24)  # a row step larger than the row


@pytest.mark.parametrize("size", [(37, 53), (9, 130), (101, 150)])
def test_shade_kernels_ragged_sizes_and_steps(A, size):
    """cols not a multiple of 64, rows not a multiple of 4 or 8; the maps are windows of the VGA maps across the edge of
    the surface, read in place (their row step is the VGA row's) and from a dense copy"""
    pts, nrm = _raycast(A, "256-vga", "turned")
    P = host(pts)
    hit = ~np.isnan(P[..., 0])
    rows, cols = size
    # the window with the most even split of hits and misses among those centred on the image's middle row
    y0 = (P.shape[0] - rows) // 2
    share = [hit[y0:y0 + rows, x:x + cols].mean() for x in range(0, P.shape[1] - cols, 8)]
    x0 = 8 * int(np.argmin(np.abs(np.array(share) - 0.5)))
    wp, wn = pts[y0:y0 + rows, x0:x0 + cols], nrm[y0:y0 + rows, x0:x0 + cols]
    for light in RS.LIGHTS:
        RS.check_conditions(host(wp), host(wn), light)
        for p, n in ((wp, wn), (wp.contiguous(), wn.contiguous())):
            _shade_vs_statement(A, p, n, light, pad=0)
            _shade_vs_statement(A, p, n, light, pad=3)


def test_shade_kernels_one_pixel(A):
    pts, nrm = _raycast(A, "256-vga", "turned")
    hit = ~np.isnan(host(pts)[..., 0])
    ys, xs = np.nonzero(hit)
    ym, xm = np.nonzero(~hit)
    for y, x in ((int(ys[len(ys) // 2]), int(xs[len(xs) // 2])), (int(ym[len(ym) // 2]), int(xm[len(xm) // 2]))):
        p, n = pts[y:y + 1, x:x + 1].contiguous(), nrm[y:y + 1, x:x + 1].contiguous()
        for light in RS.LIGHTS:
            _shade_vs_statement(A, p, n, light, pad=0)
            _shade_vs_statement(A, p, n, light, pad=5)


@pytest.mark.parametrize("light", RS.LIGHTS, ids=["origin", "off-axis"])
@pytest.mark.parametrize("cfg_name", ["256-vga", "256-720p"])
def test_depth_form_equals_statement(A, cfg_name, light):
    import torch
    v, voxel, trunc, intr, W, H = _volume(A, cfg_name, "turned")
    c2v, ri = RS.camera("turned")
    dep = torch.zeros((H, W), dtype=torch.uint16, device="cuda")
    nrm = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    A.tsdf_raycast_depth(v, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, dep, nrm)
    D, N = host(dep), host(nrm)
    # the input conditions, on the points the kernel reprojects
    z = D.astype(np.float32) * np.float32(0.001)
    P = np.full((H, W, 4), np.nan, np.float32)
    u, w = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    P[..., 0], P[..., 1], P[..., 2] = z * (u - intr[2]) / intr[0], z * (w - intr[3]) / intr[1], z
    P[D == 0] = np.nan
    RS.check_conditions(P, N, light)
    for pad in (0, 16):
        buf, view = _image(H, W, pad)
        A.render_image_depth(dep, nrm, *intr, light, view)
        _same(buf, R.render_image_depth(D, N, *intr, light), pad)


# ----------------------------------------------------------------------- fused launch == raycast + shade ----
def _two_launches(A, pts, nrm, light, mode):
    """raycast maps shaded by the shade kernels on the GPU, assembled as the fused launch lays them out"""
    rows, cols = pts.shape[:2]
    out = []
    if mode != R.NORMALS:
        buf, view = _image(rows, cols)
        A.render_image_points(pts, nrm, light, view)
        out.append(host(buf))
    if mode != R.PHONG:
        buf, view = _image(rows, cols)
        A.render_tangent_colors(nrm, view)
        out.append(host(buf))
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("cam", RS.CAMERAS)
@pytest.mark.parametrize("cfg_name", ["512-vga", "256-720p"])
def test_fused_launch_equals_raycast_then_shade(A, cfg_name, cam):
    """every mode, both lights, a moved camera and a camera that sees the volume from behind"""
    v, voxel, trunc, intr, W, H = _volume(A, cfg_name, cam)
    c2v, ri = RS.camera(cam)
    pts, nrm = _raycast(A, cfg_name, cam)
    for light in RS.LIGHTS:
        RS.check_conditions(host(pts), host(nrm), light)
        images = {}
        for mode in (R.PHONG, R.NORMALS, R.BOTH):
            wide = 2 * W if mode == R.BOTH else W
            for pad in (0, 8):
                buf, view = _image(H, wide, pad)
                A.tsdf_raycast_render(v, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, W, H, light, mode, view)
                _same(buf, _two_launches(A, pts, nrm, light, mode), pad)
            images[mode] = host(view)
        # side by side: the left half is the Phong view alone, the right half the normal colours alone
        assert np.array_equal(images[R.BOTH][:, :W], images[R.PHONG])
        assert np.array_equal(images[R.BOTH][:, W:], images[R.NORMALS])
        # and the GPU's two launches are the statement's image of the GPU's maps
        assert np.array_equal(images[R.BOTH], R.render_maps(host(pts), host(nrm), light, R.BOTH))


def test_fused_launch_equals_the_numpy_statement(A):
    """raycast AND shading restated in numpy (tsdf_statement.raycast_points, then render_statement), on the fused sphere
    and sizes tests/test_tsdf_statement_cpu.py runs the numpy raycast on"""
    vol, voxel, trunc, c2v, ri, intr, W, H = RS.small_sphere()
    P, N = S.raycast_points(vol, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, W, H)
    v = dev(vol)
    for light in RS.LIGHTS:
        RS.check_conditions(P, N, light)
        for mode in (R.PHONG, R.NORMALS, R.BOTH):
            wide = 2 * W if mode == R.BOTH else W
            for pad in (0, 7):
                buf, view = _image(H, wide, pad)
                A.tsdf_raycast_render(v, voxel, trunc, c2v, ri, *intr, RS.STEP, RS.DELTA, W, H, light, mode, view)
                _same(buf, R.render_maps(P, N, light, mode), pad)


def test_fused_launch_ragged_image(A):
    """an image that is not a whole number of the raycaster's 16 x 16 tiles, 1 x 1 included"""
    vol, voxel, trunc, c2v, ri, intr, W, H = RS.small_sphere()
    v = dev(vol)
    for (w, h) in ((W - 7, H - 5), (1, 1)):
        intr2 = (intr[0], intr[1], (w - 1) / 2, (h - 1) / 2)
        P, N = S.raycast_points(vol, voxel, trunc, c2v, ri, *intr2, RS.STEP, RS.DELTA, w, h)
        if w > 1:
            RS.check_conditions(P, N, RS.LIGHTS[1])
        buf, view = _image(h, 2 * w, 3)
        A.tsdf_raycast_render(v, voxel, trunc, c2v, ri, *intr2, RS.STEP, RS.DELTA, w, h, RS.LIGHTS[1], R.BOTH, view)
        _same(buf, R.render_maps(P, N, RS.LIGHTS[1], R.BOTH), 3)


def test_argument_errors_are_loud(A):
    import torch
    pts = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(A.DynfuAmdError):
        A.render_image_points(pts, pts, [0, 0, 0], torch.zeros((4, 3, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(A.DynfuAmdError):
        A.render_tangent_colors(pts, torch.zeros((4, 4, 4), dtype=torch.int32, device="cuda"))
    v = torch.zeros((8, 8, 8), dtype=torch.int32, device="cuda")
    with pytest.raises(A.DynfuAmdError, match="unknown render mode"):
        A.tsdf_raycast_render(v, [0.1] * 3, 0.1, np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), np.eye(3), 1.0, 1.0,
                              0.0, 0.0, 0.75, 0.5, 4, 4, [0, 0, 0], 5, torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda"))
