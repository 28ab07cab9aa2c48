"""CPU statement of dfa_tsdf_integrate_warped6_color's colour half in numpy (the TSDF half is tsdf_warped6_statement's, and
the C call's volume is compared with the plain call's bit for bit).

It composes tsdf_warped6_statement.camera_points (steps 1-6) and tsdf_warped_statement.probe (the first half of step 7)
exactly as tsdf_warped6_statement.integrate does: that gives, per voxel, the texel (px, py) the distance is fetched from,
`updated`, this frame's `tsdf` and the DECIDED set — which already requires the texel and (tsdf == 1) to agree at all 27
perturbed points, so the colour rule needs no further margin: it is integer arithmetic on a decided texel.

The rule (include/dynfu_amd.h), for a voxel with updated and tsdf < 1 (`coloured`):
  o the old word, w = o >> 24, pixel = image[py, px] (b, g, r, x);
  per channel c with the pixel's byte `in`:  c' = (c w + in + ((w + 1) >> 1)) // (w + 1);
  w' = min(w + 1, max_color_weight);  every other word is left alone.
"""
import numpy as np

import tsdf_warped6_statement as W6
import tsdf_warped_statement as WST
from extract_statement import fma32

FAR = 1 << 40  # a texel coordinate far from every image


def rule(old, pix, max_color_weight):
    """the rule on arrays of words `old` and pixels `pix` (uint32 each, bytes b, g, r, weight / x) -> the new words"""
    o = np.asarray(old, np.uint32).astype(np.int64)
    p = np.asarray(pix, np.uint32).astype(np.int64)
    w = o >> 24
    new = np.minimum(w + 1, int(max_color_weight)) << 24
    for ch in range(3):
        c, i = (o >> (8 * ch)) & 255, (p >> (8 * ch)) & 255
        new |= ((c * w + i + ((w + 1) >> 1)) // (w + 1)) << (8 * ch)
    return new.astype(np.uint32)


def rule_scalar(o, pix, max_color_weight):
    """one word, in plain Python integers"""
    o, pix = int(o), int(pix)
    w = o >> 24
    new = min(w + 1, int(max_color_weight)) << 24
    for ch in range(3):
        c, i = (o >> (8 * ch)) & 255, (pix >> (8 * ch)) & 255
        new |= ((c * w + i + ((w + 1) >> 1)) // (w + 1)) << (8 * ch)
    return new


def pixels(image):
    """(rows, cols, 4) uint8 b, g, r, x -> (rows, cols) uint32, byte 0 = b"""
    return np.ascontiguousarray(image, np.uint8).view("<u4")[..., 0]


def texels(shape, dists, voxel_size, trunc, vol2node, node2cam, fx, fy, cx, cy, nodes, node_dq, node_w, k, mode):
    """camera_points + probe as tsdf_warped6_statement.integrate composes them.  dict of (Z, Y, X) arrays: updated, decided
    (bool), px, py (int64, -1 where nothing is fetched), tsdf (float32), qx, qy (raw_texels: what an UNDECIDED voxel's texel is
    measured against — an active voxel outside the image has a projection, and no px)"""
    c = W6.camera_points(shape, voxel_size, vol2node, node2cam, nodes, node_dq, node_w, k, mode)
    act, vc64 = c["active"], c["vc64"]
    rho = 2 * W6.WARPED6_DEVIATION * W6.frame_scale(c)
    n = len(act)
    upd, px, py, tsdf = np.zeros(n, bool), np.full(n, -1), np.full(n, -1), np.full(n, np.nan, np.float32)
    qx, qy = np.full(n, FAR), np.full(n, FAR)
    decided = (np.abs(c["qmin"].astype(np.float64) - 1.0) > WST.Q_MARGIN) & ~c["hemi"]
    if act.any():
        a = np.flatnonzero(act)
        u0, x0, y0, t0 = WST.probe(vc64[a].astype(np.float32), dists, trunc, fx, fy, cx, cy)
        upd[a], px[a], py[a], tsdf[a] = u0, x0, y0, t0
        qx[a], qy[a] = raw_texels(vc64[a].astype(np.float32), fx, fy, cx, cy)
        same = np.ones(len(a), bool)
        for s in np.ndindex(3, 3, 3):
            if s == (1, 1, 1):
                continue
            u, x, y, t = WST.probe((vc64[a] + rho * (np.array(s, np.float64) - 1)).astype(np.float32), dists, trunc, fx, fy, cx, cy)
            same &= (u == u0) & (x == x0) & (y == y0) & ((t == 1) == (t0 == 1))
        decided[a] &= same
    r = lambda m: m.reshape(shape)
    return dict(updated=r(upd), decided=r(decided), px=r(px), py=r(py), tsdf=r(tsdf), qx=r(qx), qy=r(qy))


def raw_texels(vc, fx, fy, cx, cy):
    """floor of the projection of camera-frame points vc (n, 3) float32, by probe's expressions, NOT clipped to the image:
    (qx, qy) int64, FAR where vc.z <= 0 or the projection is not finite"""
    vc = np.asarray(vc, np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        coox = fma32(np.float32(fx), vc[:, 0] / vc[:, 2], np.float32(cx))
        cooy = fma32(np.float32(fy), vc[:, 1] / vc[:, 2], np.float32(cy))
    ok = (vc[:, 2] > 0) & np.isfinite(coox) & np.isfinite(cooy) & (np.abs(coox) < 1e9) & (np.abs(cooy) < 1e9)
    return (np.where(ok, np.floor(np.where(ok, coox, 0)), FAR).astype(np.int64),
            np.where(ok, np.floor(np.where(ok, cooy, 0)), FAR).astype(np.int64))


def apply(colors, image, tex, max_color_weight):
    """one call's colour half on `colors` (uint32 (Z, Y, X)) given texels(): (the new colour volume, coloured (bool))"""
    colors = np.array(colors, np.uint32)
    with np.errstate(invalid="ignore"):
        col = tex["updated"] & (tex["tsdf"] < np.float32(1))
    if col.any():
        pix = pixels(image)[tex["py"][col], tex["px"][col]]
        colors[col] = rule(colors[col], pix, max_color_weight)
    return colors, col


def integrate(colors, image, dists, voxel_size, trunc, max_color_weight, vol2node, node2cam, fx, fy, cx, cy, nodes, node_dq, node_w, k,
              mode):
    """The call's colour half.  dict: colors (the new colour volume), coloured, and texels()'s arrays"""
    tex = texels(np.asarray(colors).shape, dists, voxel_size, trunc, vol2node, node2cam, fx, fy, cx, cy, nodes, node_dq, node_w, k, mode)
    out, col = apply(colors, image, tex, max_color_weight)
    return dict(tex, colors=out, coloured=col)
