"""CPU statement of dfa_color_sample in numpy, fp64: the colour volume blended over the 8 corners of a vertex's cell.

Per vertex p (float32 input), with the float32 inputs taken to fp64:
  q = R p + t with to_volume (q = p without one);  g = q / voxel_size per axis;  i0 = floor(g), f = g - i0;
  corner (dx, dy, dz) of the cell: t = wx wy wz, each factor f (d = 1) or 1 - f (d = 0); it COUNTS when it is inside the volume
  and the weight byte of its word is > 0;  den = sum of t, s_c = sum of t c over the counting corners;
  den < 0.25 or a coordinate not finite: 0, 0, 0, 0;  otherwise b, g, r = s_c / den (not rounded here) and a = 255.

sample() returns the unrounded channels, a, den and a per-vertex bound on |kernel byte - channel|: 1 for the final rounding
(rintf of a float32 quotient against the unrounded fp64 one) plus 255 * 4 * delta, where delta is the float32 deviation of g
in cells — measured by deviation() (the kernel's float32 expressions against fp64) on a case's inputs and recorded with the
cases, not guessed.  A vertex is DECIDED when |den - 0.25| > 1e-3: there `a` is exact.
"""
import numpy as np

import tsdf_warped6_statement as W6

DEN_MIN = 0.25
DEN_MARGIN = 1e-3


def cells64(vertices, voxel_size, to_volume):
    q = W6.apply64(to_volume, np.asarray(vertices, np.float32)[:, :3].astype(np.float64))
    with np.errstate(all="ignore"):
        return q / np.asarray(voxel_size, np.float32).astype(np.float64)


def cells32(vertices, voxel_size, to_volume):
    """g as the kernel forms it: mulR's fused dot + t (tsdf_warped6_statement.apply32), then one float32 division per axis"""
    q = W6.apply32(to_volume, np.asarray(vertices, np.float32)[:, :3])
    with np.errstate(all="ignore"):
        return (q / np.asarray(voxel_size, np.float32)).astype(np.float32)


def deviation(vertices, voxel_size, to_volume, dims):
    """delta: the largest |g32 - g64| in cells over the vertices within two cells of the volume (dims = (X, Y, Z)) — beyond,
    no corner of either cell is inside and the output is 0 in any arithmetic"""
    g64, g32 = cells64(vertices, voxel_size, to_volume), cells32(vertices, voxel_size, to_volume).astype(np.float64)
    with np.errstate(invalid="ignore"):
        near = (np.isfinite(g64) & (g64 >= -2.0) & (g64 <= np.asarray(dims, np.float64) + 2.0)).all(1)
    return float(np.abs(g32[near] - g64[near]).max()) if near.any() else 0.0


def sample(colors, voxel_size, vertices, to_volume, delta):
    """dict: bgr (N, 3) fp64 unrounded (0 where a == 0), a (N,) uint8, den (N,) fp64, decided (N,) bool, bound (N,) fp64"""
    colors = np.asarray(colors, np.uint32)
    Z, Y, X = colors.shape
    g = cells64(vertices, voxel_size, to_volume)
    N = len(g)
    finite = np.isfinite(g).all(1)
    gs = np.where(finite[:, None], g, 0.0)
    # (a cell far outside has no corner inside: clip before the conversion, the corners stay outside)
    gs = np.clip(gs, -4.0, np.array([X, Y, Z], np.float64) + 4.0)
    i0 = np.floor(gs).astype(np.int64)
    f = gs - i0
    den = np.zeros(N)
    s = np.zeros((N, 3))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                d = np.array([dx, dy, dz])
                at = i0 + d
                inside = ((at >= 0) & (at < np.array([X, Y, Z]))).all(1)
                word = colors[np.clip(at[:, 2], 0, Z - 1), np.clip(at[:, 1], 0, Y - 1), np.clip(at[:, 0], 0, X - 1)].astype(np.int64)
                counts = inside & ((word >> 24) > 0) & finite
                t = np.where(d == 1, f, 1.0 - f).prod(1)
                den += np.where(counts, t, 0.0)
                for ch in range(3):
                    s[:, ch] += np.where(counts, t * ((word >> (8 * ch)) & 255), 0.0)
    has = finite & (den >= DEN_MIN)
    bgr = np.where(has[:, None], s / np.where(den > 0, den, 1.0)[:, None], 0.0)
    decided = ~finite | (np.abs(den - DEN_MIN) > DEN_MARGIN)
    return dict(bgr=bgr, a=np.where(has, 255, 0).astype(np.uint8), den=den, decided=decided,
                bound=np.full(N, 1.0 + 255.0 * 4.0 * float(delta)))
