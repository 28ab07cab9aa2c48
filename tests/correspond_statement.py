"""CPU statement of the two correspondence searches in numpy: dfa_correspond (exact 1-NN of every live vertex among the
canonical ones, and the gathered clouds) and dfa_correspond_projective (the gates of find_coresp), written from the
contract in include/dynfu_amd.h — plus the choice between the four search forms of dfa_correspond (csrc/capi_warp.cpp) and the
geometry of the two grids (grid_setup_kernel, pgrid_finalize_kernel in csrc/knn_grid.hip) in float32, so that a test can say
in which cell, and how far from its walls, a query sits.

Every result is exact: integers, or float32 values compared by their bits."""
from collections import namedtuple

import numpy as np

f32 = np.float32
NAN_KEY = np.uint32(0xFFFFFFFF)  # behind every distance, +inf included


# ------------------------------------------------------------------------------------------ dfa_correspond
def nearest(canon, live, qchunk=256, cchunk=65536):
    """per live vertex the canonical point with the smallest (squared distance, index): (idx int32 (n,), d2 float32 (n,)).
    The distance is float32 ((d0*d0 + d1*d1) + d2*d2) with d = live - canon (dist2 of csrc/knn_device.hpp; nothing is
    fused).  A NaN distance is never a neighbour, an infinite one is (KnnList::pack orders the bits of the distance: +inf
    sorts before the empty slot, a NaN behind it); -1 / NaN only if every distance is NaN.
    Chunked over both axes with a running minimum: argmin takes the first of equal keys, and only a strictly smaller key
    replaces the one held, so the lower index stays."""
    canon = np.ascontiguousarray(canon, f32).reshape(-1, 3)
    live = np.ascontiguousarray(live, f32).reshape(-1, 3)
    n = len(live)
    idx = np.full(n, -1, np.int32)
    key = np.full(n, NAN_KEY, np.uint32)
    for s in range(0, n, qchunk):
        q = live[s:s + qchunk]
        bk, bi = key[s:s + qchunk], idx[s:s + qchunk]
        rows = np.arange(len(q))
        for c in range(0, len(canon), cchunk):
            p = canon[c:c + cchunk]
            with np.errstate(all="ignore"):
                d0, d1, d2 = (q[:, None, a] - p[None, :, a] for a in range(3))
                d = (d0 * d0 + d1 * d1) + d2 * d2
            # the order of non-negative floats is the order of their bits (a sum of squares is never -0)
            k = np.where(np.isnan(d), NAN_KEY, d.view(np.uint32))
            j = np.argmin(k, axis=1)
            kj = k[rows, j]
            take = kj < bk
            bk[take], bi[take] = kj[take], (c + j[take]).astype(np.int32)
    d2 = np.where(idx >= 0, key, np.uint32(0x7FC00000)).astype(np.uint32).view(f32)
    return idx, d2


def gather(canon_v, canon_n, idx):
    """the clouds dfa_correspond writes: the canonical vertex / normal at idx — at idx == -1 (no neighbour at all) those of
    canonical point 0, as include/dynfu_amd.h states.  (vertices, normals or None)"""
    j = np.maximum(np.asarray(idx, np.int64), 0)
    v = np.ascontiguousarray(canon_v, f32).reshape(-1, 3)[j]
    return v, None if canon_n is None else np.ascontiguousarray(canon_n, f32).reshape(-1, 3)[j]


def want_grid(D, n_query):
    """csrc/capi_internal.hpp"""
    return D >= 64 and (D * n_query >= (1 << 22) or D >= 1024)


def search_form(n_canon, n_live):
    """the form dfa_correspond takes: "scan" | "node_grid" | "point_grid" | "point_grid_large" """
    if not want_grid(n_canon, n_live):
        return "scan"
    if n_canon >= 16384:
        return "point_grid_large" if n_canon > 500000 else "point_grid"
    return "node_grid"


# ------------------------------------------------------------------------------------------ the grids
# bmin float32 (3,), cs float32, dim (3,) int; the two candidates of the cell size: cs is the larger one
Geometry = namedtuple("Geometry", "bmin cs dim volume_term cap_term inv_cs")


def _geometry(points, aim, cap):
    p = np.ascontiguousarray(points, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        bmin, bmax = np.fmin.reduce(p, axis=0), np.fmax.reduce(p, axis=0)  # fminf / fmaxf: a NaN never wins
        ext = np.maximum(bmax - bmin, f32(0))
        volume = f32(aim) * np.cbrt((ext[0] * ext[1] * ext[2]) / f32(len(p)))
        cap_term = ext.max() / f32(cap)
        cs = max(volume, cap_term)
        if not cs > 0:
            cs = f32(1)
        inv_cs = f32(1) / cs
        dim = np.minimum(np.maximum((ext * inv_cs).astype(np.int32) + 1, 1), cap)
    return Geometry(bmin, f32(cs), dim, f32(volume), f32(cap_term), f32(inv_cs))


def node_grid_geometry(points):
    """grid_setup_kernel / grid_build_one_kernel: cs = max(cbrt(volume / n), longest extent / 32), at most 32 cells per axis"""
    return _geometry(points, 1.0, 32)


def point_grid_geometry(points):
    """pgrid_finalize_kernel: cs = max(0.7 cbrt(volume / n), longest extent / 128); above 500 000 points 0.5 and 256"""
    large = len(np.asarray(points).reshape(-1, 3)) > 500000
    return _geometry(points, 0.5 if large else 0.7, 256 if large else 128)


def grid_geometry(points, n_live):
    """the geometry of the grid dfa_correspond builds for this call (None for the exhaustive scan)"""
    form = search_form(len(np.asarray(points).reshape(-1, 3)), n_live)
    return None if form == "scan" else node_grid_geometry(points) if form == "node_grid" else point_grid_geometry(points)


def cell_coordinates(geo, q):
    """(cell int (n, 3), position in the cell float32 (n, 3)) of queries, as cell_of and knn_grid_query compute them:
    the cell is clamped into the grid, so a query outside has a position below 0 or above 1"""
    q = np.ascontiguousarray(q, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = (q - geo.bmin) * geo.inv_cs
        cell = np.clip(np.floor(np.where(np.isfinite(t), t, 0)), 0, geo.dim - 1).astype(np.int32)
        return cell, (t - cell.astype(f32)).astype(f32)


# ------------------------------------------------------------------------------------------ float32 fused multiply-add
def fma32(a, b, c):
    """fmaf(a, b, c), correctly rounded, for finite float32 arrays: the product of two float32 is exact in fp64; the fp64 sum
    is made with its exact error (TwoSum) and rounded to odd, after which the rounding to float32 is the rounding of the
    exact value (fp64 carries more than two extra bits)."""
    a, b, c = (np.asarray(x, f32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.uint64) & np.uint64(1)).astype(bool)
        nudge = np.isfinite(s) & (e != 0) & ~odd
        s = np.where(nudge, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def dot32(a, b):
    """dot of csrc/device_math.hpp: fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def _project(f, x, z, c):
    """fmaf(f, x / z, c), exactly (fma32) — and where the plainer evaluation, the fp64 sum of the exact product and c rounded
    to float32, would give another float32: that can happen only where the fp64 sum was itself rounded onto a float32 tie.
    The tests require that no vertex of their inputs is such a one, so either evaluation states them."""
    with np.errstate(all="ignore"):
        r = (x / z).astype(f32)
        n = len(r)
        u = fma32(np.full(n, f, f32), r, np.full(n, c, f32))
        plain = (np.float64(f) * r.astype(np.float64) + np.float64(c)).astype(f32)
        return u, u.view(np.uint32) != plain.view(np.uint32)


# ------------------------------------------------------------------------------------------ dfa_correspond_projective
def projective(vertices, normals, vmap, nmap, fx, fy, cx, cy, dist_thresh, min_cosine):
    """include/dynfu_amd.h, dfa_correspond_projective: every vertex with z > 0 is projected (u = fmaf(fx, x / z, cx), w
    likewise), accepted if 0 <= u < cols and 0 <= w < rows, point-sampled at floor; rejected if the map vertex's x is NaN,
    if the float32 squared distance (dot32) exceeds the float32 dist_thresh * dist_thresh, with a normal map if the map
    normal's x is NaN, and with vertex normals as well if |n . n'| < min_cosine.  Rejected entries: NaN vertex, NaN normal,
    pixel -1.  vmap / nmap: (rows, cols, 4) float32 (any row pitch).
    Returns (v (n, 3), n (n, 3) or None, pixel int32 (n,), mask (n,)): the mask marks vertices in front of the camera whose
    u or w differs between fmaf and the fp64-then-float32 evaluation (see _project)."""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    rows, cols = vmap.shape[:2]
    fx, fy, cx, cy, dist_thresh, min_cosine = (f32(t) for t in (fx, fy, cx, cy, dist_thresh, min_cosine))
    qnan = np.uint32(0x7FC00000).view(f32)
    with np.errstate(all="ignore"):
        front = v[:, 2] > 0
        u, tu = _project(fx, v[:, 0], v[:, 2], cx)
        w, tw = _project(fy, v[:, 1], v[:, 2], cy)
        inside = front & (u >= 0) & (w >= 0) & (u < f32(cols)) & (w < f32(rows))
        iu = np.where(inside, np.floor(u), 0).astype(np.int64)
        iw = np.where(inside, np.floor(w), 0).astype(np.int64)
        mv = np.asarray(vmap, f32)[iw, iu]
        ok = inside & ~np.isnan(mv[:, 0])
        sd = v - mv[:, :3]
        ok &= ~(dot32(sd, sd) > dist_thresh * dist_thresh)
        mn = None
        if nmap is not None:
            mn = np.asarray(nmap, f32)[iw, iu][:, :3]
            ok &= ~np.isnan(mn[:, 0])
            if normals is not None:
                ok &= ~(np.abs(dot32(np.asarray(normals, f32).reshape(-1, 3), mn)) < min_cosine)
    out_v = np.where(ok[:, None], mv[:, :3], qnan).astype(f32)
    out_n = None if mn is None else np.where(ok[:, None], mn, qnan).astype(f32)
    pixel = np.where(ok, iw * cols + iu, -1).astype(np.int32)
    return out_v, out_n, pixel, (tu | tw) & front
