"""CPU statement of dfa_visible_vertices (include/dynfu_amd.h) in numpy float32, written from its contract.

One vertex (x, y, z) in the camera frame against a float4 point map M of the model's visible surface (quiet NaN where nothing
is seen).  Every operation is a float32 operation, rounded on its own, in this order:
  1. x, y or z not finite, or z <= 0:                                   flag 0
  2. qx = x / z, qy = y / z                                              correctly rounded divisions
  3. u = fma(fx, qx, cx), v = fma(fy, qy, cy)                            one rounding each (extract_statement.fma32)
  4. ru = rint(u), rv = rint(v), ties to even; unless 0 <= ru <= cols - 1 and 0 <= rv <= rows - 1, compared as floats:
                                                                         flag 0
  5. M = map[rv][ru]; M.x is NaN:                                        flag 1 (nothing of the model covers the pixel)
  6. otherwise                                                           flag = z <= M.z + z_tol (one addition, one comparison)
The count is the number of set flags."""
import numpy as np

from extract_statement import fma32

f32 = np.float32


def visible_vertices(vertices, model_points, fx, fy, cx, cy, z_tol):
    """vertices (N, 3) or (N, 4) float32, model_points (rows, cols, 4) float32 -> (flags (N,) uint8, count)"""
    V = np.asarray(vertices, np.float32)
    M = np.asarray(model_points, np.float32)
    assert V.ndim == 2 and V.shape[1] in (3, 4) and M.ndim == 3 and M.shape[2] == 4
    rows, cols = M.shape[:2]
    x, y, z = V[:, 0], V[:, 1], V[:, 2]
    flags = np.zeros(len(V), np.uint8)
    with np.errstate(all="ignore"):
        alive = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (z > 0)                      # 1.
        zs = np.where(alive, z, f32(1))
        qx, qy = (x / zs).astype(np.float32), (y / zs).astype(np.float32)                       # 2.
        u, v = fma32(f32(fx), qx, f32(cx)), fma32(f32(fy), qy, f32(cy))                         # 3.
        ru, rv = np.rint(u).astype(np.float32), np.rint(v).astype(np.float32)                   # 4. (numpy rounds half to even)
        inside = alive & (ru >= 0) & (ru <= f32(cols - 1)) & (rv >= 0) & (rv <= f32(rows - 1))
        i, j = np.where(inside, ru, 0).astype(np.int64), np.where(inside, rv, 0).astype(np.int64)
        m = M[j, i]
        free = np.isnan(m[:, 0])                                                                # 5.
        front = z <= (m[:, 2] + f32(z_tol)).astype(np.float32)                                  # 6.
    flags[inside & (free | front)] = 1
    return flags, int(flags.sum())
