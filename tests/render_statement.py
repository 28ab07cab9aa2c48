"""CPU statement of the render kernels (src/kfusion/cuda/imgproc.cu:363-514) in numpy float32: the Phong view of a point
map (:413-461) and of a depth map (:363-411), and the normal colours (:485-504, the `#else` branch).

Written from the reference's source, as tests/tsdf_statement.py and tests/img_statement.py are, in the same arithmetic
convention: every operation a float32 operation in the source's order, a multiply-add fused only inside dot().  The
three CUDA intrinsics of these kernels have no portable definition; the project fixes them as IEEE sequences
(dynfu_amd/csrc/render.hip states the same list) so that the image is reproducible byte for byte:
  - __powf(x, 20.f): five multiplications, x2 = x x, x4 = x2 x2, x5 = x4 x, x10 = x5 x5, x20 = x10 x10;
  - normalized: tsdf_statement.normalized, v * (1 / sqrt(dot(v, v)));
  - uchar(__saturatef(c) * 255.f): NaN -> 0, clamp to [0, 1], multiply, truncate;
  - the normal colours' uchar((5 - n k) * 25.5f) has no clamp in the reference and is undefined for NaN and outside
    [0, 256): NaN -> 0, else clamp to [0, 255], truncate;
  - fmax(0.f, d) returns 0 for a NaN d (numpy's fmax).
A pixel is the reference's RGB (types.hpp): the bytes b, g, r, 0.  Images are returned as (rows, cols, 4) uint8.

The view of a volume from a pose (KinFu::renderImage(image, pose, flag), kinfu.cpp:289-316) is
tsdf_statement.raycast_points followed by this module: raycast_render below.
"""
import numpy as np

from tsdf_statement import QNAN, dot, normalized  # noqa: F401  (QNAN: what a raycast miss holds)

f32 = np.float32
PHONG, NORMALS, BOTH = 0, 1, 2  # dfa_tsdf_raycast_render's mode
BGR1 = [f32(4) / f32(255), f32(2) / f32(255), f32(2) / f32(255)]  # :376 / :426
BGR2 = [f32(236) / f32(255), f32(120) / f32(255), f32(120) / f32(255)]  # :377 / :427


def unit_to_byte(c):
    """static_cast<unsigned char>(__saturatef(c) * 255.f) (:406-408)"""
    c = np.asarray(c, np.float32)
    s = np.where(c > 0, np.where(c < 1, c, f32(1)), f32(0)).astype(np.float32)  # NaN -> 0
    return np.trunc(s * f32(255)).astype(np.uint8)


def clamp_to_byte(v):
    """the project's definition of static_cast<unsigned char>(v) (:499-501)"""
    v = np.asarray(v, np.float32)
    return np.trunc(np.where(v > 0, np.where(v < 255, v, f32(255)), f32(0))).astype(np.uint8)


def pow20(x):
    x2 = x * x
    x4 = x2 * x2
    x5 = x4 * x
    x10 = x5 * x5
    return (x10 * x10).astype(np.float32)


def specular(P, N, light):
    """max(0, R . V) of :397-401 — the base of the specular power, for the tests' input conditions"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L = normalized([f32(light[k]) - P[k] for k in range(3)])
        V = normalized([f32(0) - P[k] for k in range(3)])
        nl = dot(N, L)
        R = normalized([(f32(2) * N[k]) * nl - L[k] for k in range(3)])
        return np.fmax(f32(0), dot(R, V)).astype(np.float32), nl


def phong(P, N, light):
    """Ix of :397-401 for points P and normals N (3 arrays each)"""
    rv, nl = specular(P, N, light)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((f32(0.3) + f32(0.5) * np.fmax(f32(0), nl)) + f32(0.2) * pow20(rv)).astype(np.float32)


def _shade(miss, P, N, light):
    rows, cols = miss.shape
    img = np.zeros((rows, cols, 4), np.uint8)
    w = (np.arange(rows, dtype=np.float32) / f32(rows))[:, None] * np.ones((1, cols), np.float32)  # :379 / :429
    Ix = unit_to_byte(phong(P, N, light))
    for c in range(3):
        img[..., c] = np.where(miss, unit_to_byte(BGR1[c] * (f32(1) - w) + BGR2[c] * w), Ix)  # :380 / :430
    return img


def render_image_points(points, normals, light):
    """:413-461.  points, normals: (rows, cols, 4) float32"""
    P = np.asarray(points, np.float32)
    N = np.asarray(normals, np.float32)
    return _shade(np.isnan(P[..., 0]), [P[..., k] for k in range(3)], [N[..., k] for k in range(3)], light)


def render_image_depth(depth, normals, fx, fy, cx, cy, light):
    """:363-411.  depth: (rows, cols) uint16 millimetres"""
    d = np.asarray(depth, np.uint16)
    N = np.asarray(normals, np.float32)
    rows, cols = d.shape
    finvx, finvy = f32(1) / f32(fx), f32(1) / f32(fy)
    z = d.astype(np.float32) * f32(0.001)  # :382
    u = np.arange(cols, dtype=np.float32)[None, :]
    v = np.arange(rows, dtype=np.float32)[:, None]
    P = [(z * (u - f32(cx))) * finvx, (z * (v - f32(cy))) * finvy, z]  # Reprojector, device.hpp:50-54
    return _shade(d == 0, P, [N[..., k] for k in range(3)], light)


def render_tangent_colors(normals):
    """:485-504"""
    N = np.asarray(normals, np.float32)
    img = np.zeros(N.shape[:2] + (4,), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        img[..., 2] = clamp_to_byte((f32(5) - N[..., 0] * f32(3.5)) * f32(25.5))  # r
        img[..., 1] = clamp_to_byte((f32(5) - N[..., 1] * f32(2.5)) * f32(25.5))  # g
        img[..., 0] = clamp_to_byte((f32(5) - N[..., 2] * f32(3.5)) * f32(25.5))  # b
    return img


def render_maps(points, normals, light, mode):
    """kinfu.cpp:304-315 on given maps: Phong, normal colours, or both side by side"""
    if mode == PHONG:
        return render_image_points(points, normals, light)
    if mode == NORMALS:
        return render_tangent_colors(normals)
    return np.concatenate([render_image_points(points, normals, light), render_tangent_colors(normals)], axis=1)


def raycast_render(vol, voxel_size, trunc, cam2vol, Rinv, fx, fy, cx, cy, step_factor, delta_factor, cols, rows, light, mode):
    import tsdf_statement as S
    P, N = S.raycast_points(vol, voxel_size, trunc, cam2vol, Rinv, fx, fy, cx, cy, step_factor, delta_factor, cols, rows)
    return render_maps(P, N, light, mode)
