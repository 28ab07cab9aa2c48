"""The cases tests/test_visibility_statement_cpu.py and tests/test_gpu_visibility.py share (dfa_visible_vertices).

two_planes   a 64 x 48 image; a near quad at z = 1.0 over the left 40 columns (two triangles; its corners project a quarter
             pixel outside the centres of columns 0 / 39 and rows 0 / 47, so it covers exactly those and its own vertices land
             inside it), rasterised by raster_statement.rasterize32 on the CPU or dfa_mesh_rasterize on the GPU.  The cloud:
             1 031 points on the plane z = 1.5 all over the image (not a multiple of 64 or 256; none within 0.05 pixel of the
             quad's edge column boundary u = 39.5), then the quad's own four vertices.  Expected: behind the quad 0, beside it 1,
             the quad's vertices 1.
edge_values  hand-made vertices against a hand-made 8 x 6 map, fx = fy = 4, cx = 3, cy = 2, z_tol = 0.25 — powers of two, so
             that every projection below is exact — with the answers worked by hand beside each vertex.
"""
import numpy as np

f32 = np.float32
NAN = f32(np.nan)


# ------------------------------------------------------------------------------------------------------------ two_planes
TP = dict(cols=64, rows=48, intr=(60.0, 60.0, 31.5, 23.5), z_tol=0.01, z_near=0.1, n_plane=1031, quad_cols=40)


def two_planes_quad():
    """the near quad: (vertices (4, 4) float32 with w = 1, indices (6,) int32)"""
    fx, fy, cx, cy = TP["intr"]
    u0, u1, v0, v1 = -0.25, TP["quad_cols"] - 0.75, -0.25, TP["rows"] - 0.75
    xy = [((u - cx) / fx, (v - cy) / fy) for u, v in ((u0, v0), (u1, v0), (u1, v1), (u0, v1))]
    verts = np.array([[x, y, 1.0, 1.0] for x, y in xy], np.float32)
    return verts, np.array([0, 1, 2, 0, 2, 3], np.int32)


def two_planes_cloud():
    """-> (vertices (1 035, 3) float32, expected flags (1 035,) uint8)"""
    fx, fy, cx, cy = TP["intr"]
    rng = np.random.default_rng(7)
    n = TP["n_plane"]
    u = rng.uniform(-0.4, TP["cols"] - 0.6, n)
    v = rng.uniform(-0.4, TP["rows"] - 0.6, n)
    edge = TP["quad_cols"] - 0.5
    u = np.where(np.abs(u - edge) < 0.05, u + 0.1, u)  # (the expected answer is geometry, not a rounding)
    z = 1.5
    plane = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, np.full(n, z)], 1).astype(np.float32)
    quad, _ = two_planes_quad()
    verts = np.concatenate([plane, quad[:, :3]]).astype(np.float32)
    expected = np.concatenate([(u > edge).astype(np.uint8), np.ones(4, np.uint8)])
    return verts, expected


# ------------------------------------------------------------------------------------------------------------ edge_values
EV = dict(cols=8, rows=6, intr=(4.0, 4.0, 3.0, 2.0), z_tol=0.25, pad=3)
THIRD = f32(1.0) / f32(3.0)
T = f32(THIRD + f32(0.25))  # the threshold under pixel (5, 4): one float32 addition, which rounds


def edge_values_map():
    """(rows, cols + pad, 4) float32 storage whose first `cols` columns are the map; the padding holds finite points at
    z = 0 that would hide everything, had they been read"""
    store = np.zeros((EV["rows"], EV["cols"] + EV["pad"], 4), np.float32)
    m = store[:, :EV["cols"]]
    m[...] = NAN
    for (r, c), z in {(2, 0): 0.5, (2, 2): 0.25, (2, 3): 2.0, (2, 4): 0.25, (1, 3): 0.25, (3, 3): 0.25, (4, 5): THIRD}.items():
        m[r, c] = (0.0, 0.0, z, 0.0)
    m[1, 6] = (NAN, 0.0, 0.1, 0.0)  # x is NaN: a miss, whatever z says
    m[0, 6] = (0.0, 0.0, NAN, 0.0)  # a hit without a depth: the comparison with NaN fails
    return store


def _up(x):
    return np.nextafter(f32(x), f32(np.inf))


def _down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def edge_values_vertices():
    """-> (vertices (N, 3) float32, expected (N,) uint8); u = 4 x / z + 3, v = 4 y / z + 2"""
    inf = f32(np.inf)
    rows = [
        ((0, 0, 0), 0),                      # z == 0
        ((0, 0, -1), 0),                     # z < 0
        ((NAN, 0, 1), 0), ((0, NAN, 1), 0), ((0, 0, NAN), 0),
        ((inf, 0, 1), 0), ((0, -inf, 1), 0), ((0, 0, inf), 0),
        ((-0.875, 0, 1), 0),                 # u = -0.5 -> rint = -0: column 0, whose point at z = 0.5 hides z = 1
        ((-0.4375, 0, 0.5), 1),              # u = -0.5 again, z = 0.5 <= 0.5 + 0.25
        ((_down(-0.4375), 0, 0.5), 0),       # u one ulp below -0.5 -> -1: outside
        ((1.125, 0, 1), 0),                  # u = 7.5 = cols - 0.5 -> 8 (even): outside
        ((_down(1.125), 0, 1), 1),           # u just below 7.5 -> 7: pixel (7, 2) is a miss
        ((-0.125, 0, 1), 0),                 # u = 2.5 -> 2 (even; half-up would say 3): pixel (2, 2) at z = 0.25 hides
        ((0.125, 0, 1), 0),                  # u = 3.5 -> 4 (even; half-down would say 3): pixel (4, 2) at z = 0.25 hides
        ((0, 0.125, 1), 1),                  # v = 2.5 -> 2: pixel (3, 2) at z = 2 (row 3 would hide)
        ((0, -0.125, 1), 1),                 # v = 1.5 -> 2 (row 1 would hide)
        ((0, 0, 2.25), 1),                   # z == M.z + z_tol exactly
        ((0, 0, _up(2.25)), 0),              # one ulp behind it
        ((0, 0, _down(2.25)), 1),            # one ulp in front
        ((f32(0.5) * T, f32(0.5) * T, T), 1),                        # pixel (5, 4): z == fl(1/3 + 0.25)
        ((f32(0.5) * _up(T), f32(0.5) * _up(T), _up(T)), 0),
        ((f32(0.5) * _down(T), f32(0.5) * _down(T), _down(T)), 1),
        ((0.75, -0.25, 1), 1),               # pixel (6, 1): M.x is NaN, M.z = 0.1 is not looked at
        ((0.75, -0.5, 1), 0),                # pixel (6, 0): M.x finite, M.z NaN
        ((0, -0.625, 1), 1),                 # v = -0.5 -> -0: row 0, a miss
        ((0, 0.875, 1), 0),                  # v = 5.5 = rows - 0.5 -> 6 (even): outside
        ((0, _down(0.875), 1), 0),           # y one ulp below: 4 y + 2 lies halfway between two floats and the fma rounds it
                                             # to the even one, 5.5 again -> 6: outside
        ((0, _down(_down(0.875)), 1), 1),    # two ulps below: v = 5.5 - 2^-21 -> 5: a miss
        ((100, 0, 1), 0),                    # far outside
        ((3e38, 0, 1e-30), 0),               # x / z overflows: u = inf fails the comparison
    ]
    return np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.uint8)


def edge_values_variants():
    """(name, vertices (N, 3 or 4), expected): stride 3 and 4 (the fourth float is never looked at), N = 0, N = 1"""
    v, e = edge_values_vertices()
    v4 = np.concatenate([v, np.full((len(v), 1), NAN, np.float32)], 1)
    one = 17  # z == M.z + z_tol exactly
    return [("stride 3", v, e), ("stride 4", v4, e), ("N = 0", v[:0], e[:0]), ("N = 1", v[one:one + 1], e[one:one + 1]),
            ("N = 1, stride 4", v4[one:one + 1], e[one:one + 1])]
