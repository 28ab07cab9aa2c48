"""The cases of the dfa_color_sample tests, shared by the CPU statement tests and the -m gpu tests.  Colour volumes: the
statement's outputs of two fusion cases (tests/tsdf_color_cases.py) — "padded" ((9, 7, 14), a junk start: nearly every word
has a weight) and "main_volume_skip" ((32, 32, 32), an empty start: colour in the truncation band only, so den runs through
every value between 0 and 1).  Vertices: about 2 000 seeded random points in and around the volume, the lattice-edge
vertices of mc_indexed_statement on the same case's fused TSDF volume, points far outside, non-finite points; each both in the
volume's frame (to_volume None) and in a posed frame (to_volume a rotation of 0.4 rad plus a translation).  N = 0 is a case of
the tests themselves."""
import functools

import numpy as np

import color_sample_statement as CS
import mc_indexed_statement as MI
import tsdf_color_cases as CC
import tsdf_warped6_cases as C6
import tsdf_warped6_statement as W6

CASES = {  # name: (fusion case, posed)
    "small": ("padded", False), "small_posed": ("padded", True),
    "main": ("main_volume_skip", False), "main_posed": ("main_volume_skip", True),
}
# delta per case: the largest float32 deviation of g in cells, measured by color_sample_statement.deviation on the case's
# inputs (tests/test_color_sample_statement_cpu.py measures it again on every run)
# "main": 0 — its voxel size is 2^-5 and it has no frame, so the one division is exact
DELTA = {"small": 4.8e-7, "small_posed": 1.3e-6, "main": 0.0, "main_posed": 3.8e-6}  # measured 4.766e-07, 1.273e-06, 0, 3.782e-06


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: colors (uint32 (Z, Y, X)), voxel_size, vertices ((N, 4) float32, the 4th float junk), to_volume (12 float32 or None),
    delta, ref (the statement's answer).  Read-only."""
    fusion, posed = CASES[name]
    c = CC.case(fusion)
    colors = c["cref"]["colors"]
    Z, Y, X = colors.shape
    vs = np.asarray(c["voxel_size"], np.float32)
    rng = np.random.default_rng(900 + sorted(CASES).index(name))
    dims = np.array([X, Y, Z], np.float64)
    rand = rng.uniform(-1.5, dims + 0.5, (2000, 3)) * vs
    on_lattice = np.floor(rng.uniform(0, dims, (40, 3))) * vs  # f = 0 exactly: one corner has all the weight
    keys = np.flatnonzero(MI.vertex_edges(c["ref"]["vol"]).ravel())
    mesh = MI.positions(c["ref"]["vol"], vs, keys)[:, :3].astype(np.float64)
    far = np.array([[-50.0, 0.1, 0.1], [0.1, 1e6, 0.1], [0.1, 0.1, -3e9], [1e30, 1e30, 1e30], [3e38, 0.0, 0.0]])
    pts = np.concatenate([rand, on_lattice, mesh, far])
    to_volume = C6.rigid([0.2, 0.9, -0.4], 0.4, [0.31, -0.12, 0.57]) if posed else None
    if posed:
        pts = W6.apply64(W6.invert(to_volume), pts)
    with np.errstate(over="ignore"):
        verts = np.concatenate([pts.astype(np.float32), rng.standard_normal((len(pts), 1)).astype(np.float32)], 1)
    bad = np.array([[np.nan, 0.1, 0.1, 1], [0.1, np.inf, 0.1, 1], [0.1, 0.1, -np.inf, 1], [np.nan, np.nan, np.nan, np.nan]], np.float32)
    verts = np.ascontiguousarray(np.concatenate([verts, bad]))
    ref = CS.sample(colors, vs, verts, to_volume, DELTA[name])
    for a in (verts, *ref.values()):
        a.setflags(write=False)
    return dict(name=name, colors=colors, voxel_size=vs, vertices=verts, to_volume=to_volume, delta=DELTA[name], ref=ref,
                n_mesh=len(mesh), n_bad=len(bad))
