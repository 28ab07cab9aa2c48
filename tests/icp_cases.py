"""The shape cases of the rigid-ICP sums, shared by tests/test_img_statement_cpu.py (which measures the constant of the
per-sum bar over them and checks that none has a knife-edge pixel) and tests/test_gpu_icp.py (which runs the kernel on
them).  Inputs are the statement's own maps (tests/img_statement.py) of the synthetic frames 0 (previous) and 4
(current); a ragged size is a crop of the T1 maps with cx, cy shifted by the crop's origin.

Sizes are (cols, rows).  The launch tile of icp.hip is 32 x 8 pixels, four waves of 64."""
import functools

import numpy as np

import img_statement as St
from dynfu_amd import synth
from gpu_util_cpu import rot

# The constant c of the per-sum bar, measured by tests/test_img_statement_cpu.py (see its docstring): one over the nine
# sizes of the shape matrix, and one of its own for the nearly converged wall crop, where d - s cancels four digits
# that the scale abs64 of a b sum does not see.
C_BAR = 2048
C_BAR_CONVERGED = 65536
CONVERGED_CASES = ("37x53-wall",)

NEAR = ([0.2, 1.0, 0.1], 0.01, [0.004, -0.003, 0.006])
FAR = ([1.0, 0.0, 0.3], 0.04, [-0.02, 0.01, 0.03])
MID = ([1.0, 0.0, 0.3], 0.008, [-0.004, 0.002, 0.006])      # FAR moves a pixel by ten rows: too far for the images of 7 to 9 rows
TINY = ([0.2, 1.0, 0.1], 5e-4, [0.0002, 0.0003, 0.001])      # a fraction of a pixel: what a single row can still match
TINY2 = ([1.0, 0.3, 0.0], -3e-4, [-0.0001, 0.0002, 0.002])  # (both move the row down, into the image)
CONVERGED = ([0.3, 1.0, -0.2], 1e-4, [8e-5, -6e-5, 1e-4])   # a level's last iterations: residuals of a tenth of a millimetre

# name: (cols, rows), source, crop origin (x0, y0) or None, poses, least matched fraction (of the better pose)
CASES = {
    "1x1": ((1, 1), "T1", (170, 130), (TINY, TINY2), 0.0),
    "1x64": ((64, 1), "T1", (120, 110), (TINY, TINY2), 0.0),            # one row, one full wave wide
    "37x53": ((53, 37), "T1", (100, 60), (NEAR, FAR), 0.3),           # 37 rows of 53 pixels
    "8x130": ((130, 8), "T1", (40, 100), (NEAR, MID), 0.3),           # 8 rows of 130 pixels: one tile row, 4 full tiles + 2 columns
    "80x60": ((80, 60), "T1/4", None, (NEAR, FAR), 0.3),              # T1 at pyramid level 2
    "33x9": ((33, 9), "T1", (140, 100), (NEAR, MID), 0.3),            # one column and one row past a tile
    "31x7": ((31, 7), "T1", (140, 100), (NEAR, MID), 0.3),            # one column and one row short of a tile
    "640x480": ((640, 480), "C2", None, (NEAR, FAR), 0.3),
    "1280x720": ((1280, 720), "C4", None, (NEAR, FAR), 0.3),
    "37x53-wall": ((53, 37), "T1", (8, 8), (CONVERGED,), 0.3),        # the wall beside the sphere, nearly aligned
}
VARIANTS = ("depth", "points")


def affine(pose):
    axis, ang, t = pose
    return np.concatenate([rot(axis, ang).astype(np.float32).reshape(-1), np.array(t, np.float32)])


@functools.lru_cache(maxsize=None)
def _maps(source, variant):
    """((curr, ncurr, prev, nprev), level intrinsics) of a whole synthetic frame pair"""
    name, _, div = source.partition("/")
    cfg = synth.CONFIGS[name]
    intr = synth.intrinsics(cfg)
    d0, d1 = synth.depth_frame(cfg, 0), synth.depth_frame(cfg, 4)
    if not div:
        f = St.normals_mask_depth if variant == "depth" else St.points_normals
        (a0, n0), (a1, n1) = f(d0, *intr), f(d1, *intr)
        return (a1, n1, a0, n0), intr
    li = tuple(v / 4 for v in intr)  # setLevelIntr at level 2
    if variant == "depth":  # the pyramid: two halvings of the depth, then the level's own normals (kinfu.cpp:150-167)
        d0, d1 = (St.depth_pyr(St.depth_pyr(d, 0.04), 0.04) for d in (d0, d1))
        (a0, n0), (a1, n1) = St.normals_mask_depth(d0, *li), St.normals_mask_depth(d1, *li)
    else:  # the resizers: level 0 maps halved twice
        (a0, n0), (a1, n1) = St.points_normals(d0, *intr), St.points_normals(d1, *intr)
        for _ in range(2):
            (a0, n0), (a1, n1) = St.resize_points_normals(a0, n0), St.resize_points_normals(a1, n1)
    return (a1, n1, a0, n0), li


def inputs(name, variant):
    """-> ((curr, ncurr, prev, nprev) contiguous arrays of the case's size, (fx, fy, cx, cy))"""
    (cols, rows), source, origin, _, _ = CASES[name]
    maps, (fx, fy, cx, cy) = _maps(source, variant)
    if origin is None:
        assert maps[0].shape[:2] == (rows, cols)
        return maps, (fx, fy, cx, cy)
    x0, y0 = origin
    return tuple(np.ascontiguousarray(m[y0:y0 + rows, x0:x0 + cols]) for m in maps), (fx, fy, cx - x0, cy - y0)


def poses(name):
    return CASES[name][3]


def c_of(name):
    return C_BAR_CONVERGED if name in CONVERGED_CASES else C_BAR


def within_bar(got, sum64, abs64, c=C_BAR):
    """the per-sum bar |got[q] - sum64[q]| <= c 2^-24 abs64[q], for every q; a NaN only where the statement has one"""
    got, sum64, abs64 = (np.asarray(v, np.float64) for v in (got, sum64, abs64))
    nan = np.isnan(sum64)
    return bool(np.array_equal(np.isnan(got), nan) and (np.abs(got - sum64)[~nan] <= c * 2.0 ** -24 * abs64[~nan]).all())


# ------------------------------------------------------------------------------------- whole iterations ----
SCHEDULE = (10, 5, 4)                      # KinFu's default iterations per level, level 0 = full resolution
GATES = dict(dist_thres=0.1, angle_thres=30.0 * 0.017453293)  # kinfu.cpp:31-32
MOTION_ANGLE, MOTION_T = 0.021, (0.015, -0.008, 0.010)  # the current camera: 1.2 degrees about y, (15, -8, 10) mm


def motion():
    """X_prev = R X_cur + t, what the estimate has to recover (tests/cpp/test_host_icp.cpp)"""
    c, s = np.cos(MOTION_ANGLE), np.sin(MOTION_ANGLE)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), np.array(MOTION_T)


def render(W, H, f, R, t):
    """u16 depth of two spheres in front of a tilted wall seen from the camera pose X_world = R X_cam + t: the scene of
    tests/cpp/test_host_icp.cpp (roll about the optical axis is observable), in float64"""
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dw = np.stack([(x - cx) / f, (y - cy) / f, np.ones_like(x)], -1) @ np.asarray(R, np.float64).T
    t = np.asarray(t, np.float64)
    best = np.full((H, W), 1e9)
    for C, rad in (((0.25, -0.1, 1.6), 0.45), ((-0.55, 0.3, 2.0), 0.3)):
        oc = t - np.array(C)
        a, b, c = (dw * dw).sum(-1), 2 * (dw @ oc), oc @ oc - rad * rad
        disc = b * b - 4 * a * c
        s = (-b - np.sqrt(np.where(disc > 0, disc, 0))) / (2 * a)
        best = np.where((disc > 0) & (s > 0) & (s < best), s, best)
    pn, pd = np.array([0.3, 0.2, -0.933]), -2.6 * 0.933
    den = dw @ pn
    s = (pd - pn @ t) / np.where(np.abs(den) > 1e-6, den, 1.0)
    best = np.where((np.abs(den) > 1e-6) & (s > 0) & (s < best), s, best)
    d = np.where(best < 60.0, np.rint(best * 1000.0), 0).astype(np.uint16)
    d[:3], d[-3:], d[:, :3], d[:, -3:] = 0, 0, 0, 0
    return d


@functools.lru_cache(maxsize=None)
def pyramids(config, variant):
    """per level (curr, ncurr, prev, nprev) and intrinsics, built as KinFu::operator() does (kinfu.cpp:150-167):
    bilateral filter, depth pyramid, the level's own maps; previous camera at the origin, current one moved by motion()"""
    cfg = synth.CONFIGS[config]
    intr = synth.intrinsics(cfg)
    R, t = motion()
    f = St.normals_mask_depth if variant == "depth" else St.points_normals
    per_frame = []
    for Rc, tc in ((R, t), (np.eye(3), np.zeros(3))):
        d = St.bilateral(render(cfg["width"], cfg["height"], cfg["focal"], Rc, tc), 7, 4.5, 0.04)
        levels = []
        for lv in range(len(SCHEDULE)):
            levels.append(f(d, *(v / (1 << lv) for v in intr)))
            d = St.depth_pyr(d, 0.04)
        per_frame.append(levels)
    return [(per_frame[0][lv] + per_frame[1][lv], tuple(v / (1 << lv) for v in intr)) for lv in range(len(SCHEDULE))]


def iterate(config, variant, sums_at, observe=None):
    """the coarse-to-fine loop of ProjectiveICP::estimateTransform from the identity: sums_at(args, li, aff12) -> 27 sums,
    St.icp_update after each; observe(level, iteration, args, li, aff12 before).  -> [(level, aff12 after)], one per iteration"""
    pyr = pyramids(config, variant)
    aff = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
    out = []
    for lv in range(len(SCHEDULE) - 1, -1, -1):
        args, li = pyr[lv]
        for it in range(SCHEDULE[lv]):
            if observe:
                observe(lv, it, args, li, aff)
            ok, aff = St.icp_update(sums_at(args, li, aff), aff)
            assert ok, (lv, it)
            out.append((lv, aff))
    return out


def sums32(args, li, aff):
    """the float32 statement's sums as the kernel delivers them: rounded to float32"""
    return St.icp(*args, aff, li, **GATES)[0].astype(np.float32)


def sums64(args, li, aff):
    return St.icp64(*args, aff, li, **GATES)[3]


def level_gaps(a, b):
    """largest |pose entry difference| between two trajectories, per level"""
    gaps = [0.0] * len(SCHEDULE)
    for (lv, x), (_, y) in zip(a, b):
        gaps[lv] = max(gaps[lv], float(np.abs(x.astype(np.float64) - y).max()))
    return gaps


def pose_bar(gap):
    """4 times the measured gap, rounded up to two significant digits"""
    e = 10.0 ** (np.floor(np.log10(4 * gap)) - 1)
    return float(np.ceil(4 * gap / e - 1e-9) * e)


# The pose bar of the GPU-driven trajectory, per (configuration, variant) and level 0, 1, 2: 4 times the largest pose-entry
# difference between the float32-statement-driven and the fp64-driven trajectories, as tests/test_img_statement_cpu.py
# measures it (gaps 1.29e-5, 2.13e-5, 8.38e-8 / 9.59e-8, 1.02e-7, 8.87e-8 / 7.82e-7, 4.48e-7, 2.51e-8 / 3.54e-7,
# 7.36e-8, 4.56e-8 in the order below), rounded up to two digits.
POSE_BARS = {
    ("T1", "depth"): (5.2e-05, 8.6e-05, 3.4e-07),
    ("T1", "points"): (3.9e-07, 4.1e-07, 3.6e-07),
    ("C2", "depth"): (3.2e-06, 1.8e-06, 1.1e-07),
    ("C2", "points"): (1.5e-06, 3.0e-07, 1.9e-07),
}
