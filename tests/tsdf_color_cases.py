"""The cases of the colour-fusion tests (dfa_tsdf_integrate_warped6_color), shared by the CPU statement tests and the -m gpu
tests: all twelve of tsdf_warped6_cases.CASES — volumes (32, 32, 32), (50, 38, 44), (9, 7, 14) and (1, 2, 12), an 80 x 60
frame — with, per case, a seeded random b, g, r, x image, an "empty" or a "junk" starting colour volume and max_color_weight
(255; 3 on one case with a junk start, so that the cap binds).  Junk: random words with the weights 0 (channels non-zero:
not "no colour" by its bits, yet weight 0), 1, 254 and 255 planted.  "antipodal" takes the image and the colours of its twin:
the statement's colour volume must be the same, exactly."""
import functools

import numpy as np

import tsdf_color_statement as CST
import tsdf_warped6_cases as C6

#        name                      colours  max_color_weight
COLOR = {
    "main_volume_skip":       ("empty", 255),
    "main_posed_rigid_junk":  ("junk",  255),
    "odd_scan_moved":         ("junk",    3),
    "odd_grid_rigid_posed":   ("empty", 255),
    "big_moved":              ("junk",  255),
    "padded":                 ("junk",  255),
    "thin":                   ("junk",  255),
    "thin_padded":            ("empty", 255),
    "no_nodes_skip":          ("junk",  255),
    "no_nodes_rigid":         ("empty", 255),
    "antipodal":              ("junk",  255),
    "tiny_k3_grid_moved":     ("junk",  255),
}
CAP_CASE = "odd_scan_moved"
SMALL = ("padded", "thin", "thin_padded", "no_nodes_skip", "tiny_k3_grid_moved")  # the volumes a scalar loop walks
assert set(COLOR) == set(C6.CASES)


def start_colors(dims, start, seed):
    X, Y, Z = dims
    if start == "empty":
        return np.zeros((Z, Y, X), np.uint32)
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, (Z, Y, X), dtype=np.uint64).astype(np.uint32)
    planted = rng.choice(np.array([0, 1, 254, 255], np.uint32), (Z, Y, X))
    plant = rng.random((Z, Y, X)) < 0.5
    words = np.where(plant, (words & np.uint32(0x00ffffff)) | (planted << 24), words).astype(np.uint32)
    zero_w = (words >> 24) == 0
    return np.where(zero_w & ((words & 0xffffff) == 0), np.uint32(0x00010203), words).astype(np.uint32)  # (weight 0, channels non-zero)


@functools.lru_cache(maxsize=None)
def case(name):
    """tsdf_warped6_cases.case(name) with image, colors, max_color_weight and cref: the colour statement's answer (colors after
    one call, colors2 after two, coloured, decided, updated, px, py, tsdf).  Computed once per process; read-only."""
    c = C6.case(name)
    start, cap = COLOR[name]
    seed = sorted(C6.CASES).index(C6.ANTIPODAL_OF.get(name, name))
    rng = np.random.default_rng(700 + seed)
    rows, cols = c["dists"].shape
    image = rng.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    colors = start_colors(c["dims"], start, 800 + seed)
    cref = CST.integrate(colors, image, c["dists"], c["voxel_size"], c["trunc"], cap, c["vol2node"], c["node2cam"], *c["intr"],
                         c["nodes"], c["node_dq"], c["node_w"], c["k"], c["mode"])
    cref["colors2"] = CST.apply(cref["colors"], image, cref, cap)[0]
    for a in (image, colors, *cref.values()):
        a.setflags(write=False)
    return dict(c, image=image, colors=colors, max_color_weight=cap, cref=cref)
