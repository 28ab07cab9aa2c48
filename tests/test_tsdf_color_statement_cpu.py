"""CPU checks of the colour-fusion statement (tests/tsdf_color_statement.py) and of its cases (tests/tsdf_color_cases.py): the
composition is tsdf_warped6_statement.integrate's, the rule holds against a scalar loop and a few words worked by hand, the
cases colour something wherever they update something, and q / -q give the same colour volume."""
import numpy as np
import pytest

import tsdf_color_cases as CC
import tsdf_color_statement as CST
import tsdf_warped6_cases as C6

# coloured / coloured-and-decided voxels per case, as counted with tsdf_warped6_statement on the CPU
COUNTS = {
    "main_volume_skip": (1439, 1439), "main_posed_rigid_junk": (3292, 3292), "odd_scan_moved": (3187, 3186),
    "odd_grid_rigid_posed": (4016, 4016), "big_moved": (1420, 1417), "padded": (194, 194), "thin": (4, 4), "thin_padded": (9, 9),
    "tiny_k3_grid_moved": (225, 225), "no_nodes_rigid": (3108, 3108), "no_nodes_skip": (0, 0),
}


def test_rule_by_hand():
    word = lambda b, g, r, w: b | (g << 8) | (r << 16) | (w << 24)
    # no colour yet: the pixel itself, weight 1 (the pixel's x byte plays no part)
    assert CST.rule_scalar(0, 0xff0a0b0c, 255) == word(0x0c, 0x0b, 0x0a, 1)
    # weight 0 with junk channels: the channels count for nothing
    assert CST.rule_scalar(word(9, 9, 9, 0), word(1, 2, 3, 0), 255) == word(1, 2, 3, 1)
    # w = 1: (c + in + 1) // 2 — the half rounds up; b: (10 + 13 + 1) // 2 = 12, g: (0 + 1 + 1) // 2 = 1, r: (255 + 255 + 1) // 2 = 255
    assert CST.rule_scalar(word(10, 0, 255, 1), word(13, 1, 255, 7), 255) == word(12, 1, 255, 2)
    # w = 255: (255 c + in + 128) // 256; c = 255, in = 0: 65153 // 256 = 254; c = 0, in = 255: 383 // 256 = 1; the weight stays 255
    assert CST.rule_scalar(word(255, 0, 100, 255), word(0, 255, 100, 0), 255) == word(254, 1, 100, 255)
    # the cap binds from above as well: a weight beyond it comes down to it
    assert CST.rule_scalar(word(5, 5, 5, 254), word(5, 5, 5, 0), 3) >> 24 == 3
    assert CST.rule_scalar(word(5, 5, 5, 2), word(5, 5, 5, 0), 3) >> 24 == 3
    assert CST.rule_scalar(word(5, 5, 5, 1), word(5, 5, 5, 0), 3) >> 24 == 2
    # a channel never leaves the byte: the extreme of every weight
    w = np.arange(256, dtype=np.uint32)
    new = CST.rule((w << 24) | 0x00ffffff, np.full(256, 0xffffffff, np.uint32), 255)
    assert np.all((new & 0xffffff) == 0xffffff)


@pytest.mark.parametrize("name", list(C6.CASES))
def test_composition_is_the_tsdf_statements(name):
    """updated, tsdf and the decided set are tsdf_warped6_statement.integrate's own; the texel is inside the image"""
    c = CC.case(name)
    ref, cref = c["ref"], c["cref"]
    assert np.array_equal(cref["updated"], ref["updated"]) and np.array_equal(cref["decided"], ref["decided"])
    assert np.array_equal(cref["tsdf"], ref["tsdf"], equal_nan=True)
    col = cref["coloured"]
    rows, cols = c["dists"].shape
    assert np.all((cref["px"][col] >= 0) & (cref["px"][col] < cols) & (cref["py"][col] >= 0) & (cref["py"][col] < rows))
    assert not (col & ~ref["updated"]).any()


@pytest.mark.parametrize("name", CC.SMALL)
def test_rule_against_a_scalar_loop(name):
    c = CC.case(name)
    cref = c["cref"]
    pix = CST.pixels(c["image"])
    want = c["colors"].copy()
    Z, Y, X = want.shape
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                if cref["updated"][z, y, x] and cref["tsdf"][z, y, x] < 1:
                    want[z, y, x] = CST.rule_scalar(want[z, y, x], pix[cref["py"][z, y, x], cref["px"][z, y, x]], c["max_color_weight"])
    assert np.array_equal(cref["colors"], want)


@pytest.mark.parametrize("name", list(C6.CASES))
def test_cases_colour_something(name):
    c = CC.case(name)
    cref = c["cref"]
    col, dec = cref["coloured"], cref["decided"]
    n, nd = int(col.sum()), int((col & dec).sum())
    print("%-24s coloured %d, coloured and decided %d, updated %d" % (name, n, nd, int(cref["updated"].sum())))
    if cref["updated"].any():
        assert nd > 0
    assert (n, nd) == COUNTS[C6.ANTIPODAL_OF.get(name, name)]
    # nothing else moves, and a coloured voxel's weight is the rule's
    assert np.array_equal(cref["colors"][~col], c["colors"][~col])
    assert np.array_equal(cref["colors"][col] >> 24, np.minimum((c["colors"][col] >> 24) + 1, c["max_color_weight"]))


def test_cases_cover_the_matrix():
    assert {v[0] for v in CC.COLOR.values()} == {"empty", "junk"}
    assert sorted(v[1] for v in CC.COLOR.values()) == [3] + [255] * 11 and CC.COLOR[CC.CAP_CASE] == ("junk", 3)
    c = CC.case(CC.CAP_CASE)
    col = c["cref"]["coloured"]
    w0 = c["colors"][col] >> 24
    for planted in (0, 1, 254, 255):
        assert (w0 == planted).sum() > 0
    assert (((c["colors"] >> 24) == 0) & ((c["colors"] & 0xffffff) != 0)).sum() > 0
    # the cap binds: weights beyond it come down to it, twice over they stop there
    assert (w0 >= 3).sum() > 0 and np.all((c["cref"]["colors"][col] >> 24) <= 3)
    assert np.all((c["cref"]["colors2"][col] >> 24) == np.minimum(np.minimum(w0 + 1, 3) + 1, 3))


def test_antipodal_equality():
    for name, base in C6.ANTIPODAL_OF.items():
        a, b = CC.case(name), CC.case(base)
        assert np.array_equal(a["image"], b["image"]) and np.array_equal(a["colors"], b["colors"])
        assert np.array_equal(a["cref"]["colors"], b["cref"]["colors"])
        assert (a["cref"]["colors"] != a["colors"]).sum() > 500
