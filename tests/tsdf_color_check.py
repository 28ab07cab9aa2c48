"""The per-voxel comparison of a colour volume after dfa_tsdf_integrate_warped6_color with tests/tsdf_color_statement.py,
shared by tests/test_gpu_tsdf_color.py and the north-star frame statement (tests/northstar_statement.py): on DECIDED voxels
the colour volume is the statement's, word for word (what the statement leaves alone holds its input); an undecided voxel
holds its input word, or an update by the rule from a texel within one pixel of the statement's (where the statement has no
projection at all — an unsupported voxel on the edge of support — from a texel of the image)."""
import numpy as np

import tsdf_color_statement as CST


def check_colors(got, want, before, c):
    """`got` against the statement's `want`, from the colour volume `before`.  c: name, cref (tsdf_color_statement.integrate's
    dict), image, max_color_weight"""
    cref = c["cref"]
    dec = cref["decided"]
    col = cref["coloured"]
    print("%s: %d voxels, %d coloured by the statement, %d undecided; decided words differing: %d" %
          (c["name"], got.size, int(col.sum()), int((~dec).sum()), int((got != want)[dec].sum())))
    assert np.array_equal(got[dec], want[dec]), "colour words of decided voxels"
    assert np.array_equal(got[dec & ~col], before[dec & ~col]), "decided voxels the statement leaves alone"
    und = np.flatnonzero(~dec.ravel())
    pix = CST.pixels(c["image"])
    rows, cols = pix.shape
    g, b = got.ravel()[und], before.ravel()[und]
    qx, qy = cref["qx"].ravel()[und], cref["qy"].ravel()[und]
    ok = g == b
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            x, y = qx + dx, qy + dy
            inside = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
            p = pix[np.where(inside, y, 0), np.where(inside, x, 0)]
            ok |= inside & (CST.rule(b, p, c["max_color_weight"]) == g)
    for i in np.flatnonzero(~ok & (qx == CST.FAR)):  # no projection in the statement: any texel of the image
        ok[i] = bool((CST.rule(np.full(pix.size, b[i], np.uint32), pix.ravel(), c["max_color_weight"]) == g[i]).any())
    assert ok.all(), "an undecided voxel holds neither its input nor an update from a texel next to the statement's"
