"""CPU checks of the colour-sample statement (tests/color_sample_statement.py) and its cases: a cell worked by hand, the
recorded float32 deviations hold, at most 1 % of the vertices are undecided, and the cases reach every branch."""
import numpy as np
import pytest

import color_sample_cases as SC
import color_sample_statement as CS


def word(b, g, r, w):
    return np.uint32(b | (g << 8) | (r << 16) | (w << 24))


def test_a_cell_by_hand():
    """a (2, 2, 2) volume of 0.5 m voxels; corner (0, 0, 0) = (10, 20, 30), corner (1, 0, 0) = (110, 120, 130), corner
    (0, 1, 0) has weight 0 (its channels count for nothing), the other five are (50, 50, 50)"""
    col = np.full((2, 2, 2), word(50, 50, 50, 9), np.uint32)
    col[0, 0, 0], col[0, 0, 1], col[0, 1, 0] = word(10, 20, 30, 1), word(110, 120, 130, 255), word(200, 200, 200, 0)
    vs = [0.5, 0.5, 0.5]
    v = np.array([[0.125, 0.0, 0.0],   # g = (0.25, 0, 0): 0.75 of corner 0, 0.25 of corner 1
                  [0.0, 0.25, 0.0],    # g = (0, 0.5, 0): half the weight sits on the corner without colour: den = 0.5
                  [0.0, 0.4, 0.0],     # g = (0, 0.8, 0): den = 0.2 < 0.25
                  [0.75, 0.0, 0.0],    # g = (1.5, 0, 0): the cell's far side is outside the volume: den = 0.5, corner 1 alone
                  [-0.4, 0.0, 0.0],    # g = (-0.8, 0, 0): corner 0 with t = 0.2: nothing
                  [np.nan, 0.0, 0.0]], np.float32)
    r = CS.sample(col, vs, v, None, 0.0)
    assert r["a"].tolist() == [255, 255, 0, 255, 0, 0]
    assert np.allclose(r["den"][:5], [1.0, 0.5, 0.2, 0.5, 0.2], atol=1e-6)
    assert np.allclose(r["bgr"][0], [0.75 * 10 + 0.25 * 110, 0.75 * 20 + 0.25 * 120, 0.75 * 30 + 0.25 * 130])
    assert np.allclose(r["bgr"][1], [10, 20, 30]) and np.allclose(r["bgr"][3], [110, 120, 130], atol=1e-4)
    assert np.all(r["bgr"][[2, 4, 5]] == 0) and r["decided"].all() and np.all(r["bound"] == 1.0)
    # a frame: the same answers for the vertices taken to it
    to_volume = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, 0.25, -0.5, 1.0], np.float32)  # q = R p + t
    R, t = to_volume[:9].reshape(3, 3).astype(np.float64), to_volume[9:].astype(np.float64)
    p = ((v[:5].astype(np.float64) - t) @ R).astype(np.float32)  # R^T (q - t)
    rp = CS.sample(col, vs, p, to_volume, 0.0)
    assert rp["a"].tolist() == r["a"][:5].tolist() and np.allclose(rp["bgr"], r["bgr"][:5], atol=1e-4)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_recorded_deviation_holds(name):
    c = SC.case(name)
    Z, Y, X = c["colors"].shape
    d = CS.deviation(c["vertices"], c["voxel_size"], c["to_volume"], (X, Y, Z))
    print("%-12s delta measured %.4e, recorded %.4e" % (name, d, c["delta"]))
    assert d <= c["delta"] < 1e-4
    assert d > c["delta"] / 2 or c["delta"] == 0.0


@pytest.mark.parametrize("name", list(SC.CASES))
def test_undecided_share_and_coverage(name):
    c = SC.case(name)
    r = c["ref"]
    N = len(c["vertices"])
    und = int((~r["decided"]).sum())
    print("%-12s %d vertices (%d of the mesh), a = 255 on %d, %d undecided, bound %.6f" %
          (name, N, c["n_mesh"], int((r["a"] == 255).sum()), und, float(r["bound"].max())))
    assert und <= 0.01 * N
    assert N >= 2000 and c["n_mesh"] >= 300
    assert (r["a"] == 255).sum() >= 300 and (r["a"] == 0).sum() >= 300
    assert ((r["den"] > 0.3) & (r["den"] < 0.9)).sum() >= 100 and ((r["den"] > 0.0) & (r["den"] < 0.2)).sum() >= 20
    assert np.all(r["a"][-c["n_bad"]:] == 0) and np.all(r["bgr"] >= 0) and np.all(r["bgr"] <= 255)
    assert np.all(r["bound"] == 1.0 + 255.0 * 4.0 * c["delta"])
