"""-m gpu tests of dfa_color_sample against the fp64 statement tests/color_sample_statement.py on the cases of
tests/color_sample_cases.py: on DECIDED vertices (|den - 0.25| > 1e-3) `a` is the statement's exactly and every channel is
within the statement's bound (1 for the final rounding + 255 * 4 * delta); an undecided vertex is either 0, 0, 0, 0 or a = 255
with channels within the bound of the statement's quotient; strides 3 and 4 give the same bytes; N = 0 succeeds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import color_sample_cases as SC  # noqa: E402
from gpu_util import dev, host  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


@pytest.mark.parametrize("name", list(SC.CASES))
def test_against_statement(A, name):
    c = SC.case(name)
    r = c["ref"]
    colors = dev(c["colors"])
    got = host(A.color_sample(colors, c["voxel_size"], dev(c["vertices"]), c["to_volume"]))
    got3 = host(A.color_sample(colors, c["voxel_size"], dev(c["vertices"][:, :3]), c["to_volume"]))
    assert got.shape == (len(c["vertices"]), 4) and got.dtype == np.uint8
    assert np.array_equal(got, got3), "stride 3 and stride 4 differ"
    dec = r["decided"]
    err = np.abs(got[:, :3].astype(np.float64) - r["bgr"])
    lit = got[:, 3] == 255
    print("%s: %d vertices, %d undecided, a differing on decided: %d, largest channel error %.4f (bound %.6f)" %
          (name, len(got), int((~dec).sum()), int((got[:, 3] != r["a"])[dec].sum()), float(err[dec].max()), float(r["bound"].max())))
    assert np.array_equal(got[dec, 3], r["a"][dec]), "a on decided vertices"
    assert np.all(err[dec] <= r["bound"][dec, None]), "channels on decided vertices"
    assert np.all(got[~lit] == 0) and np.all((got[:, 3] == 0) | lit), "a vertex without colour is 0, 0, 0, 0"
    # an undecided vertex: den is within 1e-3 of the threshold, either answer stands — the quotient is the statement's
    for i in np.flatnonzero(~dec):
        if got[i, 3] == 255 and r["a"][i] == 255:
            assert np.all(np.abs(got[i, :3].astype(np.float64) - r["bgr"][i]) <= r["bound"][i])


def test_no_vertices(A):
    import torch
    c = SC.case("small")
    out = A.color_sample(dev(c["colors"]), c["voxel_size"], torch.empty((0, 4), dtype=torch.float32, device="cuda"))
    assert tuple(out.shape) == (0, 4)
