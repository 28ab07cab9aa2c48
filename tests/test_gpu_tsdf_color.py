"""-m gpu tests of dfa_tsdf_integrate_warped6_color against the numpy statement tests/tsdf_color_statement.py on the cases of
tests/tsdf_color_cases.py, every case both searching and from a KnnField:
  1. the TSDF volume and the occupancy map are those of tsdf_integrate_warped6 with the same field, bit for bit;
  2. on DECIDED voxels the colour volume is the statement's, word for word (what the statement leaves alone holds its input);
  3. an undecided voxel holds its input word, or an update by the rule from a texel within one pixel of the statement's
     (where the statement has no projection at all — an unsupported voxel on the edge of support — from a texel of the image);
  4. the colour volume with the field is the searching one's, bit for bit;
  5. colours only (vol=None): the same colour volume, the occupancy map untouched;
  6. two calls in a row are the statement applied twice; on the cap case the weights stop at 3;
  7. two streams, two volumes, the same bits.
Each case's calls are made once and shared by the checks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tsdf_color_cases as CC  # noqa: E402
import tsdf_color_statement as CST  # noqa: E402
import tsdf_warped6_cases as C6  # noqa: E402
import tsdf_warped6_statement as W6  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from tsdf_color_check import check_colors  # noqa: E402  (checks 2 and 3)

MODE = {W6.SKIP: "skip", W6.RIGID: "rigid"}
NAMES = list(C6.CASES)
FIELD = [False, True]


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def nodes_of(c):
    return tuple(dev(c[n]) if c["D"] else None for n in ("nodes", "node_dq", "node_w"))


def make_field(A, c, keep):
    f = A.KnnField(c["dims"], c["voxel_size"], c["k"], vol2node=c.get("vol2node"))
    f.build(keep[0], keep[2])
    return f


def occ_pattern(A, vol):
    import torch
    occ = A.tsdf_occupancy(vol)
    before = np.random.default_rng(5).integers(0, 4, tuple(occ.shape)).astype(np.uint8)
    before[::2] = 0
    occ.copy_(torch.from_numpy(before))
    return occ, before


def call(A, c, vol, colors, keep, field=None, occupancy=None):
    A.tsdf_integrate_warped6_color(vol, colors, dev(c["image"]), dev(c["dists"]), c["voxel_size"], float(c["trunc"]), C6.MAX_WEIGHT,
                                   c["max_color_weight"], c["vol2node"], c["node2cam"], *c["intr"], *keep, c["k"],
                                   unsupported=MODE[c["mode"]], occupancy=occupancy, field=field)


_RESULTS = {}


def results(A, name, with_field):
    """every call of one case in one mode, made ONCE — a failure is kept and raised again, not run again"""
    key = (name, with_field)
    if key not in _RESULTS:
        try:
            _RESULTS[key] = _run(A, name, with_field)
        except Exception as e:  # noqa: BLE001
            _RESULTS[key] = e
    if isinstance(_RESULTS[key], Exception):
        raise _RESULTS[key]
    return _RESULTS[key]


def _run(A, name, with_field):
    c = CC.case(name)
    keep = nodes_of(c)
    f = make_field(A, c, keep) if with_field else None
    out = {}
    # the plain call
    vol = dev(c["vol"])
    occ, out["occ_before"] = occ_pattern(A, vol)
    A.tsdf_integrate_warped6(vol, dev(c["dists"]), c["voxel_size"], float(c["trunc"]), C6.MAX_WEIGHT, c["vol2node"], c["node2cam"],
                             *c["intr"], *keep, c["k"], unsupported=MODE[c["mode"]], occupancy=occ, field=f)
    out["plain_vol"], out["plain_occ"] = host(vol, np.uint32), host(occ)
    # the fused call, then a second one on its outputs
    vol, colors = dev(c["vol"]), dev(c["colors"])
    occ, _ = occ_pattern(A, vol)
    call(A, c, vol, colors, keep, f, occ)
    out["vol"], out["occ"], out["colors"] = host(vol, np.uint32), host(occ), host(colors, np.uint32)
    call(A, c, vol, colors, keep, f, occ)
    out["colors2"] = host(colors, np.uint32)
    # colours only
    colors = dev(c["colors"])
    occ, _ = occ_pattern(A, vol)
    call(A, c, None, colors, keep, f, occ)
    out["only_colors"], out["only_occ"] = host(colors, np.uint32), host(occ)
    if f is not None:
        f.close()
    return out


@pytest.mark.parametrize("with_field", FIELD)
@pytest.mark.parametrize("name", NAMES)
def test_tsdf_half_is_the_plain_call(A, name, with_field):
    r = results(A, name, with_field)
    assert np.array_equal(r["vol"], r["plain_vol"]), "the TSDF volume differs from the plain call's"
    assert np.array_equal(r["occ"], r["plain_occ"]), "the occupancy map differs from the plain call's"


@pytest.mark.parametrize("with_field", FIELD)
@pytest.mark.parametrize("name", NAMES)
def test_colors_against_statement(A, name, with_field):
    c = CC.case(name)
    r = results(A, name, with_field)
    check_colors(r["colors"], c["cref"]["colors"], c["colors"], c)


@pytest.mark.parametrize("name", NAMES)
def test_field_gives_the_searching_colors(A, name):
    a, b = results(A, name, False), results(A, name, True)
    assert np.array_equal(a["colors"], b["colors"]) and np.array_equal(a["colors2"], b["colors2"])


@pytest.mark.parametrize("with_field", FIELD)
@pytest.mark.parametrize("name", NAMES)
def test_colors_only(A, name, with_field):
    r = results(A, name, with_field)
    assert np.array_equal(r["only_colors"], r["colors"]), "colours only: another colour volume"
    assert np.array_equal(r["only_occ"], r["occ_before"]), "colours only: the occupancy map was written"


@pytest.mark.parametrize("with_field", FIELD)
@pytest.mark.parametrize("name", NAMES)
def test_two_calls_are_the_statement_twice(A, name, with_field):
    c = CC.case(name)
    r = results(A, name, with_field)
    cref = c["cref"]
    m = cref["decided"]  # (an undecided voxel may have taken another way in either call)
    assert np.array_equal(r["colors2"][m], cref["colors2"][m])
    if name == CC.CAP_CASE:
        col = cref["coloured"] & cref["decided"]
        w0, w2 = c["colors"][col] >> 24, r["colors2"][col] >> 24
        assert (w0 >= 1).sum() > 0 and np.all(w2[w0 >= 1] == 3), "a weight of 1 and more is at the cap after two calls"
        assert (w0 == 0).sum() > 0 and np.all(w2[w0 == 0] == 2) and np.all(w2 <= 3)


def test_antipodal_gives_the_same_colors(A):
    for name, base in C6.ANTIPODAL_OF.items():
        assert np.array_equal(results(A, name, False)["colors"], results(A, base, False)["colors"])


def test_two_streams(A):
    """two calls with different node sets in flight on two streams: the scratch (node grid, brick flags) is per stream"""
    import torch
    names = ("main_posed_rigid_junk", "big_moved")
    cases = [CC.case(n) for n in names]
    single = [results(A, n, False) for n in names]
    torch.cuda.synchronize()
    streams = torch.cuda.Stream(), torch.cuda.Stream()
    for rep in range(3):
        out = []
        for c, s in zip(cases, streams):
            vol, colors, keep = dev(c["vol"]), dev(c["colors"]), nodes_of(c)
            args = (dev(c["image"]), dev(c["dists"]))
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                A.tsdf_integrate_warped6_color(vol, colors, args[0], args[1], c["voxel_size"], float(c["trunc"]), C6.MAX_WEIGHT,
                                               c["max_color_weight"], c["vol2node"], c["node2cam"], *c["intr"], *keep, c["k"],
                                               unsupported=MODE[c["mode"]])
            out.append((vol, colors, keep, args))
        torch.cuda.synchronize()
        for (vol, colors, _, _), want in zip(out, single):
            assert np.array_equal(host(vol, np.uint32), want["vol"]) and np.array_equal(host(colors, np.uint32), want["colors"])
