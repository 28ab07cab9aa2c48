"""-m gpu tests of dfa_tsdf_integrate_warped6 against the numpy statement tests/tsdf_warped6_statement.py on the cases of
tests/tsdf_warped6_cases.py, under the bar of tests/test_gpu_tsdf_warped.py: on DECIDED voxels the update set and the
weights are the statement's exactly, the unpacked distance is within rho sqrt(3) / trunc + 2^-11 of it, and what the
statement leaves alone is the input bit for bit; an undecided voxel holds its input or a valid update.  A brick the support
pre-pass missed shows as decided, supported voxels that did not change: the "posed" and "moved" cases are what exercise it.

And with no tolerance at all: a supported voxel moves as dfa_solver6_warp_with moves a vertex at its position."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tsdf_warped6_cases as C6  # noqa: E402
import tsdf_warped6_statement as W6  # noqa: E402
import tsdf_warped_statement as WST  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from tsdf_warped6_check import check  # noqa: E402  (the bar of the module docstring)

MODE = {W6.SKIP: "skip", W6.RIGID: "rigid"}


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


def run(A, c, occupancy=None):
    """the call on a copy of the case's starting volume -> the volume after it (uint32 (Z, Y, X))"""
    vol = dev(c["vol"])
    nodes, dq, w = (dev(c[n]) if c["D"] else None for n in ("nodes", "node_dq", "node_w"))
    A.tsdf_integrate_warped6(vol, dev(c["dists"]), c["voxel_size"], float(c["trunc"]), C6.MAX_WEIGHT, c["vol2node"], c["node2cam"],
                             *c["intr"], nodes, dq, w, c["k"], unsupported=MODE[c["mode"]], occupancy=occupancy)
    return host(vol, np.uint32)


@pytest.mark.parametrize("name", list(C6.CASES))
def test_against_statement(A, name):
    c = C6.case(name)
    check(run(A, c), c)


def test_antipodal_gives_the_same_volume(A):
    """q and -q: the hemisphere sign is taken against the first active neighbour, so the float32 products are the same numbers"""
    for name, base in C6.ANTIPODAL_OF.items():
        assert np.array_equal(run(A, C6.case(name)), run(A, C6.case(base)))


def test_the_same_blend_as_the_solves_warp(A):
    """No tolerance.  32^3, both transforms NULL, (D, k) = (300, 8), SKIP: a Solver6 plan over the voxel positions as its cloud
    and the case's nodes; warp_with(node_dq) is the device's own p.  With NULL transforms c = v and vc = p exactly, so step 7
    (probe, update: float32 statements) applied to that p must give the kernel's volume bit for bit on every supported voxel
    whose support quotient is more than 1e-6 from 1 — any difference is a difference in the blend or the weights."""
    c = C6.case("main_volume_skip")
    assert c["vol2node"] is None and c["node2cam"] is None and (c["D"], c["k"], c["mode"]) == (300, 8, W6.SKIP)
    ref = c["ref"]
    v = WST.voxel_positions(c["vol"].shape, c["voxel_size"])
    assert len(v) == 32768
    s = A.Solver6(c["D"], len(v), c["k"])
    keep = [dev(c["nodes"]), dev(c["node_dq"]), dev(c["node_w"]), dev(v)]
    s.set_problem(keep[0], keep[1], keep[2], keep[3], None)
    p, _ = s.warp_with(keep[1], want_normals=False)
    p = host(p)
    upd, _, _, tsdf = WST.probe(p, c["dists"], c["trunc"], *c["intr"])
    want = c["vol"].reshape(-1).copy()
    want[upd] = WST.update(want[upd], tsdf[upd], C6.MAX_WEIGHT)
    got = run(A, c).reshape(-1)
    where = ref["supported"].reshape(-1) & (np.abs(ref["qmin"].reshape(-1).astype(np.float64) - 1.0) > 1e-6)
    print("%d supported voxels compared, %d of them updated; differing: %d" %
          (int(where.sum()), int((upd & where).sum()), int((got != want)[where].sum())))
    assert where.sum() >= 500 and (upd & where).sum() >= 500
    assert np.array_equal(got[where], want[where])


def test_no_nodes_skip_changes_nothing(A):
    c = C6.case("no_nodes_skip")
    assert np.array_equal(run(A, c), c["vol"])


def test_no_nodes_rigid_is_the_rigid_integrate(A):
    """D = 0, RIGID, a "posed" pair: every voxel takes p = c — dfa_tsdf_integrate with vol2cam = node2cam . vol2node up to the
    rounding of the two products against one and its running sum of positions, hence compared under the statement's rule"""
    c = C6.case("no_nodes_rigid")
    assert c["frame"] == "posed"
    vol = dev(c["vol"])
    A.tsdf_integrate(vol, dev(c["dists"]), c["voxel_size"], float(c["trunc"]), C6.MAX_WEIGHT, W6.compose(c["node2cam"], c["vol2node"]),
                     *c["intr"])
    check(run(A, c), c, want=host(vol, np.uint32))


@pytest.mark.parametrize("name", ["odd_scan_moved", "main_posed_rigid_junk"])
def test_occupancy_superset(A, name):
    """the map of dfa_tsdf_integrate_occ: bytes are only set, and the box of every voxel the call updated has bit 0"""
    import torch
    c = C6.case(name)
    vol0 = dev(c["vol"])
    occ = A.tsdf_occupancy(vol0)
    before = np.random.default_rng(5).integers(0, 4, tuple(occ.shape)).astype(np.uint8)
    before[::2] = 0
    occ.copy_(torch.from_numpy(before))
    got = run(A, c, occupancy=occ)
    after = host(occ)
    assert np.array_equal(got, run(A, c)), "the map changes the volume"
    assert np.array_equal(after & before, before), "a byte lost a bit"
    touched = (got != c["vol"]) | (c["ref"]["updated"] & c["ref"]["decided"])
    z, y, x = np.nonzero(touched)
    assert len(z) > 0
    assert np.all(after[z // 8, y // 2, x // 32] & 1), "an updated voxel in an unmarked box"


def test_two_streams(A):
    """two calls with different node sets in flight on two streams: the scratch (node grid, brick flags) is per stream"""
    import torch
    ca, cb = C6.case("main_posed_rigid_junk"), C6.case("big_moved")
    single = run(A, ca), run(A, cb)
    torch.cuda.synchronize()
    streams = torch.cuda.Stream(), torch.cuda.Stream()
    both = []
    for rep in range(3):
        out = []
        for c, s in zip((ca, cb), streams):
            vol = dev(c["vol"])
            args = [dev(c[n]) for n in ("dists", "nodes", "node_dq", "node_w")]
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                A.tsdf_integrate_warped6(vol, args[0], c["voxel_size"], float(c["trunc"]), C6.MAX_WEIGHT, c["vol2node"], c["node2cam"],
                                         *c["intr"], args[1], args[2], args[3], c["k"], unsupported=MODE[c["mode"]])
            out.append((vol, args))
        torch.cuda.synchronize()
        both.append([host(v, np.uint32) for v, _ in out])
    for got in both:
        assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1])
