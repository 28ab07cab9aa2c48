"""-m gpu: dfa_visible_vertices against its numpy statement (tests/visibility_statement.py) on the cases of
tests/visibility_cases.py.  Both sides run the same correctly rounded float32 sequence, so every flag of every vertex and the
count are compared for equality, with no exclusions; the model map of the two-plane case is dfa_mesh_rasterize's own output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import visibility_cases as C  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402
from visibility_statement import visible_vertices  # noqa: E402


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


@pytest.fixture(scope="module")
def quad_map(A):
    """the near quad of two_planes rasterised on the device: (device map, host copy)"""
    import torch
    quad, idx = C.two_planes_quad()
    cols, rows = C.TP["cols"], C.TP["rows"]
    zb = torch.empty((rows, cols), dtype=torch.int64, device="cuda")
    points = torch.empty((rows, cols, 4), dtype=torch.float32, device="cuda")
    A.mesh_rasterize(dev(quad), None, dev(idx), None, *C.TP["intr"], C.TP["z_near"], cols, rows, zb, points=points)
    return points, host(points).copy()


def _compare(A, v, m_dev, m_host, intr, z_tol, label):
    flags, count = A.visible_vertices(dev(v), m_dev, *intr, z_tol, count=True)
    ref, ref_count = visible_vertices(v, m_host, *intr, z_tol)
    got = host(flags)
    assert got.dtype == np.uint8 and got.shape == (len(v),), label
    assert np.array_equal(got, ref), (label, np.flatnonzero(got != ref)[:10])
    assert int(count.item()) == ref_count, (label, int(count.item()), ref_count)
    alone = A.visible_vertices(dev(v), m_dev, *intr, z_tol)  # without the count: the same flags
    assert np.array_equal(host(alone), ref), label
    return got


def test_two_planes(A, quad_map):
    m_dev, m_host = quad_map
    v, expected = C.two_planes_cloud()
    got = _compare(A, v, m_dev, m_host, C.TP["intr"], C.TP["z_tol"], "two_planes")
    assert np.array_equal(got, expected), np.flatnonzero(got != expected)[:10]  # behind 0, beside 1, the quad's own 1
    v4 = np.concatenate([v, np.ones((len(v), 1), np.float32)], 1)
    _compare(A, v4, m_dev, m_host, C.TP["intr"], C.TP["z_tol"], "two_planes, stride 4")


def test_edge_values_on_a_pitched_map_whose_padding_stays(A):
    store = C.edge_values_map()
    d_store = dev(store)
    before = d_store.clone()
    cols = C.EV["cols"]
    m_dev = d_store[:, :cols]  # a row stride of cols + pad pixels
    assert m_dev.stride(0) == 4 * (cols + C.EV["pad"])
    for name, v, expected in C.edge_values_variants():
        got = _compare(A, v, m_dev, store[:, :cols], C.EV["intr"], C.EV["z_tol"], name)
        assert np.array_equal(got, expected), (name, np.flatnonzero(got != expected))
    assert np.array_equal(bits(host(d_store)), bits(host(before)))  # map and padding: read, never written
    # the same map packed gives the same flags: the padding (points at z = 0) was not read either
    v, expected = C.edge_values_vertices()
    packed = dev(np.ascontiguousarray(store[:, :cols]))
    assert np.array_equal(host(A.visible_vertices(dev(v), packed, *C.EV["intr"], C.EV["z_tol"])), expected)


def test_two_streams_get_their_own_answers(A, quad_map):
    """the per-workgroup counts are scratch of the stream: two streams with different inputs in flight together"""
    import torch
    m_dev, m_host = quad_map
    v, _ = C.two_planes_cloud()
    inputs = [np.tile(v, (40, 1)), np.tile(v[::-1] * np.float32([1, 1, 0.6]), (23, 1)).astype(np.float32)]  # plane at 1.5 / 0.9
    tols = [C.TP["z_tol"], 0.0]
    d_in = [dev(x) for x in inputs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    out = [None, None]
    for rep in range(3):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                out[i] = A.visible_vertices(d_in[i], m_dev, *C.TP["intr"], tols[i], count=True)
    torch.cuda.synchronize()
    counts = []
    for i in (0, 1):
        ref, ref_count = visible_vertices(inputs[i], m_host, *C.TP["intr"], tols[i])
        assert np.array_equal(host(out[i][0]), ref), i
        assert int(out[i][1].item()) == ref_count, i
        counts.append(ref_count)
    assert counts[0] != counts[1] and min(counts) > 0


def test_argument_checks(A):
    import torch
    m = torch.full((4, 4, 4), float("nan"), device="cuda")
    with pytest.raises(A.DynfuAmdError):
        A.visible_vertices(torch.zeros((3, 5), device="cuda"), m, 1.0, 1.0, 0.0, 0.0, 0.0)
    L = A.load()
    v = torch.zeros((2, 3), device="cuda")
    f = torch.zeros((2,), dtype=torch.uint8, device="cuda")
    for args, text in (((v.data_ptr(), 5, 2, m.data_ptr(), 64, 4, 4), b"dfa_visible_vertices: stride must be 3 or 4 floats"),
                       ((v.data_ptr(), 3, -1, m.data_ptr(), 64, 4, 4), b"dfa_visible_vertices: negative vertex count"),
                       ((None, 3, 2, m.data_ptr(), 64, 4, 4), b"dfa_visible_vertices: null vertices / flags"),
                       ((v.data_ptr(), 3, 2, None, 64, 4, 4), b"dfa_visible_vertices: null model map"),
                       ((v.data_ptr(), 3, 2, m.data_ptr(), 64, 0, 4), b"dfa_visible_vertices: non-positive image size"),
                       ((v.data_ptr(), 3, 2, m.data_ptr(), 63, 4, 4), b"dfa_visible_vertices: row step smaller than a float4 row")):
        assert L.dfa_visible_vertices(*args, 1.0, 1.0, 0.0, 0.0, 0.0, f.data_ptr(), None, None) == 1, text
        assert L.dfa_last_error() == text
