"""dfa_mesh_rasterize on the GPU against tests/raster_statement.py (rasterize32), byte for byte, on the cases of
tests/raster_cases.py; and one cross-check against the raycast of the volume the sphere mesh was extracted from."""
import numpy as np
import pytest

import raster_cases as RC
import raster_statement as RS

pytestmark = pytest.mark.gpu

MARKER = 123.25  # fills the maps, padding included, before a call
PAD = 3          # pixels of padding behind every row of a map


def _map(c):
    import torch
    full = torch.full((c["rows"], c["cols"] + PAD, 4), MARKER, dtype=torch.float32, device="cuda")
    return full, full[:, :c["cols"]]


def _run(c, vertex_normals=True, want_points=True, want_normals=True, buffers=None):
    """-> (z-buffer uint64, points, normals as numpy; None for a map not asked for), the buffers used"""
    import torch
    import dynfu_amd as A
    from gpu_util import dev, host
    if buffers is None:
        buffers = (torch.zeros((c["rows"], c["cols"]), dtype=torch.int64, device="cuda"), _map(c), _map(c))
    zb, (pfull, pview), (nfull, nview) = buffers
    normals = dev(c["normals"]) if vertex_normals and c["normals"] is not None else None
    A.mesh_rasterize(dev(c["vertices"]), normals, dev(c["indices"]), c["world2cam"], *c["intr"], c["z_near"], c["cols"],
                     c["rows"], zb, pview if want_points else None, nview if want_normals else None)
    torch.cuda.synchronize()
    out = [host(zb, np.uint64)]
    for full, want in ((pfull, want_points), (nfull, want_normals)):
        h = host(full)
        assert (h[:, c["cols"]:] == MARKER).all(), "padding written"
        out.append(h[:, :c["cols"]].copy() if want else None)
        if not want:
            assert (h == MARKER).all(), "a map that was not asked for was written"
    return out, buffers


def _same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", RC.NAMES)
def test_maps_are_the_statements_byte_for_byte(name):
    c = RC.case(name)
    ref_z, ref_p, ref_n = RC.reference(name)
    (z, p, n), buffers = _run(c)
    differ = z != ref_z
    assert not differ.any(), "%d pixels of the z-buffer differ, first %s" % (differ.sum(), np.argwhere(differ)[:3].tolist())
    assert _same_bytes(p, ref_p), "point map"
    assert _same_bytes(n, ref_n), "normal map"
    # a second call into the same buffers: the fill step clears the first call's z-buffer
    (z2, p2, n2), _ = _run(c, buffers=buffers)
    assert np.array_equal(z2, z) and _same_bytes(p2, p) and _same_bytes(n2, n)


@pytest.mark.parametrize("name", ["g", "i"])
def test_triangle_order_does_not_change_depth_or_points(name):
    shuffled, perm = RC.permuted(name)
    ref_z, ref_p, _ = RC.reference(name)
    (z, p, _), _ = _run(shuffled, want_normals=False)
    assert np.array_equal(RS.depth_bits(z), RS.depth_bits(ref_z)) and _same_bytes(p, ref_p)
    hit = z != RS.MISS
    assert np.array_equal(hit, ref_z != RS.MISS) and (perm[RS.coverage(z)[hit]] != RS.coverage(ref_z)[hit]).mean() < 0.01


def test_either_map_may_be_null():
    c = RC.case("i")
    ref_z, ref_p, ref_n = RC.reference("i")
    (z, p, n), _ = _run(c, want_normals=False)
    assert n is None and np.array_equal(z, ref_z) and _same_bytes(p, ref_p)
    (z, p, n), _ = _run(c, want_points=False)
    assert p is None and np.array_equal(z, ref_z) and _same_bytes(n, ref_n)
    (z, p, n), _ = _run(c, want_points=False, want_normals=False)
    assert np.array_equal(z, ref_z)


@pytest.mark.parametrize("name", ["i", "j"])
def test_face_normals_without_vertex_normals(name):
    ref_z, ref_p, ref_n = RC.reference(name, face_normals=True)
    (z, p, n), _ = _run(RC.case(name), vertex_normals=False)
    assert np.array_equal(z, ref_z) and _same_bytes(p, ref_p) and _same_bytes(n, ref_n)
    assert not _same_bytes(ref_n, RC.reference(name)[2])


def test_invalid_arguments():
    import torch
    import dynfu_amd as A
    from gpu_util import dev
    c = RC.case("a")
    v, idx = dev(c["vertices"]), dev(c["indices"])
    zb = torch.zeros((16, 16), dtype=torch.int64, device="cuda")
    pts = torch.zeros((16, 16, 4), dtype=torch.float32, device="cuda")
    L = A._lib
    f, st = L.load().dfa_mesh_rasterize, L._stream()

    def call(vertices=v.data_ptr(), N=3, indices=idx.data_ptr(), T=1, z_near=0.1, cols=16, rows=16, zbuffer=zb.data_ptr(),
             points=pts.data_ptr(), step=256):
        return f(vertices, None, N, indices, T, None, 1, 1, 0, 0, z_near, cols, rows, zbuffer, points, step, None, 0, st)

    assert call() == 0
    for kw in (dict(zbuffer=None), dict(cols=0), dict(rows=0), dict(cols=8193, step=8193 * 16), dict(rows=8193), dict(z_near=0.0),
               dict(z_near=-1.0), dict(T=-1), dict(N=-1), dict(vertices=None), dict(indices=None), dict(step=240),
               dict(points=pts.data_ptr() + 4), dict(zbuffer=zb.data_ptr() + 4)):
        assert call(**kw) == 1, kw  # DFA_ERR_INVALID
    assert call(vertices=None, N=0, indices=None, T=0) == 0  # no triangle is a valid mesh
    torch.cuda.synchronize()
    assert torch.isnan(pts).all()
    with pytest.raises(A.DynfuAmdError):
        A.mesh_rasterize(v, None, idx, None, 1, 1, 0, 0, 0.1, 16, 16, zb[:8], pts, None)


def test_depth_agrees_with_the_raycast_of_the_same_volume():
    """both trace the zero level set of the same volume from the same camera, one linearly per lattice edge and one
    trilinearly per cell: over the pixels both hit, the median depth difference is below one voxel edge"""
    import torch
    import dynfu_amd as A
    import render_scenes
    from gpu_util import dev, host
    _, _, _, vol, voxel, trunc, intr, cols, rows = RC.sphere_mesh()
    c = RC.case("i")
    w2c = np.asarray(c["world2cam"], np.float64)
    assert np.array_equal(w2c[:9].reshape(3, 3), np.eye(3))
    cam2vol = np.concatenate([np.eye(3).reshape(-1), -w2c[9:]]).astype(np.float32)
    rp = torch.empty((rows, cols, 4), dtype=torch.float32, device="cuda")
    rn = torch.empty_like(rp)
    A.tsdf_raycast_points(dev(vol), voxel, trunc, cam2vol, np.eye(3, dtype=np.float32).reshape(-1), *intr, render_scenes.STEP,
                          render_scenes.DELTA, rp, rn)
    (z, p, _), _ = _run(c, want_normals=False)
    ray_z = host(rp)[..., 2]
    both = (z != RS.MISS) & ~np.isnan(ray_z)
    diff = np.abs(p[..., 2][both].astype(np.float64) - ray_z[both])
    print("%d pixels hit by both (%d raster, %d raycast), median |dz| %.4g m, voxel %.4g m"
          % (both.sum(), (z != RS.MISS).sum(), (~np.isnan(ray_z)).sum(), np.median(diff), float(voxel[0])))
    assert both.sum() > 0.1 * rows * cols
    assert np.median(diff) < float(voxel[0])
