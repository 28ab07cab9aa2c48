"""Device-event timing of the mesh rasteriser (dfa_mesh_rasterize) on the welded marching-cubes mesh of volumes fused from
the synthetic depth frame (dynfu_amd/synth.py, frame 0, as bench.py builds them), from the configuration's own camera — C2
(512^3, VGA) and C4 (1024^3, 1280 x 720) — beside dfa_tsdf_raycast_points of the same volume and camera IN THE SAME RUN:
  fill + draw                 the call with both maps NULL
  fill + draw + resolve       the whole call (resolve = the difference of the medians)
  the same two from a camera 4 x nearer to the sphere, where a triangle covers some tens of pixels
  raycast_points              context, not a bar: it does other work and fetches no vertices
The large-triangle threshold is a compile-time constant of csrc/raster.hip (DFA_RASTER_WIDE_BOX).  Other values are other
builds of the library:  bash tools/ab_variant.sh wide16 raster.hip -DDFA_RASTER_WIDE_BOX=16  and then
`--variant wide16=dynfu_amd/build/libdynfu_amd_wide16.so`; every variant's items alternate with the product library's inside
every window.  Per item: the median over the windows with [min, max] — the spread a difference has to exceed.
usage: python tools/mesh_view_timing.py [--configs C2 C4] [--windows 9] [--reps 100] [--variant tag=path ...]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dynfu_amd as A
from dynfu_amd import synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["C2", "C4"])
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--variant", action="append", default=[])
    args = ap.parse_args()
    L = A._lib
    libs = [("product", L.load())]
    for v in args.variant:
        tag, path = v.split("=", 1)
        with L.use_library(os.path.abspath(path)) as lib:
            libs.append((tag, lib))
    tri, nv = (torch.from_numpy(t).cuda() for t in A.mc_default_tables())
    for name in args.configs:
        cfg = synth.CONFIGS[name]
        intr = synth.intrinsics(cfg)
        voxel, trunc, vol2cam, cam2vol, rinv = synth.volume_params(cfg)
        W, H, dim = cfg["width"], cfg["height"], cfg["dim"]
        depth = torch.from_numpy(synth.depth_frame(cfg, 0).copy()).cuda()
        dists = torch.empty(depth.shape, dtype=torch.uint16, device="cuda")
        A.compute_dists(depth, dists, *intr)
        vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
        A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, *intr)
        _, _, t = A.marching_cubes_indexed(vol, voxel, tri, nv, 0, 0)
        nvert, nidx = (int(v) for v in t.cpu())
        verts, idx, _ = A.marching_cubes_indexed(vol, voxel, tri, nv, nvert, nidx)
        normals = A.tsdf_vertex_normals(vol, voxel, synth.GRADIENT_DELTA_FACTOR, verts)
        zb = torch.zeros((H, W), dtype=torch.int64, device="cuda")
        pts = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        nrm = torch.zeros_like(pts)
        rp, rn = torch.zeros_like(pts), torch.zeros_like(pts)
        near = np.array(vol2cam, np.float32)  # the mesh is in the volume's frame: vol2cam is its world2cam
        near[11] -= 0.75 * (synth.SPHERE_C[2] - synth.SPHERE_R)  # the camera 4 x nearer to the front of the sphere
        cams = {"": L._aff12(vol2cam), ", near": L._aff12(near)}
        st = L._stream()
        dv, dn, di, dz, dp, dm = L._dev(verts), L._dev(normals), L._dev(idx), L._dev(zb), L._dev(pts), L._dev(nrm)

        def raster(lib, cam, maps):
            L._check(lib.dfa_mesh_rasterize(dv, dn, nvert, di, nidx // 3, cam, *intr, 0.05, W, H, dz, dp if maps else None, W * 16,
                                            dm if maps else None, W * 16, st))

        vs, aff, rinv9 = L._farr(voxel, 3), L._aff12(cam2vol), L._farr(np.asarray(rinv, np.float32).reshape(-1), 9)

        def raycast():
            L._check(libs[0][1].dfa_tsdf_raycast_points(L._dev(vol), dim, dim, dim, vs, trunc, aff, rinv9, *intr,
                                                        synth.RAYCAST_STEP_FACTOR, synth.GRADIENT_DELTA_FACTOR, L._dev(rp), W * 16,
                                                        L._dev(rn), W * 16, W, H, st))

        items = [("raycast_points", raycast)]
        for tag, lib in libs:
            for cname, cam in cams.items():
                items.append((f"{tag}: fill + draw{cname}", lambda lib=lib, cam=cam: raster(lib, cam, False)))
                items.append((f"{tag}: fill + draw + resolve{cname}", lambda lib=lib, cam=cam: raster(lib, cam, True)))
        for _, fn in items:  # warm-up
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        # what is timed is the same picture in every build
        pictures = {}
        for tag, lib in libs:
            for cname, cam in cams.items():
                raster(lib, cam, True)
                pictures.setdefault(cname, []).append((zb.clone(), pts.clone()))
        for cname, ps in pictures.items():
            assert all(torch.equal(p[0], ps[0][0]) and torch.equal(p[1].view(torch.int32), ps[0][1].view(torch.int32)) for p in ps), cname
        ms = {label: [] for label, _ in items}
        for _ in range(args.windows):
            for label, fn in items:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                ms[label].append(e0.elapsed_time(e1) / args.reps)
        hit = {c: float((p[0][0] != -1).float().mean().item()) for c, p in pictures.items()}
        print(f"{name}: {dim}^3 volume, {nidx // 3} triangles on {nvert} vertices, {W} x {H}; hit {hit['']:.1%}, near {hit[', near']:.1%}; "
              f"raycast hit {float((~torch.isnan(rp[..., 0])).float().mean().item()):.1%}; {args.windows} windows x {args.reps} calls, "
              f"median [min, max] ms per call")
        for label, _ in items:
            print(f"  {label:48s} {np.median(ms[label]):7.4f} ms [{min(ms[label]):.4f}, {max(ms[label]):.4f}]")
        del vol, verts, idx, normals, zb, pts, nrm, rp, rn
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
