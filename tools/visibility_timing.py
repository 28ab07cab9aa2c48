"""Device-event timing of dfa_visible_vertices and of the vertex-mask gather (dfa_solver6_set_vertex_mask) at the size of
the C2 adaptor frame: the marching-cubes cloud of the 512^3 volume fused from the synthetic depth frame (dynfu_amd/synth.py,
frame 0, as bench.py builds it; about 1.08 M vertices) against the VGA point map dfa_tsdf_raycast_points makes of that volume.
  visible_vertices            flags only (one launch)
  visible_vertices + count    with the count (two launches)
  set_vertex_mask             the gather of N bytes through the plan's vertex order (a plan over C2's nodes and that cloud)
Items alternate inside every window; per item the median over the windows with [min, max] — the spread a difference has to
exceed.  The frame of DynFusion::operator() with DynFuParams::north_star_visible_only on and off is a host-adaptor figure:
DFA_HOST_PROFILE=1 prints the frame's stages (the added one is "visible vertices").
usage: python tools/visibility_timing.py [--config C2] [--windows 9] [--reps 100]"""
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
    ap.add_argument("--config", default="C2")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    cfg = synth.CONFIGS[args.config]
    intr = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, cam2vol, rinv = synth.volume_params(cfg)
    W, H, dim, k = cfg["width"], cfg["height"], cfg["dim"], cfg["k"]
    depth = torch.from_numpy(synth.depth_frame(cfg, 0).copy()).cuda()
    dists = torch.empty(depth.shape, dtype=torch.uint16, device="cuda")
    A.compute_dists(depth, dists, *intr)
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, *intr)
    tri, nv = (torch.from_numpy(t).cuda() for t in A.mc_default_tables())
    _, total = A.marching_cubes(vol, voxel, tri, nv, 1)
    n = int(total.item())
    soup, _ = A.marching_cubes(vol, voxel, tri, nv, n)
    cloud = A.transform_points(A.repack_points(soup[:n], 3), list(A._lib._aff12(vol2cam)))  # volume -> camera frame, packed N x 3
    pts = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    nrm = torch.empty_like(pts)
    A.tsdf_raycast_points(vol, voxel, trunc, cam2vol, rinv, *intr, synth.RAYCAST_STEP_FACTOR, synth.GRADIENT_DELTA_FACTOR, pts, nrm)
    z_tol = 2.0 * float(max(voxel))
    flags, count = A.visible_vertices(cloud, pts, *intr, z_tol, count=True)
    c = synth.canonical(cfg)
    nodes, node_dq, node_w = (torch.from_numpy(np.ascontiguousarray(c[x])).cuda() for x in ("node_pos", "node_dq", "node_w"))
    plan = A.Solver6(len(nodes), n, k)
    plan.set_problem(nodes, node_dq, node_w, cloud)
    items = [("visible_vertices", lambda: A.visible_vertices(cloud, pts, *intr, z_tol)),
             ("visible_vertices + count", lambda: A.visible_vertices(cloud, pts, *intr, z_tol, count=True)),
             ("set_vertex_mask", lambda: plan.set_vertex_mask(flags))]
    for _, fn in items:  # warm-up (the mask's plan memory is allocated by its first call)
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
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
    print(f"{args.config}: {n} vertices against a {W} x {H} map ({float((~torch.isnan(pts[..., 0])).float().mean().item()):.1%} hit), "
          f"{int(count.item())} visible (z_tol {z_tol:.4f} m); D {len(nodes)}, k {k}; {args.windows} windows x {args.reps} calls, "
          f"median [min, max] ms per call (the Python call included: the flags tensor is allocated per call)")
    for label, _ in items:
        print(f"  {label:28s} {np.median(ms[label]):7.4f} ms [{min(ms[label]):.4f}, {max(ms[label]):.4f}]")
    plan.close()


if __name__ == "__main__":
    main()
