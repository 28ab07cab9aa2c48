"""Device-event timing of dfa_tsdf_integrate_warped and dfa_tsdf_integrate_warped6 (both modes each) beside
dfa_tsdf_integrate of the same frame, at 512^3 with 2 k nodes on the surface, VGA, k = 8 (dynfu_amd/synth.py: the C2 scene; the
nodes are its canonical nodes taken to the volume's frame, each with a translation of up to a centimetre; for the north-star
call the same nodes stay in the camera frame, where the scene has them — vol2node is the volume's pose, node2cam the identity).

The items alternate inside every window, after a warm-up of each; per item the median over the windows [min, max].  Beside
the times: the share of bricks (64 x 4 x 1 voxels, a workgroup of the sweep) the support pre-pass marks — restated here in
numpy from the nodes, the flags themselves are the library's scratch — and, to say where the time goes, dfa_warp_to_live
(the same search and blend, one point per lane, nothing else) over the positions of every voxel of the marked bricks.
usage: python tools/warped_integrate_timing.py [--config C2] [--k 8] [--windows 7] [--reps 10]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dynfu_amd as A
from dynfu_amd import synth

BRICK = (64, 4, 1)  # csrc/warped_bricks.hpp: WBX, WBY, WBZ


def marked_bricks(dim, voxel, nodes, w_max):
    """the bricks whose box of voxel positions comes within w_max of a node (csrc/tsdf_warped.hip: mark_bricks_kernel,
    without the rounding margins of csrc/warped_mark_device.hpp: mark_radius): bool (bz, by, bx)"""
    nb = [-(-dim // b) for b in BRICK]
    lo = [np.arange(n) * b * voxel for n, b in zip(nb, BRICK)]
    hi = [np.minimum(np.arange(n) * b + b - 1, dim - 1) * voxel for n, b in zip(nb, BRICK)]
    out = np.zeros((nb[2], nb[1], nb[0]), bool)
    for s in range(0, len(nodes), 16):
        g = nodes[s:s + 16].astype(np.float64)
        d = [np.maximum(np.maximum(lo[c][None, :] - g[:, c:c + 1], g[:, c:c + 1] - hi[c][None, :]), 0.0) for c in range(3)]
        d2 = d[2][:, :, None, None] ** 2 + d[1][:, None, :, None] ** 2 + d[0][:, None, None, :] ** 2
        out |= (d2 <= w_max * w_max).any(axis=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    A.load()
    cfg = synth.CONFIGS[args.config]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    dim, D, k = cfg["dim"], cfg["D"], args.k
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dists = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
    A.compute_dists(dev(synth.depth_frame(cfg, 0).copy()), dists, fx, fy, cx, cy)
    nxt = torch.empty_like(dists)
    A.compute_dists(dev(synth.depth_frame(cfg, 1).copy()), nxt, fx, fy, cx, cy)
    c = synth.canonical(cfg)
    rng = np.random.default_rng(7)
    nodes = (c["node_pos"] - np.array(synth.VOLUME_POSE_T, np.float32)).astype(np.float32)  # camera frame -> volume frame
    dq = c["node_dq"].copy()
    dq[:, 5:8] = 0.5 * rng.uniform(-0.01, 0.01, (D, 3))  # real = identity: dual = (0, t) / 2
    d_nodes, d_dq, d_w = dev(nodes), dev(dq), dev(c["node_w"])
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)  # frame 0: the canonical volume

    marked = marked_bricks(dim, float(voxel[0]), nodes, float(c["node_w"].max()))
    bz, by, bx = np.nonzero(marked)
    # every voxel position of the marked bricks, for the search + blend alone
    oz, oy, ox = np.meshgrid(np.arange(BRICK[2]), np.arange(BRICK[1]), np.arange(BRICK[0]), indexing="ij")
    pts = np.stack([(bx[:, None] * BRICK[0] + ox.ravel()[None, :]).ravel(), (by[:, None] * BRICK[1] + oy.ravel()[None, :]).ravel(),
                    (bz[:, None] * BRICK[2] + oz.ravel()[None, :]).ravel()], 1).astype(np.float32) * voxel[None, :]
    d_pts = dev(pts)
    flags = A.unsupported_vertices(d_nodes, d_w, k, d_pts)
    supported = int((flags == 0).sum().item())

    def warped(mode):
        return lambda: A.tsdf_integrate_warped(vol, nxt, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, d_nodes, d_dq,
                                               d_w, k, unsupported=mode)

    # the north-star call: the same volume, frame and nodes, the nodes in the camera frame (the volume's pose takes a voxel
    # there; the pose is a translation, so the transforms are the same numbers) and the camera where it was
    d_nodes6 = dev((nodes.astype(np.float64) + np.asarray(vol2cam, np.float64)[9:12]).astype(np.float32))

    def warped6(mode):
        return lambda: A.tsdf_integrate_warped6(vol, nxt, voxel, trunc, synth.MAX_WEIGHT, vol2cam, None, fx, fy, cx, cy, d_nodes6,
                                                d_dq, d_w, min(k, 8), unsupported=mode)

    items = [
        ("tsdf_integrate (rigid, same frame)", lambda: A.tsdf_integrate(vol, nxt, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)),
        ("tsdf_integrate_warped skip", warped("skip")),
        ("tsdf_integrate_warped rigid", warped("rigid")),
        ("tsdf_integrate_warped6 skip", warped6("skip")),
        ("tsdf_integrate_warped6 rigid", warped6("rigid")),
        ("warp_to_live, voxels of marked bricks", lambda: A.warp_to_live(d_nodes, d_dq, d_w, k, d_pts)),
    ]
    for _, fn in items:  # warm-up
        for _ in range(3):
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
    print(f"{args.config}: {dim}^3 volume, {cfg['width']}x{cfg['height']} depth, D = {D} nodes (w = {float(c['node_w'].max()):.3f} m), "
          f"k = {k}; {args.windows} windows x {args.reps} calls, median [min, max] ms")
    print(f"  bricks marked: {int(marked.sum())} of {marked.size} ({marked.mean():.2%}); their voxels: {len(pts)}, "
          f"{supported} supported ({supported / dim ** 3:.2%} of the volume)")
    for label, _ in items:
        print(f"  {label:40s} {np.median(ms[label]):8.3f} ms [{min(ms[label]):.3f}, {max(ms[label]):.3f}]")


if __name__ == "__main__":
    main()
