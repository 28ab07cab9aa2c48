"""Device-event timing of the k-NN field (dfa_knn_field_*) and of the warped integrations served from it beside the searching
calls, in ONE run: the set-up of tools/warped_integrate_timing.py — 512^3 with 2 k nodes on the surface, VGA, k = 8
(dynfu_amd/synth.py: the C2 scene; the nodes in the volume's frame for dfa_tsdf_integrate_warped, in the camera frame with
vol2node = the volume's pose for dfa_tsdf_integrate_warped6), each node with a translation of up to a centimetre.

Items: the four searching calls (two warp fields x SKIP / RIGID), the four cached ones (all eight calls run kernels of
csrc/tsdf_warped.hip over the one body of csrc/warped_sweep_device.hpp; build and append are csrc/knn_field.hip), dfa_tsdf_integrate of the same frame
and dfa_warp_to_live_graph over the voxels of the stored bricks (the blend from stored ids, one point per lane, nothing
else) as yardsticks.  They alternate inside every window, after a warm-up of each; per item the median over the windows
[min, max].  Then, one call per window each: dfa_knn_field_build of both fields, and dfa_knn_field_append of the last 16
nodes to a field built on the others — events around the call, which waits on the stream once inside.  And the fields'
sizes.  Before anything is timed the cached volumes are compared with the searching ones, bit for bit.
usage: python tools/knn_field_timing.py [--config C2] [--k 8] [--windows 7] [--reps 10] [--new-nodes 16]"""
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
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--new-nodes", type=int, default=16)
    args = ap.parse_args()
    A.load()
    cfg = synth.CONFIGS[args.config]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    dim, D, k = cfg["dim"], cfg["D"], args.k
    k6 = min(k, 8)
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
    d_nodes6 = dev((nodes.astype(np.float64) + np.asarray(vol2cam, np.float64)[9:12]).astype(np.float32))
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)  # frame 0: the canonical volume

    field = A.KnnField((dim, dim, dim), voxel, k)
    field.build(d_nodes, d_w)
    field6 = A.KnnField((dim, dim, dim), voxel, k6, vol2node=vol2cam)
    field6.build(d_nodes6, d_w)

    def warped(mode, f, v=vol):
        return lambda: A.tsdf_integrate_warped(v, nxt, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, d_nodes, d_dq, d_w, k,
                                               unsupported=mode, field=f)

    def warped6(mode, f, v=vol):
        return lambda: A.tsdf_integrate_warped6(v, nxt, voxel, trunc, synth.MAX_WEIGHT, vol2cam, None, fx, fy, cx, cy, d_nodes6, d_dq,
                                                d_w, k6, unsupported=mode, field=f)

    # cached = searching, bit for bit, on copies of the canonical volume
    for make, f in ((warped, field), (warped6, field6)):
        for mode in ("skip", "rigid"):
            a, b = vol.clone(), vol.clone()
            make(mode, None, a)(), make(mode, f, b)()
            assert torch.equal(a, b), (make.__name__, mode)
            assert not torch.equal(a, vol)

    # the voxels of the stored bricks (of the reference-mode field) and their rows, for the blend alone
    z, y, x = np.meshgrid(np.arange(dim), np.arange(0, dim, 4), np.arange(0, dim, 64), indexing="ij")
    corners = dev(np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32))
    stored = (field.lookup(corners)[:, 0] >= 0).cpu().numpy()
    oy, ox = np.meshgrid(np.arange(4), np.arange(64), indexing="ij")
    base = corners.cpu().numpy()[stored]
    vox = np.stack([(base[:, None, 0] + ox.ravel()[None, :]).ravel(), (base[:, None, 1] + oy.ravel()[None, :]).ravel(),
                    np.repeat(base[:, 2], 256)], 1).astype(np.int32)
    d_vox = dev(vox)
    d_rows = field.lookup(d_vox)
    d_pts = dev(vox.astype(np.float32) * voxel[None, :])

    items = [
        ("tsdf_integrate (rigid, same frame)", lambda: A.tsdf_integrate(vol, nxt, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)),
        ("tsdf_integrate_warped skip", warped("skip", None)),
        ("tsdf_integrate_warped skip, field", warped("skip", field)),
        ("tsdf_integrate_warped rigid", warped("rigid", None)),
        ("tsdf_integrate_warped rigid, field", warped("rigid", field)),
        ("tsdf_integrate_warped6 skip", warped6("skip", None)),
        ("tsdf_integrate_warped6 skip, field", warped6("skip", field6)),
        ("tsdf_integrate_warped6 rigid", warped6("rigid", None)),
        ("tsdf_integrate_warped6 rigid, field", warped6("rigid", field6)),
        ("warp_to_live_graph, voxels of stored bricks", lambda: A.warp_to_live_graph(d_nodes, d_dq, d_w, d_rows, d_pts)),
    ]
    for _, fn in items:  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {label: [] for label, _ in items}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    for _ in range(args.windows):
        for label, fn in items:
            ms[label].append(timed(fn, args.reps))

    # build and append: one call per window (each waits on the stream once inside)
    part = D - args.new_nodes
    once = {"knn_field_build": [], "knn_field_build, vol2node": [], "knn_field_append, %d nodes" % args.new_nodes: [],
            "knn_field_append, %d nodes, vol2node" % args.new_nodes: []}
    scratch, scratch6 = A.KnnField((dim, dim, dim), voxel, k), A.KnnField((dim, dim, dim), voxel, k6, vol2node=vol2cam)
    for w in range(args.windows + 1):  # (the first window warms up: allocations)
        row = [timed(lambda: scratch.build(d_nodes, d_w), 1), timed(lambda: scratch6.build(d_nodes6, d_w), 1)]
        scratch.build(d_nodes[:part], d_w[:part]), scratch6.build(d_nodes6[:part], d_w[:part])
        torch.cuda.synchronize()
        row += [timed(lambda: scratch.append(d_nodes, d_w), 1), timed(lambda: scratch6.append(d_nodes6, d_w), 1)]
        if w:
            for key, t in zip(once, row):
                once[key].append(t)
    assert scratch.info() == field.info() and torch.equal(scratch.lookup(d_vox), d_rows)

    print(f"{args.config}: {dim}^3 volume, {cfg['width']}x{cfg['height']} depth, D = {D} nodes (w = {float(c['node_w'].max()):.3f} m), "
          f"k = {k}; {args.windows} windows x {args.reps} calls, median [min, max] ms")
    for name, f in (("field", field), ("field, vol2node", field6)):
        i = f.info()
        print(f"  {name}: {i['stored_bricks']} of {i['total_bricks']} bricks stored ({i['stored_bricks'] / i['total_bricks']:.2%}), "
              f"{i['bytes'] / 2 ** 20:.1f} MiB of rows (k = {i['k']}), D = {i['D']}")
    print(f"  voxels of the stored bricks: {len(vox)} ({len(vox) / dim ** 3:.2%} of the volume)")
    for label, _ in items:
        print(f"  {label:46s} {np.median(ms[label]):8.3f} ms [{min(ms[label]):.3f}, {max(ms[label]):.3f}]")
    print(f"  one call per window, {args.windows} windows:")
    for label, v in once.items():
        print(f"  {label:46s} {np.median(v):8.3f} ms [{min(v):.3f}, {max(v):.3f}]")


if __name__ == "__main__":
    main()
