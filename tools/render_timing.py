"""Device-event timing of the model views: per launch, on volumes fused from the synthetic depth frame
(dynfu_amd/synth.py, frame 0, as bench.py builds them), from the configuration's own camera — C2 (512^3, VGA) and C4
(1024^3, 1280 x 720):
  (a) dfa_tsdf_raycast_points alone                     (the two float4 maps: 32 B per pixel written)
  (b) (a) + dfa_render_image_points                     (what the reference's renderImage(image, pose, flag) does)
  (c) dfa_tsdf_raycast_render, Phong                    (the fused launch: 4 B per pixel written)
  (d) dfa_render_image_points alone, with the rate its 36 B per pixel imply
  (e) dfa_tsdf_raycast_render, both views side by side
The items alternate inside every window, after a warm-up of each; per item the median over the windows is printed with
its minimum and maximum — the run-to-run spread a difference between two items has to exceed.
`--raycast-only` times (a) alone: the section that also runs on a checkout without the render entry points, for the
comparison of (c) with the raycast as it was before them.
usage: python tools/render_timing.py [--configs C2 C4] [--windows 11] [--reps 500] [--raycast-only]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dynfu_amd as A
from dynfu_amd import synth

HBM_PEAK = 8.0e12  # B/s (MI355X)
LIGHT = [0.4, -0.3, 0.2]


def fused_volume(name):
    cfg = synth.CONFIGS[name]
    intr = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, cam2vol, rinv = synth.volume_params(cfg)
    depth = torch.from_numpy(synth.depth_frame(cfg, 0).copy()).cuda()
    dists = torch.empty(depth.shape, dtype=torch.uint16, device="cuda")
    A.compute_dists(depth, dists, *intr)
    dim = cfg["dim"]
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, *intr)
    return vol, voxel, trunc, cam2vol, rinv, intr, cfg["width"], cfg["height"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["C2", "C4"])
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--raycast-only", action="store_true")
    args = ap.parse_args()
    A.load()
    for name in args.configs:
        vol, voxel, trunc, c2v, ri, intr, W, H = fused_volume(name)
        pts = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        nrm = torch.zeros_like(pts)
        img = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        img2 = torch.zeros((H, 2 * W, 4), dtype=torch.uint8, device="cuda")
        # the ctypes arguments are built once: per call the host then costs less than the shortest kernel here
        L = A._lib
        lib = L.load()
        dim = vol.shape[0]
        vs, aff, rinv9, light = L._farr(voxel, 3), L._aff12(c2v), L._farr(np.asarray(ri, np.float32).reshape(-1), 9), L._farr(LIGHT, 3)
        head = (L._dev(vol), dim, dim, dim, vs, trunc, aff, rinv9, *intr, synth.RAYCAST_STEP_FACTOR, synth.GRADIENT_DELTA_FACTOR)
        dp, dn, di, di2, st = L._dev(pts), L._dev(nrm), L._dev(img), L._dev(img2), L._stream()

        def raycast():
            L._check(lib.dfa_tsdf_raycast_points(*head, dp, W * 16, dn, W * 16, W, H, st))

        def shade():
            L._check(lib.dfa_render_image_points(dp, W * 16, dn, W * 16, W, H, light, di, W * 4, st))

        def raycast_then_shade():
            raycast()
            shade()

        def fused(mode, image, step):
            L._check(lib.dfa_tsdf_raycast_render(*head, W, H, light, mode, image, step, st))

        items = [("(a) raycast_points", raycast, None)]
        if not args.raycast_only:
            items += [("(b) raycast_points + render_image_points", raycast_then_shade, None),
                      ("(c) raycast_render, Phong", lambda: fused(A.RENDER_PHONG, di, W * 4), None),
                      ("(d) render_image_points", shade, 36.0 * W * H),
                      ("(e) raycast_render, both views", lambda: fused(A.RENDER_BOTH, di2, W * 8), None)]
        for _, fn, _ in items:  # warm-up
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        if not args.raycast_only:  # what is timed is what the tests compare
            raycast_then_shade()
            two = img.clone()
            fused(A.RENDER_PHONG, di, W * 4)
            assert torch.equal(two, img), "the fused launch and the two launches disagree"
        ms = {label: [] for label, _, _ in items}
        for _ in range(args.windows):
            for label, fn, _ in items:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                ms[label].append(e0.elapsed_time(e1) / args.reps)
        hits = float((~torch.isnan(pts[..., 0])).float().mean().item())
        print(f"{name}: {vol.shape[0]}^3 volume, {W} x {H} rays, {hits:.1%} hit; {args.windows} windows x {args.reps} launches, "
              f"median [min, max] ms per launch")
        for label, _, nbytes in items:
            m = np.median(ms[label])
            rate = "" if nbytes is None else f"  {nbytes / 1e6:6.1f} MB  {nbytes / (m * 1e-3) / 1e9:6.0f} GB/s  {nbytes / (m * 1e-3) / HBM_PEAK:5.1%} of 8 TB/s"
            print(f"  {label:44s} {m:7.4f} ms [{min(ms[label]):.4f}, {max(ms[label]):.4f}]{rate}")
        del vol, pts, nrm, img, img2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
