"""Device-event timing of the point-cloud extraction (dfa_tsdf_extract_cloud / _occ, dfa_tsdf_extract_normals) beside the
marching-cubes count sweep, on volumes fused from the synthetic depth frame (dynfu_amd/synth.py, frame 0, as bench.py
builds them): C2 (512^3, 512 MiB: more than the 256 MiB Infinity Cache, so HBM figures) and C4 (1024^3).

The items alternate inside every window, after a warm-up of each; per item the median over the windows is printed with
the points it produces, its algorithmic bytes — the volume (4 B per voxel), or for the _occ forms the boxes of the map
with a weight (2 KiB each, 32 x 2 x 8 voxels), plus 16 B per point written; for the normals 16 B per point read and
16 B per normal written (the trilinear fetches not counted) — the rate those bytes imply and its share of 8 TB/s.
usage: python tools/extract_timing.py [--configs C2 C4] [--windows 7] [--reps 20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dynfu_amd as A
from dynfu_amd import synth

HBM_PEAK = 8.0e12  # B/s (MI355X)


def fused_volume(name):
    cfg = synth.CONFIGS[name]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    depth = torch.from_numpy(synth.depth_frame(cfg, 0).copy()).cuda()
    dists = torch.empty(depth.shape, dtype=torch.uint16, device="cuda")
    A.compute_dists(depth, dists, fx, fy, cx, cy)
    dim = cfg["dim"]
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    occ = A.tsdf_occupancy(vol)
    A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy, occupancy=occ)
    return vol, occ, voxel, vol2cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["C2", "C4"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    A.load()
    tri, nv = (torch.from_numpy(t).cuda() for t in A.mc_default_tables())
    for name in args.configs:
        vol, occ, voxel, pose = fused_volume(name)
        dim = vol.shape[0]
        _, total = A.tsdf_extract_cloud(vol, voxel, pose, 0)
        n = int(total.item())
        pts, _ = A.tsdf_extract_cloud(vol, voxel, pose, n)
        pts = pts[:n].contiguous()
        rinv = np.eye(3, dtype=np.float32)  # (the synthetic volume pose is a translation)
        nrm = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        buf = torch.empty((max(n, 1), 4), dtype=torch.float32, device="cuda")
        tot = torch.zeros((1,), dtype=torch.int32, device="cuda")
        L = A._lib
        lib = L.load()
        X = Y = Z = dim
        vb = 4.0 * dim ** 3
        mapped = float((occ != 0).sum().item()) * 32 * 2 * 8 * 4
        vs, aff, ri = L._farr(voxel, 3), L._aff12(pose), L._farr(rinv.reshape(-1), 9)

        def cloud(cap, use_occ):
            if use_occ:
                L._check(lib.dfa_tsdf_extract_cloud_occ(L._dev(vol), L._dev(occ), X, Y, Z, vs, aff,
                                                        L._dev(buf) if cap else None, cap, L._dev(tot), L._stream()))
            else:
                L._check(lib.dfa_tsdf_extract_cloud(L._dev(vol), X, Y, Z, vs, aff, L._dev(buf) if cap else None, cap,
                                                    L._dev(tot), L._stream()))

        def normals():
            L._check(lib.dfa_tsdf_extract_normals(L._dev(vol), X, Y, Z, vs, aff, ri, synth.GRADIENT_DELTA_FACTOR,
                                                  L._dev(pts), n, L._dev(nrm), L._stream()))

        items = [  # label, call, points, bytes
            ("extract count-only", lambda: cloud(0, False), n, vb),
            ("extract + emit", lambda: cloud(n, False), n, vb + 16.0 * n),
            ("extract_occ count-only", lambda: cloud(0, True), n, mapped),
            ("extract_occ + emit", lambda: cloud(n, True), n, mapped + 16.0 * n),
            ("marching cubes count sweep", lambda: A.marching_cubes(vol, voxel, tri, nv, 0), None, vb),
            ("marching cubes_occ count sweep", lambda: A.marching_cubes(vol, voxel, tri, nv, 0, occupancy=occ), None, mapped),
            ("extract_normals", normals, n, 32.0 * n),
        ]
        for _, fn, _, _ in items:  # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {label: [] for label, _, _, _ in items}
        for _ in range(args.windows):
            for label, fn, _, _ in items:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                ms[label].append(e0.elapsed_time(e1) / args.reps)
        print(f"{name}: {dim}^3 volume ({vb / 2**20:.0f} MiB), {n} points, map: {mapped / vb:.1%} of the volume in boxes "
              f"with a weight; {args.windows} windows x {args.reps} calls, median [min, max] ms")
        for label, _, pts_n, nbytes in items:
            m = np.median(ms[label])
            rate = nbytes / (m * 1e-3)
            p = "" if pts_n is None else f"{pts_n:>9d} pts"
            print(f"  {label:32s} {m:7.3f} ms [{min(ms[label]):.3f}, {max(ms[label]):.3f}] {p:>13s}  "
                  f"{nbytes / 1e6:8.1f} MB  {rate / 1e9:7.0f} GB/s  {rate / HBM_PEAK:6.1%} of 8 TB/s")
        del vol, occ, pts, nrm, buf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
