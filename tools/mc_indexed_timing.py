"""Device-event timing of dfa_marching_cubes (the triangle soup) beside dfa_marching_cubes_indexed (every vertex once plus
an index list) on the same volume, fused from the synthetic depth frame (dynfu_amd/synth.py, frame 0, as bench.py builds it):
C2 (512^3, 512 MiB: more than the 256 MiB Infinity Cache, so HBM figures) and C4 (1024^3), each with and without the
occupancy map.

The yardstick of the indexed call is the soup call timed IN THE SAME RUN: the items alternate inside every window, after a
warm-up of each, every call writes into buffers of exactly its totals, and per item the median over the windows is printed
with [min, max], what it writes (16 B per point, 4 B per index), and indexed / soup as a ratio of the medians.
usage: python tools/mc_indexed_timing.py [--configs C2 C4] [--windows 7] [--reps 20]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dynfu_amd as A
from dynfu_amd import synth


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
    return vol, occ, voxel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["C2", "C4"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    A.load()
    L = A._lib
    lib = L.load()
    tri, nv = (torch.from_numpy(t).cuda() for t in A.mc_default_tables())
    for name in args.configs:
        vol, occ, voxel = fused_volume(name)
        X = Y = Z = vol.shape[0]
        _, _, t = A.marching_cubes_indexed(vol, voxel, tri, nv, 0, 0)
        nvert, nidx = (int(v) for v in t.cpu())
        soup = torch.empty((max(nidx, 1), 4), dtype=torch.float32, device="cuda")
        verts = torch.empty((max(nvert, 1), 4), dtype=torch.float32, device="cuda")
        idx = torch.empty((max(nidx, 1),), dtype=torch.int32, device="cuda")
        tot = torch.zeros((2,), dtype=torch.int32, device="cuda")
        cs = L._farr(voxel, 3)

        def soup_call(use_occ):
            if use_occ:
                L._check(lib.dfa_marching_cubes_occ(L._dev(vol), L._dev(occ), X, Y, Z, cs, L._dev(tri), L._dev(nv), L._dev(soup),
                                                    nidx, L._dev(tot), L._stream()))
            else:
                L._check(lib.dfa_marching_cubes(L._dev(vol), X, Y, Z, cs, L._dev(tri), L._dev(nv), L._dev(soup), nidx,
                                                L._dev(tot), L._stream()))

        def indexed_call(use_occ):
            L._check(lib.dfa_marching_cubes_indexed(L._dev(vol), L._dev(occ) if use_occ else None, X, Y, Z, cs, L._dev(tri),
                                                    L._dev(nv), L._dev(verts), nvert, L._dev(idx), nidx, L._dev(tot),
                                                    L._stream()))

        items = [  # label, call, bytes written
            ("soup", lambda: soup_call(False), 16.0 * nidx),
            ("indexed", lambda: indexed_call(False), 16.0 * nvert + 4.0 * nidx),
            ("soup, occupancy map", lambda: soup_call(True), 16.0 * nidx),
            ("indexed, occupancy map", lambda: indexed_call(True), 16.0 * nvert + 4.0 * nidx),
        ]
        for _, fn, _ in items:  # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert [int(v) for v in tot.cpu()] == [nvert, nidx]
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
        print(f"{name}: {X}^3 volume, {nidx} soup vertices = indices, {nvert} distinct vertices ({nidx / max(nvert, 1):.2f} x); "
              f"{args.windows} windows x {args.reps} calls, median [min, max] ms")
        med = {label: float(np.median(v)) for label, v in ms.items()}
        for label, _, nbytes in items:
            base = med["soup, occupancy map" if "occupancy" in label else "soup"]
            print(f"  {label:24s} {med[label]:7.3f} ms [{min(ms[label]):.3f}, {max(ms[label]):.3f}]  writes {nbytes / 1e6:7.1f} MB"
                  f"  {med[label] / base:5.2f} x the soup call")
        del vol, occ, soup, verts, idx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
