"""What the growing canonical model costs (DynFuParams::north_star_regrow_canonical), in two parts.

1. The extraction.  dfa_marching_cubes_indexed_min_weight (floor 2 and floor 1) beside dfa_marching_cubes_indexed on the SAME
   canonical volume: 512^3, two synthetic VGA depth frames fused into it (dynfu_amd/synth.py frames 0 and 1, so weights 1 and
   2 coexist), with and without the occupancy map.  Device events; the items alternate inside every window after a warm-up of
   each, every call writes into buffers of exactly its totals; per item the median over the windows with [min, max] and the
   ratio to the plain call.
2. The frame.  dynfu_amd/host/build/sequence_bench (a child process of its own: this process holds no GPU memory by then) over
   the synthetic sequence at the same settings in three modes run one after the other: the north-star sequence with
   north_star_fuse_canonical (the path there was before), with fuse_unsupported_rigid added, and with
   north_star_regrow_canonical added to those.  Per mode: the median frame after the first `--skip` frames, [min, max], and
   the canonical cloud's size by frame.

usage: python tools/regrow_timing.py [--config C2] [--windows 7] [--reps 20] [--frames 14] [--skip 4] [--part extraction|frame]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def extraction(name, windows, reps):
    import torch

    import dynfu_amd as A
    from dynfu_amd import synth
    A.load()
    L = A._lib
    lib = L.load()
    cfg = synth.CONFIGS[name]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    dim = cfg["dim"]
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    occ = A.tsdf_occupancy(vol)
    dists = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
    for f in (0, 1):
        A.compute_dists(torch.from_numpy(synth.depth_frame(cfg, f).copy()).cuda(), dists, fx, fy, cx, cy)
        (A.tsdf_clear_integrate if f == 0 else A.tsdf_integrate)(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx,
                                                                cy, occupancy=occ)
    w = (vol.view(torch.int32) >> 16) & 0xFFFF
    print(f"{name}: {dim}^3 canonical volume of two fused frames: {int((w == 1).sum())} voxels of weight 1, {int((w == 2).sum())} of weight 2")
    del w
    tri, nv = (torch.from_numpy(t).cuda() for t in A.mc_default_tables())
    cs = L._farr(voxel, 3)
    tot = torch.zeros((2,), dtype=torch.int32, device="cuda")
    items = []
    for label, floor in (("plain", None), ("floor 1", 1), ("floor 2", 2)):
        _, _, t = A.marching_cubes_indexed(vol, voxel, tri, nv, 0, 0, min_weight=floor or 1)
        nvert, nidx = (int(v) for v in t.cpu())
        verts = torch.empty((max(nvert, 1), 4), dtype=torch.float32, device="cuda")
        idx = torch.empty((max(nidx, 1),), dtype=torch.int32, device="cuda")
        for use_occ in (False, True):
            def call(floor=floor, verts=verts, idx=idx, nvert=nvert, nidx=nidx, use_occ=use_occ):
                head = (L._dev(vol), L._dev(occ) if use_occ else None, dim, dim, dim, cs, L._dev(tri), L._dev(nv))
                tail = (L._dev(verts), nvert, L._dev(idx), nidx, L._dev(tot), L._stream())
                if floor is None:
                    L._check(lib.dfa_marching_cubes_indexed(*head, *tail))
                else:
                    L._check(lib.dfa_marching_cubes_indexed_min_weight(*head, floor, *tail))
            items.append((label + (", occupancy map" if use_occ else ""), call, nvert, nidx))
    for _, fn, _, _ in items:  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {label: [] for label, _, _, _ in items}
    for _ in range(windows):
        for label, fn, _, _ in items:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[label].append(e0.elapsed_time(e1) / reps)
    med = {label: float(np.median(v)) for label, v in ms.items()}
    print(f"  {windows} windows x {reps} calls, median [min, max] ms")
    for label, _, nvert, nidx in items:
        base = med["plain, occupancy map" if "occupancy" in label else "plain"]
        print(f"  {label:26s} {med[label]:7.3f} ms [{min(ms[label]):.3f}, {max(ms[label]):.3f}]  {nvert:8d} vertices {nidx:9d} indices"
              f"  {med[label] / base:5.3f} x the plain call")
    del vol, occ
    torch.cuda.empty_cache()


def frame(name, frames, skip):
    from dynfu_amd import build as B, synth
    exe = B.SEQ_BENCH
    if not os.path.exists(exe):
        sys.exit("dynfu_amd/host/build/sequence_bench is not built (python -c 'import __graft_entry__ as g; g.build()')")
    cfg = synth.CONFIGS[name]
    W, H, dim = cfg["width"], cfg["height"], cfg["dim"]
    with tempfile.TemporaryDirectory() as d:
        raw = os.path.join(d, "frames.u16")
        np.stack([synth.depth_frame(cfg, f) for f in range(frames)]).astype("<u2").tofile(raw)
        print(f"{name}: {frames} synthetic {W}x{H} depth frames, {dim}^3 volume; ms per frame inside DynFusion::operator(), "
              f"frames {skip}.. counted")
        for mode in ("northstar+fuse", "northstar+fuse+rigid", "northstar+regrow", "northstar+fuse"):
            r = subprocess.run([exe, raw, str(W), str(H), str(frames), str(dim), mode], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(f"  {mode}: failed: {r.stderr[-500:]}")
                return 1
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            t = rec["frame_ms"][skip:]
            print(f"  {mode:22s} median {float(np.median(t)):8.3f} ms [{min(t):.3f}, {max(t):.3f}]  nodes {rec['nodes_first']} -> "
                  f"{rec['nodes_last']}, valid rows {rec['valid_rows']}, skipped {rec['regrow_skipped']}")
            print(f"    canonical vertices by frame: {rec['canonical_vertices_by_frame']}")
            print(f"    frame ms: {[round(v, 2) for v in rec['frame_ms']]}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--part", choices=["extraction", "frame"])
    a = ap.parse_args()
    if a.part != "frame":
        extraction(a.config, a.windows, a.reps)
    if a.part != "extraction":
        return frame(a.config, a.frames, a.skip)
    return 0


if __name__ == "__main__":
    sys.exit(main())
