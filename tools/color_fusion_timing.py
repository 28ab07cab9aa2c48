"""Device-event timing of colour fusion (dfa_tsdf_integrate_warped6_color, dfa_color_sample) beside the plain north-star
sweeps, in ONE run: the set-up of tools/knn_field_timing.py — 512^3 with 2 k nodes on the surface, VGA, k = 8
(dynfu_amd/synth.py: the C2 scene; the nodes in the camera frame, vol2node = the volume's pose), each node with a translation
of up to a centimetre, a seeded random colour image.

Per mode (SKIP / RIGID) and neighbour source (searching / from the k-NN field), four items: the fused call; the plain
dfa_tsdf_integrate_warped6[_field] — the parent's kernel —; the colours-only call (volume == NULL); and once,
dfa_color_sample on the welded cloud of the fused volume.  The items alternate inside every window, after a warm-up of each;
per item the median over the windows [min, max].  Before anything is timed the fused call's volume is compared with the plain
call's, bit for bit, and the colours-only colour volume with the fused one.

The bar is relative, measured in this run: the fused call must cost less than the plain call plus the colours-only call
(otherwise fusing colour into the sweep has no case); its excess over the plain call is printed as it is.

Run without --only, the tool starts one child process per (mode, source) pair, each under a time limit of its own, and stops
at the first that fails, faults or runs out of time: nothing more is started on the device after that.  A pair's three calls
are always timed in ONE process, alternating.
usage: python tools/color_fusion_timing.py [--config C2] [--k 8] [--windows 7] [--reps 10] [--step-timeout 240]
       python tools/color_fusion_timing.py --only rigid:field       (one pair, in this process; "all": every pair in this process)"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import dynfu_amd as A
from dynfu_amd import synth


PAIRS = [("skip", "search"), ("skip", "field"), ("rigid", "search"), ("rigid", "field")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-sample", action="store_true", help="leave dfa_color_sample out")
    ap.add_argument("--config", default="C2")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, help="MODE:SOURCE (skip|rigid : search|field), or all")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per child process")
    args = ap.parse_args()
    if args.only is None:
        status = 0
        for i, pair in enumerate(PAIRS):
            cmd = [sys.executable, os.path.abspath(__file__), "--config", args.config, "--k", str(args.k), "--windows", str(args.windows),
                   "--reps", str(args.reps), "--only", "%s:%s" % pair] + ([] if i == 0 else ["--no-sample"])
            try:
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            except subprocess.TimeoutExpired:
                print("%s:%s ran out of its %d s: nothing more is started" % (pair + (args.step_timeout,)))
                return 124
            if rc not in (0, 1):  # (1: the pair ran and missed the bar; anything else: stop here)
                print("%s:%s ended with status %d: nothing more is started" % (pair + (rc,)))
                return rc
            status |= rc
        return status
    pairs = PAIRS if args.only == "all" else [tuple(args.only.split(":"))]
    assert all(p in PAIRS for p in pairs), args.only
    A.load()
    cfg = synth.CONFIGS[args.config]
    fx, fy, cx, cy = synth.intrinsics(cfg)
    voxel, trunc, vol2cam, _, _ = synth.volume_params(cfg)
    dim, D, k = cfg["dim"], cfg["D"], min(args.k, 8)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dists = torch.empty((cfg["height"], cfg["width"]), dtype=torch.uint16, device="cuda")
    A.compute_dists(dev(synth.depth_frame(cfg, 0).copy()), dists, fx, fy, cx, cy)
    nxt = torch.empty_like(dists)
    A.compute_dists(dev(synth.depth_frame(cfg, 1).copy()), nxt, fx, fy, cx, cy)
    c = synth.canonical(cfg)
    rng = np.random.default_rng(7)
    dq = c["node_dq"].copy()
    dq[:, 5:8] = 0.5 * rng.uniform(-0.01, 0.01, (D, 3))  # real = identity: dual = (0, t) / 2
    d_nodes, d_dq, d_w = dev(c["node_pos"]), dev(dq), dev(c["node_w"])  # (the camera frame)
    image = dev(rng.integers(0, 256, (cfg["height"], cfg["width"], 4), dtype=np.uint8))
    vol = torch.empty((dim, dim, dim), dtype=torch.int32, device="cuda")
    A.tsdf_clear_integrate(vol, dists, voxel, trunc, synth.MAX_WEIGHT, vol2cam, fx, fy, cx, cy)  # frame 0: the canonical volume
    colors = torch.zeros((dim, dim, dim), dtype=torch.int32, device="cuda")
    field = A.KnnField((dim, dim, dim), voxel, k, vol2node=vol2cam)
    field.build(d_nodes, d_w)

    def plain(mode, f, v=vol):
        return lambda: A.tsdf_integrate_warped6(v, nxt, voxel, trunc, synth.MAX_WEIGHT, vol2cam, None, fx, fy, cx, cy, d_nodes, d_dq, d_w, k,
                                                unsupported=mode, field=f)

    def fused(mode, f, v=vol, col=colors, with_tsdf=True):
        return lambda: A.tsdf_integrate_warped6_color(v if with_tsdf else None, col, image, nxt, voxel, trunc, synth.MAX_WEIGHT, 255, vol2cam,
                                                      None, fx, fy, cx, cy, d_nodes, d_dq, d_w, k, unsupported=mode, field=f)

    # fused = plain in the volume, colours only = fused in the colours, bit for bit, on copies
    coloured = {}
    for mode, source in pairs:
        for f in ((None,) if source == "search" else (field,)):
            a, b, ca, cb = vol.clone(), vol.clone(), colors.clone(), colors.clone()
            plain(mode, f, a)(), fused(mode, f, b, ca)(), fused(mode, f, None, cb, with_tsdf=False)()
            assert torch.equal(a, b) and not torch.equal(a, vol), (mode, f is not None)
            assert torch.equal(ca, cb), (mode, f is not None)
            coloured[mode] = int((ca != 0).sum())

    # the welded cloud of the fused volume, for dfa_color_sample
    tri, nv = A.mc_default_tables()
    _, _, totals = A.marching_cubes_indexed(vol, voxel, dev(tri), dev(nv), 0, 0)
    n_v, n_i = (int(t) for t in totals.cpu())
    verts, _, _ = A.marching_cubes_indexed(vol, voxel, dev(tri), dev(nv), n_v, n_i)
    fused("rigid", field)()  # colours for the sample to read

    items = []
    for mode, name in pairs:
        for f in ((None,) if name == "search" else (field,)):
            items += [("%-5s %-6s fused" % (mode, name), fused(mode, f)), ("%-5s %-6s plain" % (mode, name), plain(mode, f)),
                      ("%-5s %-6s colours only" % (mode, name), fused(mode, f, with_tsdf=False))]
    if not args.no_sample:
        items.append(("color_sample, %d vertices" % n_v, lambda: A.color_sample(colors, voxel, verts)))
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

    print(f"{args.config}: {dim}^3 volume, {cfg['width']}x{cfg['height']} frame, D = {D} nodes, k = {k}; {args.windows} windows x "
          f"{args.reps} calls, median [min, max] ms; coloured voxels after one call: {coloured}")
    for label, _ in items:
        print(f"  {label:34s} {np.median(ms[label]):8.3f} ms [{min(ms[label]):.3f}, {max(ms[label]):.3f}]")
    ok = True
    for mode, name in pairs:
        for _ in (0,):
            f, p, o = (float(np.median(ms["%-5s %-6s %s" % (mode, name, what)])) for what in ("fused", "plain", "colours only"))
            verdict = "ok" if f < p + o else "NO CASE"
            ok &= f < p + o
            print(f"  {mode:5s} {name:6s}: fused {f:.3f} vs plain + colours only {p + o:.3f} ms ({verdict}); excess over plain "
                  f"{f - p:+.3f} ms ({(f / p - 1):+.1%})")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
