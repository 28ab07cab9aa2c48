"""What the rigid pre-alignment of north-star mode costs (DynFuParams::north_star_rigid_prealign), in four parts.

1. The kernel.  dfa_rigid_sums_cloud over clouds of N = 185 693 and N = 1 083 909 vertices (the canonical clouds of the C2 and
   C4 bench configurations) against VGA maps: the vertex / normal maps of synthetic frame 1 (dynfu_amd/synth.py), the cloud
   the valid pixels of frame 0's maps repeated up to N, a small rigid estimate.  Device events; the items alternate inside
   every window after a warm-up of each; per item the median over the windows with [min, max] and the matched count.
2. The loop (dfa_rigid_align_cloud, DynFuParams::rigid_prealign_device) on the same clouds and maps, from the identity, in one
   session: the host loop's device work and read-backs — 10 x (dfa_rigid_sums_cloud, a 28-word read-back; the pose held, no
   6 x 6 solve: a lower bound of the host loop) —, the device loop of 10 iterations at full resolution without a stop, and
   the default schedule ({16, 4, 1} x {4, 5, 10}, stop 1e-5).  Host wall clock around a synchronised region (the host loop's
   time IS its synchronisations); the items alternate inside every window after a warm-up of each.
3. The whole NorthStarSolver::alignRigid inside a frame, read-backs included, for the host loop of 10 iterations, the device
   loop of the same 10 and the default schedule: sequence_bench with "+prealign", "+prealign+device10", "+prealign+device"
   as child processes under DFA_HOST_PROFILE=1, whose stage clock synchronises the device at every mark and prints the
   stage's wall time; the median over the frames after the first `--skip`.
4. The frame.  sequence_bench (child processes; this process holds no GPU memory by then) over the synthetic sequence with
   the step off, with the host loop and with the two device loops, alternating, twice each: the median frame after the first
   `--skip` frames, [min, max].

usage: python tools/rigid_align_timing.py [--config C2] [--windows 7] [--reps 20] [--frames 14] [--skip 4] [--part kernel|loop|align|frame]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SIZES = (185693, 1083909)
ESTIMATE = ([0.2, 1.0, 0.1], 0.01, [0.004, -0.003, 0.006])  # 0.6 degrees, 8 mm


def kernel(name, windows, reps):
    import torch

    import dynfu_amd as A
    from dynfu_amd import synth
    A.load()
    cfg = synth.CONFIGS[name]
    intr = synth.intrinsics(cfg)
    maps = []
    for f in (0, 1):
        depth = torch.from_numpy(synth.depth_frame(cfg, f).copy()).cuda()
        maps.append(A.compute_points_normals(depth, *intr))
    (v0, n0), (vmap, nmap) = maps
    ok = ~(torch.isnan(v0[..., 0]) | torch.isnan(n0[..., 0]))
    base_v, base_n = v0[ok][:, :3].contiguous(), n0[ok][:, :3].contiguous()
    axis, ang, t = ESTIMATE
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    aff = np.concatenate([R.reshape(-1), t]).astype(np.float32)
    print(f"{name}: {cfg['width']}x{cfg['height']} maps, {len(base_v)} valid pixels of frame 0 repeated up to N; "
          f"{windows} windows x {reps} calls, median [min, max] ms")
    items = []
    for N in SIZES:
        pick = torch.arange(N, device="cuda") % len(base_v)
        v, n = base_v[pick].contiguous(), base_n[pick].contiguous()
        sums, matched = A.rigid_sums_cloud(v, n, aff, vmap, nmap, intr, 0.1, 0.5)
        lib, L = A._lib.load(), A._lib
        out = torch.empty(28, dtype=torch.float32, device="cuda")
        args = (L._dev(v), L._dev(n), 3, N, L._aff12(aff), L._dev(vmap), vmap.stride(0) * 4, L._dev(nmap), nmap.stride(0) * 4,
                cfg["width"], cfg["height"], *[float(x) for x in intr], 0.1, 0.5, L._dev(out), L._dev(out[27:].view(torch.int32)))

        def call(args=args, keep=(v, n, out)):
            L._check(lib.dfa_rigid_sums_cloud(*args, L._stream()))
        items.append((N, call, matched))
    for _, fn, _ in items:  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {N: [] for N, _, _ in items}
    for _ in range(windows):
        for N, fn, _ in items:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[N].append(e0.elapsed_time(e1) / reps)
    for N, _, matched in items:
        # bytes the algorithm needs: 24 per vertex (position and normal), 32 per matched-or-tested gather (two float4 pixels)
        gb = (24.0 * N + 32.0 * N) / 1e9
        med = float(np.median(ms[N]))
        print(f"  N = {N:8d}  {med:7.4f} ms [{min(ms[N]):.4f}, {max(ms[N]):.4f}]  matched {matched}  "
              f"({gb / (med * 1e-3):.0f} GB/s of the {gb * 1e3:.1f} MB the call reads at most)")


def loop(name, windows, reps):
    import time

    import torch

    import dynfu_amd as A
    from dynfu_amd import synth
    A.load()
    cfg = synth.CONFIGS[name]
    intr = synth.intrinsics(cfg)
    maps = []
    for f in (0, 1):
        depth = torch.from_numpy(synth.depth_frame(cfg, f).copy()).cuda()
        maps.append(A.compute_points_normals(depth, *intr))
    (v0, n0), (vmap, nmap) = maps
    ok = ~(torch.isnan(v0[..., 0]) | torch.isnan(n0[..., 0]))
    base_v, base_n = v0[ok][:, :3].contiguous(), n0[ok][:, :3].contiguous()
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    lib, L = A._lib.load(), A._lib
    import ctypes as C
    print(f"{name}: {cfg['width']}x{cfg['height']} maps, the loop from the identity; {windows} windows x {reps} loops, host wall clock "
          f"around a synchronised region, median [min, max] ms per loop")
    for N in SIZES:
        pick = torch.arange(N, device="cuda") % len(base_v)
        v, n = base_v[pick].contiguous(), base_n[pick].contiguous()
        out = torch.empty(28, dtype=torch.float32, device="cuda")
        report = torch.empty(C.sizeof(L.RigidAlignReport), dtype=torch.uint8, device="cuda")
        head = (L._dev(v), L._dev(n), 3, N, L._aff12(ident), L._dev(vmap), vmap.stride(0) * 4, L._dev(nmap), nmap.stride(0) * 4,
                cfg["width"], cfg["height"], *[float(x) for x in intr], 0.1, 0.5)
        sums_args = head + (L._dev(out), L._dev(out[27:].view(torch.int32)))

        def host_loop():
            for _ in range(10):
                L._check(lib.dfa_rigid_sums_cloud(*sums_args, L._stream()))
                out.cpu()  # the 28-word read-back

        def device_loop(steps, iters, stop):
            ls, li = (C.c_int * len(steps))(*steps), (C.c_int * len(iters))(*iters)

            def run():
                L._check(lib.dfa_rigid_align_cloud(*head, ls, li, len(steps), stop, stop, L._dev(report), None, L._stream()))
                return report.cpu()  # the one read-back
            return run
        items = [("host loop, 10 x (sums + read-back)", host_loop), ("device loop {1} x 10, no stop", device_loop((1,), (10,), 0.0)),
                 ("device loop, default schedule", device_loop((16, 4, 1), (4, 5, 10), 1e-5))]
        ran = {}
        for label, fn in items:  # warm-up
            for _ in range(3):
                r = fn()
            if r is not None:
                rep = L.RigidAlignReport.from_buffer_copy(r.numpy().tobytes())
                ran[label] = f"iterations {list(rep.iters_run)}, matched {rep.matched_first} -> {rep.matched_last}, status {rep.status}"
        torch.cuda.synchronize()
        ms = {label: [] for label, _ in items}
        for _ in range(windows):
            for label, fn in items:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                ms[label].append((time.perf_counter() - t0) * 1e3 / reps)
        print(f"  N = {N}")
        for label, _ in items:
            t = ms[label]
            print(f"    {label:36s} {float(np.median(t)):7.4f} ms [{min(t):.4f}, {max(t):.4f}]  {ran.get(label, '')}")


def _frames_file(d, cfg, frames):
    from dynfu_amd import synth
    raw = os.path.join(d, "frames.u16")
    np.stack([synth.depth_frame(cfg, f) for f in range(frames)]).astype("<u2").tofile(raw)
    return raw


def _exe():
    from dynfu_amd import build as B
    if not os.path.exists(B.SEQ_BENCH):
        sys.exit("dynfu_amd/host/build/sequence_bench is not built (python -c 'import __graft_entry__ as g; g.build()')")
    return B.SEQ_BENCH


ALIGN_MODES = ("northstar+prealign", "northstar+prealign+device10", "northstar+prealign+device")


def align(name, frames, skip):
    from dynfu_amd import synth
    cfg = synth.CONFIGS[name]
    W, H, dim = cfg["width"], cfg["height"], cfg["dim"]
    with tempfile.TemporaryDirectory() as d:
        raw = _frames_file(d, cfg, frames)
        env = dict(os.environ, DFA_HOST_PROFILE="1")
        for mode in ALIGN_MODES * 2:
            r = subprocess.run([_exe(), raw, str(W), str(H), str(frames), str(dim), mode], capture_output=True, text=True,
                               timeout=900, env=env)
            if r.returncode != 0:
                print(f"  align: {mode} failed: {r.stderr[-500:]}")
                return 1
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            stages = {}
            for line in r.stderr.splitlines():
                m = re.match(r"\[dfa host\]\s+(.*?)\s+([0-9.]+) ms$", line)
                if m:
                    stages.setdefault(m.group(1).strip(), []).append(float(m.group(2)))
            print(f"{name}: NorthStarSolver::alignRigid as {mode}, inside a frame of the {W}x{H} / {dim}^3 sequence "
                  f"({rec['canonical_vertices']} canonical vertices), stage clock with a device synchronise at every mark; frames {skip}.. counted")
            for stage in ("alignRigid", "initializeProblemInstance", "solveAll"):
                t = stages.get(stage, [])[max(skip - 1, 0):]  # (frame 0 has no such stage)
                if t:
                    print(f"  {stage:28s} median {float(np.median(t)):8.3f} ms [{min(t):.3f}, {max(t):.3f}] over {len(t)} frames")
            print(f"  matched in the last frame: {rec['rigid_matched_first']} -> {rec['rigid_matched_last']}, skipped frames {rec['rigid_skipped']}"
                  f", iterations {rec.get('rigid_iterations', 'host loop: 10')}")
    return 0


def frame(name, frames, skip):
    from dynfu_amd import synth
    cfg = synth.CONFIGS[name]
    W, H, dim = cfg["width"], cfg["height"], cfg["dim"]
    with tempfile.TemporaryDirectory() as d:
        raw = _frames_file(d, cfg, frames)
        print(f"{name}: {frames} synthetic {W}x{H} depth frames, {dim}^3 volume; ms per frame inside DynFusion::operator(), "
              f"frames {skip}.. counted")
        for mode in (("northstar",) + ALIGN_MODES) * 2:
            r = subprocess.run([_exe(), raw, str(W), str(H), str(frames), str(dim), mode], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(f"  {mode}: failed: {r.stderr[-500:]}")
                return 1
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            t = rec["frame_ms"][skip:]
            extra = f", matched {rec['rigid_matched_first']} -> {rec['rigid_matched_last']}, skipped {rec['rigid_skipped']}" if "prealign" in mode else ""
            print(f"  {mode:28s} median {float(np.median(t)):8.3f} ms [{min(t):.3f}, {max(t):.3f}]  nodes {rec['nodes_first']} -> "
                  f"{rec['nodes_last']}, last frame's cost {rec['cost_first']:.6g} -> {rec['cost_last']:.6g}, valid rows {rec['valid_rows']}{extra}")
            print(f"    frame ms: {[round(v, 2) for v in rec['frame_ms']]}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--part", choices=["kernel", "loop", "align", "frame"])
    a = ap.parse_args()
    rc = 0
    if a.part in (None, "kernel"):
        kernel(a.config, a.windows, a.reps)
    if a.part in (None, "loop"):
        loop(a.config, a.windows, a.reps)
    if a.part in (None, "kernel", "loop"):
        if a.part is None:  # the child processes below get the device to themselves
            import torch
            torch.cuda.empty_cache()
    if a.part in (None, "align"):
        rc = rc or align(a.config, a.frames, a.skip)
    if a.part in (None, "frame"):
        rc = rc or frame(a.config, a.frames, a.skip)
    return rc


if __name__ == "__main__":
    sys.exit(main())
