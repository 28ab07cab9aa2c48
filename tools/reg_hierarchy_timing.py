"""What the multi-level regularisation graph (dfa_solver6_set_reg_hierarchy) costs and buys, switch off against switch on in
the same session, in two parts.

1. The north-star frame of bench.py (Sequence6: graph build + solve from the canonical state, the bench line's parameters) at
   C2 / C3 / C4, on ONE plan whose switch alternates from window to window after a warm-up of each.  Per window: device
   events around `--reps` graph builds (dfa_solver6_set_problem) and around `--reps` frames (build + solve + warp), walking the
   sequence's frames.  Reported per mode: median over the windows with [min, max]; and per frame of the sequence, from a pass of
   its own, pcg_iters, gn_solves, final_cost, valid_last and max_row_blocks.  slots: {2, 1, 1} at k = 4, {4, 2, 2} at k = 8;
   epsilon: `--epsilon`, or the median distance of a node to its nearest other node (the cell the nodes were seeded at).
2. The regrow sequence of tools/regrow_timing.py (dynfu_amd/host/build/sequence_bench, a child process per run: this process
   holds no GPU memory by then): northstar+regrow against northstar+regrow+hier, each run twice in alternation; per run the
   median frame after the first `--skip` frames, [min, max], and per frame the PCG iterations, solves, final energy, valid rows.

The tables go to stdout; --out FILE also appends every record as a JSON line.

usage: python tools/reg_hierarchy_timing.py [--configs C2,C3,C4] [--windows 7] [--reps 10] [--beta 4] [--epsilon 0]
                                             [--frames 14] [--skip 4] [--part frame|sequence] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SLOTS = {4: [2, 1, 1], 8: [4, 2, 2]}
STAT_KEYS = ("pcg_iters", "gn_solves", "final_cost", "valid_last", "max_row_blocks")


def frame_part(name, windows, reps, beta, epsilon, out):
    import torch

    import bench
    device = torch.device("cuda:0")
    seq = bench.Sequence6(name, device, 64)
    slots = SLOTS[4 if seq.k <= 4 else 8]
    if sum(slots) > seq.k:
        slots = [seq.k]
    if epsilon <= 0:  # the nodes' own spacing
        seq.build_graph(0)
        rg = seq.solver.graphs()[1][:, 0].long()
        epsilon = float((seq.nodes - seq.nodes[rg.clamp(min=0)]).norm(dim=1)[rg >= 0].median())
    modes = {"flat": None, "hierarchy": slots}

    def switch(mode):
        seq.solver.set_reg_hierarchy(modes[mode], epsilon, beta)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(reps):
            fn(r)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    per_frame, levels = {}, None
    for mode in modes:  # warm-up of each, and the per-frame figures
        switch(mode)
        rows = []
        for f in range(seq.n_frames):
            seq.solve(f)
            st = seq.solver.stats()
            rows.append({k: st[k] for k in STAT_KEYS})
        per_frame[mode] = rows
        if mode == "hierarchy":
            lv = seq.solver.node_levels()
            levels = np.bincount(lv.cpu().numpy()).tolist() if lv is not None else None
    torch.cuda.synchronize()
    ms = {m: dict(graph=[], frame=[]) for m in modes}
    for w in range(windows):
        for mode in (list(modes) if w % 2 == 0 else list(modes)[::-1]):
            switch(mode)
            seq.solve(0)  # (the plan's captured graphs and launch budget settle on this mode's graph)
            ms[mode]["graph"].append(timed(lambda r: seq.build_graph(r % seq.n_frames)))
            ms[mode]["frame"].append(timed(lambda r: seq.solve(r % seq.n_frames)))
    print(f"{name}: D {seq.D} N {seq.N} k {seq.k}, slots {slots}, epsilon {epsilon:.4f}, beta {beta}, level sets {levels}; "
          f"{windows} windows x {reps} calls, median [min, max] ms")
    rec = dict(part="frame", config=name, D=seq.D, N=seq.N, k=seq.k, slots=slots, epsilon=epsilon, beta=beta, level_sets=levels,
               windows=windows, reps=reps, modes={})
    for mode in modes:
        g, fr = ms[mode]["graph"], ms[mode]["frame"]
        rows = per_frame[mode]
        tot = {k: float(np.mean([r[k] for r in rows])) for k in STAT_KEYS}
        print(f"  {mode:10s} graph build {np.median(g):7.4f} [{min(g):.4f}, {max(g):.4f}]  frame {np.median(fr):7.4f} "
              f"[{min(fr):.4f}, {max(fr):.4f}]  mean over {len(rows)} frames: pcg_iters {tot['pcg_iters']:.1f} gn_solves "
              f"{tot['gn_solves']:.2f} final_cost {tot['final_cost']:.6g} valid_last {tot['valid_last']:.0f} max_row_blocks "
              f"{max(r['max_row_blocks'] for r in rows)}")
        rec["modes"][mode] = dict(graph_ms=g, frame_ms=fr, per_frame=rows)
    out.write(json.dumps(rec) + "\n")
    out.flush()
    del seq
    torch.cuda.empty_cache()


def sequence_part(name, frames, skip, out):
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
        for mode in ("northstar+regrow", "northstar+regrow+hier", "northstar+regrow", "northstar+regrow+hier"):
            r = subprocess.run([exe, raw, str(W), str(H), str(frames), str(dim), mode], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(f"  {mode}: failed: {r.stderr[-500:]}")
                return 1
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            t = rec["frame_ms"][skip:]
            print(f"  {mode:24s} median {float(np.median(t)):8.3f} ms [{min(t):.3f}, {max(t):.3f}]  nodes {rec['nodes_first']} -> "
                  f"{rec['nodes_last']}, levels {rec.get('node_levels')}")
            for key in ("pcg_iters_by_frame", "gn_solves_by_frame", "final_cost_by_frame", "valid_rows_by_frame"):
                print(f"    {key}: {rec[key]}")
            print(f"    frame ms: {[round(v, 2) for v in rec['frame_ms']]}")
            out.write(json.dumps(dict(part="sequence", config=name, skip=skip, **rec)) + "\n")
            out.flush()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3,C4")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--beta", type=int, default=4)
    ap.add_argument("--epsilon", type=float, default=0.0)
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--part", choices=["frame", "sequence"])
    ap.add_argument("--out", default=os.devnull)
    a = ap.parse_args()
    with open(a.out, "a") as out:
        if a.part != "sequence":
            for name in a.configs.split(","):
                frame_part(name, a.windows, a.reps, a.beta, a.epsilon, out)
        if a.part != "frame":
            return sequence_part("C2", a.frames, a.skip, out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
