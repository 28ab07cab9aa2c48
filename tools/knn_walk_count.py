"""CPU count behind the one-loop walk of knn_grid_query (csrc/knn_walk.hpp, profiles/r13_knn_one_loop.md): how many batches
of four candidates a wave executes in the 3 x 3 x 3 block around its queries' cells,

  nine_loops   sum over the nine rows of the longest lane's batches in that row   (nine wave-wide loops, scan_block3)
  one_loop     the longest lane's sum over its nine rows                          (one loop per lane, a batch stays in a range)
  joined       the longest lane's batches with its ranges joined                  (a batch may cross ranges)

on synth.canonical of a configuration: the grid formed as grid_build_one_kernel forms it (float32: bounding box of the
nodes, cs = max(cbrt(volume / D), longest extent / 32), dim = int(extent / cs) + 1, cells by cell_of), waves of 64
consecutive vertices.  No GPU, no library.

usage: python tools/knn_walk_count.py [C1 C2 C3 C4]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KNN_GRID_MAX_DIM = 32
BATCH = 4


def grid_of(node_pos):
    """(bmin, cs, inv_cs, dim) as grid_build_one_kernel computes them"""
    f = np.float32
    node_pos = np.asarray(node_pos, f)
    D = len(node_pos)
    bmin = node_pos.min(0)
    ext = np.maximum(node_pos.max(0) - bmin, f(0))
    cs = np.cbrt(f(f(f(ext[0] * ext[1]) * ext[2]) / f(D)))
    cs = max(f(cs), f(ext.max() / f(KNN_GRID_MAX_DIM)))
    if not cs > 0:
        cs = f(1)
    inv_cs = f(1) / f(cs)
    dim = np.clip((ext * inv_cs).astype(np.int64) + 1, 1, KNN_GRID_MAX_DIM)
    return bmin, f(cs), inv_cs, dim


def cells_of(p, bmin, inv_cs, dim):
    c = np.floor((np.asarray(p, np.float32) - bmin) * inv_cs)
    c = np.clip(np.nan_to_num(c, nan=0.0), 0, dim - 1)  # (clamped as floats: far queries; a NaN converts to 0 on the device)
    return c.astype(np.int64)


def row_lengths(node_pos, queries):
    """(n, 9) candidates of every query in the nine x-rows around its cell, row i = 3 (dz + 1) + (dy + 1)"""
    bmin, _, inv_cs, dim = grid_of(node_pos)
    nc = cells_of(node_pos, bmin, inv_cs, dim)
    counts = np.zeros((dim[2], dim[1], dim[0]), np.int64)
    np.add.at(counts, (nc[:, 2], nc[:, 1], nc[:, 0]), 1)
    prefix = np.concatenate([np.zeros((dim[2], dim[1], 1), np.int64), np.cumsum(counts, 2)], 2)  # [z, y, x]: nodes of the row before x
    qc = cells_of(queries, bmin, inv_cs, dim)
    x0, x1 = np.maximum(qc[:, 0] - 1, 0), np.minimum(qc[:, 0] + 1, dim[0] - 1)
    out = np.zeros((len(qc), 9), np.int64)
    for i in range(9):
        z, y = qc[:, 2] - 1 + i // 3, qc[:, 1] - 1 + i % 3
        inside = (z >= 0) & (z < dim[2]) & (y >= 0) & (y < dim[1])
        zc, yc = np.clip(z, 0, dim[2] - 1), np.clip(y, 0, dim[1] - 1)
        out[:, i] = np.where(inside, prefix[zc, yc, x1 + 1] - prefix[zc, yc, x0], 0)
    return out


def wave_counts(lengths):
    """per wave of 64 consecutive queries: (nine_loops, one_loop, joined) in batches"""
    n = len(lengths)
    pad = (-n) % 64
    L = np.concatenate([lengths, np.zeros((pad, 9), np.int64)]).reshape(-1, 64, 9)
    batches = (L + BATCH - 1) // BATCH
    nine = batches.max(1).sum(1)
    one = batches.sum(2).max(1)
    joined = ((L.sum(2) + BATCH - 1) // BATCH).max(1)
    return nine, one, joined


def count(cfg_name):
    from dynfu_amd import synth
    cfg = synth.CONFIGS[cfg_name]
    c = synth.canonical(cfg)
    lengths = row_lengths(c["node_pos"], c["verts"])
    nine, one, joined = wave_counts(lengths)
    return dict(config=cfg_name, nodes=cfg["D"], k=cfg["k"], vertices=len(c["verts"]), nine_loops=float(nine.mean()),
                one_loop=float(one.mean()), joined=float(joined.mean()), candidates_mean=float(lengths.sum(1).mean()))


if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("-")] or ["C1", "C2", "C3", "C4"]
    print("| config | batches of 4 per wave, nine loops | one loop per lane | ranges joined | candidates per lane, mean |")
    print("|---|---|---|---|---|")
    for name in names:
        r = count(name)
        print("| %s (%d nodes, k %d) | %.1f | %.1f | %.1f | %.1f |" % (name, r["nodes"], r["k"], r["nine_loops"], r["one_loop"], r["joined"], r["candidates_mean"]))
