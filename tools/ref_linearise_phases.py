"""dev (GPU; a -DDFA_PCG_PROFILE -DDFA_DEV_AB build: bash tools/ab_variant.sh prof all -DDFA_PCG_PROFILE -DDFA_DEV_AB):
per-workgroup life of one reference-mode linearise_kernel launch — the last re-weighting linearisation of the third frame
(the closing evaluation does not record).  Where the launch ends with its rows (the hand-off to the assembly,
solve_linearise.hip) there is no last workgroup and the tail is what is left between the last "rows finished" and the
last exit.
usage: DFA_LIB_PATH=dynfu_amd/build/libdynfu_amd_prof.so [DFA_LIN_HANDOFF=0] python tools/ref_linearise_phases.py C2"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench

name = sys.argv[1] if len(sys.argv) > 1 else "C2"
seq = bench.Sequence(name, torch.device("cuda", 0), n_frames=3)
import dynfu_amd as A
L = A.load()
seq.params.num_iter = 2
for f in range(3):
    seq.build_graph(f)
    seq.solver.solve(seq.params)
torch.cuda.synchronize()
R = seq.N + seq.D * seq.k
buf = np.zeros((1024, 8), np.uint64)
L.dfa_dev_lin_timing.argtypes = [C.c_void_p, C.c_int]
assert L.dfa_dev_lin_timing(buf.ctypes.data, 1024) == 0
buf = buf[buf[:, 0] > 0]  # the workgroups of the launch (a smaller plan has fewer than 1 024)
n = len(buf)
t = buf.astype(np.float64)
t0 = t[:, 0].min()
us = lambda x: (x - t0) / 100.0  # 100 MHz ticks
start, rows, pub, exit_ = us(t[:, 0]), us(t[:, 1]), us(t[:, 2]), us(t[:, 3])
last = np.flatnonzero(buf[:, 7] == 1)
print("%s: %d workgroups, %d rows" % (name, n, R))
print("launch span %.2f us (first start to last exit); last start at %.2f us" % (exit_.max(), start.max()))
print("rows finished, deciles [us]:", " ".join("%.1f" % x for x in np.percentile(rows, np.arange(0, 101, 10))))
print("rows finished -> published, ticket taken [us]: mean %.2f p95 %.2f max %.2f" % ((pub - rows).mean(), np.percentile(pub - rows, 95), (pub - rows).max()))
print("tail: last 'rows finished' at %.2f us -> end of the kernel %.2f us = %.2f us" % (rows.max(), exit_.max(), exit_.max() - rows.max()))
if len(last):
    b = last[0]
    loads, tree, upd = us(t[b, 4]), us(t[b, 5]), us(t[b, 6])
    print("last workgroup (block %d): rows finished %.2f | ticket %.2f | loads + tree %.2f | state update %.2f | exit %.2f" % (b, rows[b], pub[b], tree - loads, upd - tree, exit_[b]))
    print("  its own tail, rows finished -> exit: %.2f us" % (exit_[b] - rows[b]))
else:
    print("no last workgroup: the launch ends with its rows")
