"""The multi-level regularisation graph of the north-star solve, restated in numpy from the rule in include/dynfu_amd.h
(dfa_solver6_set_reg_hierarchy), not from dynfu_amd/csrc/reg_hierarchy.hip.

A configuration is levels (1..8), slots[levels], epsilon > 0, beta >= 2.

cells   c0 = floor(p / epsilon) per coordinate, in float32 (numpy's division is correctly rounded, as the device's), as a
        signed integer; c_l = c0 // beta^l, int64 floor division.  A node with a non-finite coordinate or |c0| >= 2^20
        represents no cell and has level 0.
level   a node represents level l >= 1 when it is the lowest-indexed node of its cell c_l; level(n) is the highest level
        it represents (at most levels - 1), or 0.  Cells nest: asserted here.
rows    row n is filled for l = 0 .. level(n): the slots[l] nearest nodes m with level(m) >= l, m != n, m not yet in the
        row; ascending squared distance, ties to the lower index; compact, -1 padded.

Distances are exhaustive and float64; `check_rows` compares a device graph level by level with the tie tolerance of
solve6_statement.check_graph (the device orders by float32 squared distances)."""
import numpy as np

CELL_LIMIT = 1 << 20


def cells0(node_pos, epsilon):
    """(c0 (D, 3) int64, valid (D,) bool)"""
    p = np.asarray(node_pos, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor(p / np.float32(epsilon))
        valid = (np.abs(f) < CELL_LIMIT).all(1)  # (false for NaN and +-inf)
    return np.where(valid[:, None], f, 0).astype(np.int64), valid


def node_levels(node_pos, epsilon, beta, levels):
    c0, valid = cells0(node_pos, epsilon)
    D = len(c0)
    level = np.zeros(D, np.int32)
    ids = np.flatnonzero(valid)
    reps_below = None
    for l in range(1, levels):
        # (python int power: exact; |c0| < 2^20, so every divisor from 2^20 on gives the same 0 / -1 and int64 holds it)
        c = np.floor_divide(c0[ids], min(int(beta) ** l, 1 << 40))
        _, first = np.unique(c, axis=0, return_index=True)  # return_index: the first occurrence = the lowest index
        reps = ids[first] if len(ids) else ids
        if reps_below is not None:
            assert np.isin(reps, reps_below).all(), "a level's representative that does not represent the level below"
        level[reps] = l
        reps_below = reps
    return level


def _d2(node_pos):
    p = np.asarray(node_pos, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)


def rows(node_pos, level, slots, k):
    """the statement's reg_graph (D, k) int32"""
    D = len(level)
    out = np.full((D, k), -1, np.int32)
    if D == 0:
        return out
    d2 = _d2(node_pos)
    for n in range(D):
        row = []
        for l in range(min(int(level[n]), len(slots) - 1) + 1):
            ok = (level >= l) & np.isfinite(d2[n])
            ok[n] = False
            ok[row] = False
            cand = np.flatnonzero(ok)
            cand = cand[np.argsort(d2[n, cand], kind="stable")]  # stable: ties stay in index order
            row += cand[:slots[l]].tolist()
        out[n, :len(row)] = row
    return out


def check_rows(node_pos, level, slots, k, graph, tie=1e-6):
    """a device graph against the rule: per row and level the right number of entries, each of level >= l, not the node
    itself, not in the row before, at the j-th smallest distance of the candidates of that level (ties within `tie`
    relative in either order); levels ascending, compact, -1 padded.  Returns the number of (row, level) segments checked."""
    graph = np.asarray(graph)
    D = len(level)
    assert graph.shape == (D, k), graph.shape
    if D == 0:
        return 0
    d = np.sqrt(_d2(node_pos))
    segments = 0
    for n in range(D):
        at = 0
        taken = []
        for l in range(min(int(level[n]), len(slots) - 1) + 1):
            ok = (level >= l) & np.isfinite(d[n])
            ok[n] = False
            ok[taken] = False
            ref = np.sort(d[n, ok])[:slots[l]]
            got = graph[n, at:at + len(ref)]
            assert (got >= 0).all() and ok[got].all(), (n, l, graph[n].tolist())
            assert len(set(got.tolist())) == len(got), (n, l, graph[n].tolist())
            dg = d[n, got]
            assert (np.abs(dg - ref) <= tie * np.maximum(ref, 1e-300) + 1e-12).all(), (n, l, graph[n].tolist(), dg, ref)
            taken += got.tolist()
            at += len(ref)
            segments += 1
        assert (graph[n, at:] == -1).all(), (n, graph[n].tolist())
    return segments


# ---------------------------------------------------------------------------------------- hops over a block pattern
def pattern(D, data_idx, reg_idx):
    """the block pattern of the normal matrix as a symmetric boolean csr matrix: every pair of nodes in one vertex's list,
    every regularisation edge both ways, the diagonal"""
    import scipy.sparse as sp
    r, c = [np.arange(D)], [np.arange(D)]
    data_idx = np.asarray(data_idx).reshape(len(data_idx), -1)
    for a in range(data_idx.shape[1]):
        for b in range(data_idx.shape[1]):
            both = (data_idx[:, a] >= 0) & (data_idx[:, b] >= 0)
            r.append(data_idx[both, a]), c.append(data_idx[both, b])
    reg_idx = np.asarray(reg_idx)
    n, j = np.nonzero(reg_idx >= 0)
    r += [n, reg_idx[n, j]]
    c += [reg_idx[n, j], n]
    r, c = np.concatenate(r), np.concatenate(c)
    return sp.csr_matrix((np.ones(len(r), bool), (r, c)), shape=(D, D))


def pattern_of_plan(cols, cnt):
    """the same from a plan's matrix_columns (D, cap) / matrix_row_blocks (D,)"""
    import scipy.sparse as sp
    D = len(cnt)
    used = np.arange(cols.shape[1])[None, :] < np.asarray(cnt)[:, None]
    r = np.repeat(np.arange(D), cnt)
    return sp.csr_matrix((np.ones(len(r), bool), (r, np.asarray(cols)[used])), shape=(D, D))


def hops(adj, sources):
    """breadth-first distance of every node from the nearest of `sources` (-1: not reached)"""
    D = adj.shape[0]
    dist = np.full(D, -1, np.int64)
    front = np.unique(np.asarray(sources, np.int64))
    dist[front] = 0
    h = 0
    adj = adj.tocsr()
    while len(front):
        h += 1
        nxt = np.unique(adj[front].indices)
        front = nxt[dist[nxt] < 0]
        dist[front] = h
    return dist
