"""Inputs of the correspondence tests (tests/test_correspond_statement_cpu.py, tests/test_gpu_correspond.py): data only,
built by functions.

dfa_correspond.  Five canonical clouds, one per grid the search can build (GRIDS).  Every cloud holds the eight corners of
a box with power-of-two extents, and its size is chosen so that the cells-per-axis cap decides the cell size (by more than
5 % over the volume term, so the rounding of cbrtf does not matter): the cell size is an exact power of two, every wall is
a float, and every coordinate below — a multiple of 1/256 cell — is exact.  The points are placed by hand in the first
32 x 32 cells of the grid, a few per scenario and most cells empty, so that every query has a known answer and settles at
a known stage of knn_grid_query<1, TIGHT> (csrc/knn_device.hpp); the rest of the count is filler in eight cell columns no
query comes near.  All coordinates of the plan are in CELLS from the box's minimum corner:

    y 23.5 .. 32   class 5 (empty block: the ball of cells grows, or the shell walk takes over) around two points
    y 17 .. 23.5   class 7 (the widest ball a known point can ask for)
    y 13 .. 17     class 6 (the block holds a point, the nearest one lies outside it)
    y  1 .. 13     classes 2, 3, 4, 10: one scenario per 3 x 3 block of cells, the blocks three cells apart
    y  0 ..  1     class 1 (settled by the own cell)
    x 30 .. 32, y 4 .. 8   filler

The classes (the `cls` of a query):
    1   settles in shell 0            2   needs shell 1 across a wall / an edge / a corner, pruning active
    3   exact tie across a wall       4   queries and points exactly on walls, queries on the box's corners
    5   empty 3 x 3 x 3 block         6   block not decisive          7   widest known-point ball
    8   outside the grid              9q  non-finite query            9c  NaN canonical points in or next to the cell
    10  the nearest point three times
Class 7 as "a known point five cells away" cannot exist: a point found by shells 0 and 1 lies in the 3 x 3 x 3 block, at
most 2 sqrt(3) cells from the query, so the reach of a known-point ball never exceeds four cells.  The class holds the
widest ball there is instead: the known point in the far corner of the block, the answer outside the block.

dfa_correspond_projective.  projective_case(): small maps and a few hundred vertices each, the gates' edges included."""
import functools
from collections import namedtuple

import numpy as np

import correspond_statement as S

f32 = np.float32

# box extents (m), canonical points, cell size (m), cells per axis, the search form dfa_correspond takes
Grid = namedtuple("Grid", "box n_canon cs dim form")
GRIDS = {
    "node_thin": Grid((4.0, 4.0, 2.0 ** -6), 1024, 2.0 ** -3, (32, 32, 1), "node_grid"),
    "node_3d": Grid((4.0, 4.0, 0.375), 4096, 2.0 ** -3, (32, 32, 4), "node_grid"),
    "point_thin": Grid((4.0, 4.0, 2.0 ** -6), 16384, 2.0 ** -5, (128, 128, 1), "point_grid"),
    "point_3d": Grid((4.0, 4.0, 0.125), 32768, 2.0 ** -5, (128, 128, 5), "point_grid"),
    "large_3d": Grid((8.0, 8.0, 0.25), 500001, 2.0 ** -5, (256, 256, 9), "point_grid_large"),
}
BMIN = (-2.0, 1.0, 0.5)  # the box's minimum corner (m): the walls stay exact floats
NONFINITE_QUERY_GRIDS = ("node_thin", "node_3d", "point_thin")  # (a query nothing settles walks every cell of the grid)
CLASSES = ("1", "2", "3", "4", "5", "6", "7", "8", "9q", "9c", "10")

Query = namedtuple("Query", "cls pos target note")  # pos in cells; target: the canonical index expected, or None


def _q(x):
    """to a multiple of 1/256 cell"""
    return np.round(np.asarray(x, np.float64) * 256.0) / 256.0


class _Plan:
    def __init__(self, name):
        self.name, self.g = name, GRIDS[name]
        self.zspan = self.g.box[2] / self.g.cs          # the box's height in cells
        self.three_d = self.g.dim[2] > 1
        self.zc = {1: 0, 4: 1, 5: 2, 9: 4}[self.g.dim[2]]  # the z cell most scenarios live in
        self.zr = 0.5 if self.three_d else self.zspan / 2  # ... and their height in it
        self.lists = dict(early=[], mid=[], late=[])
        self.early, self.queries = self.lists["early"], []

    # a canonical point (cells); where: its index lies before the filler's ("early"), in the middle of them ("mid") or
    # behind them ("late").  Returns a handle for `target`.
    def point(self, x, y, z=None, where="early"):
        z = self.zc + self.zr if z is None else z
        self.lists[where].append(_q((x, y, z)))
        return (where, len(self.lists[where]) - 1)

    def raw_point(self, xyz, where="early"):  # (NaN coordinates pass; the finite ones are multiples of 1/256 cell too)
        xyz = np.asarray(xyz, np.float64)
        self.lists[where].append(np.where(np.isnan(xyz), xyz, _q(np.where(np.isnan(xyz), 0, xyz))))
        return (where, len(self.lists[where]) - 1)

    def query(self, cls, x, y, z=None, target=None, note=""):
        z = self.zc + self.zr if z is None else z
        pos = np.asarray((x, y, z), np.float64)
        self.queries.append(Query(cls, np.where(np.isfinite(pos), _q(np.where(np.isfinite(pos), pos, 0)), pos), target, note))


def _axis(a, v, base):
    p = list(base)
    p[a] = v
    return p


def _build_plan(name):
    P = _Plan(name)
    g, zc, zr = P.g, P.zc, P.zr
    dimx, dimy, dimz = g.dim
    zq = zc + zr
    axes = (0, 1, 2) if P.three_d else (0, 1)
    nan = np.nan

    # ---- the box: a NaN point at index 0 (cell (0, 0, 0), with the minimum corner), then the eight corners
    P.raw_point((nan, nan, nan))
    top = (float(dimx), float(dimy), P.zspan)
    corners = [P.point(*[top[a] if (i >> a) & 1 else 0.0 for a in range(3)]) for i in range(8)]
    for i, h in enumerate(corners):
        pos = [top[a] if (i >> a) & 1 else 0.0 for a in range(3)]
        P.query("4", *pos, target=h, note="box corner %d%s" % (i, ": cell index clamped from dim" if i == 7 else ""))
    P.query("9c", 0.0, 0.0, 0.0, target=corners[0], note="a NaN point of lower index in the cell")

    # ---- class 1: the own cell settles it (row y = 0; meaningless where the cloud is thinner than 0.4 cells)
    for i in range(8):
        cx = 2 + 2 * i
        ang = i * np.pi / 4
        h = P.point(cx + 0.5 + 0.2 * np.cos(ang), 0.5 + 0.2 * np.sin(ang))
        if P.three_d or P.zspan >= 0.5:
            P.query("1", cx + 0.5, 0.5, target=h, note="nearest 0.2 cells away in the own cell")

    # ---- the scenarios of one 3 x 3 block each
    anchors = [(2 + 3 * i, 2 + 3 * j) for j in range(4) for i in range(9)]
    anchors.reverse()

    def at(anchor, u):  # position u (cells, relative to the anchor cell's minimum corner) -> plan coordinates
        return (anchor[0] + u[0], anchor[1] + u[1], zc + u[2])

    centre = (0.5, 0.5, zr)
    # class 2: 0.1 cells from a wall / an edge / a corner, the nearest point 0.1 cells beyond it, a farther point in the own
    # cell (so that d0 is finite and the wall[][] pruning decides which neighbours are read)
    signs2 = []
    for a in axes:
        for s in (0, 1):
            signs2.append({a: s})
    for a, b in ((0, 1),) + (((0, 2), (1, 2)) if P.three_d else ()):
        for sa, sb in ((0, 0), (0, 1), (1, 0), (1, 1)) if (a, b) == (0, 1) else ((0, 1), (1, 0)):
            signs2.append({a: sa, b: sb})
    if P.three_d:
        for sx, sy, sz in ((0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0)):
            signs2.append({0: sx, 1: sy, 2: sz})
    for sg in signs2:
        A = anchors.pop()
        uq, un = list(centre), list(centre)
        for a, s in sg.items():
            uq[a], un[a] = (0.9, 1.1) if s else (0.1, -0.1)
        uo = list(centre)  # the own cell's point: 0.4 cells behind the query on every axis involved
        for a, s in sg.items():
            uo[a] = 0.5
        if not P.three_d:
            uq[2] = un[2] = uo[2] = zr
        P.point(*at(A, uo))
        h = P.point(*at(A, un))
        P.query("2", *at(A, uq), target=h,
                note="across " + " ".join("%s%s" % ("-+"[s], "xyz"[a]) for a, s in sorted(sg.items())))

    # class 3: the own cell's point and a point across the high wall at exactly equal distance
    for edge in (False, True):
        for on_wall in (True, False):
            for lower_across in (True, False):
                A = anchors.pop()
                uq, ux, uo = list(centre), list(centre), list(centre)
                for a in ((0, 1) if edge else (0,)):
                    uq[a] = 0.75
                    ux[a], uo[a] = (1.0, 0.5) if on_wall else (1.25, 0.25)
                hs = {}
                for who in (("x", "o") if lower_across else ("o", "x")):
                    hs[who] = P.point(*at(A, ux if who == "x" else uo))
                P.query("3", *at(A, uq), target=hs["x" if lower_across else "o"],
                        note="tie across %s, far point %s, lower index %s" % ("an edge" if edge else "a wall",
                                                                               "on the wall" if on_wall else "inside the neighbour",
                                                                               "across" if lower_across else "in the own cell"))

    # class 4: queries on walls (an integer cell coordinate), canonical points on walls (they belong to the upper cell)
    for a in axes:
        A = anchors.pop()
        P.point(*at(A, _axis(a, 0.4, centre)))
        h = P.point(*at(A, _axis(a, -0.3, centre)))
        P.query("4", *at(A, _axis(a, 0.0, centre)), target=h, note="query on a %s wall" % "xyz"[a])
    A = anchors.pop()
    P.point(*at(A, centre))
    h = P.point(*at(A, (-0.2, -0.2, centre[2])))
    P.query("4", *at(A, (0.0, 0.0, centre[2])), target=h, note="query on an edge of its cell")
    for a in (0, 1):
        A = anchors.pop()
        P.point(*at(A, _axis(a, 0.3, centre)))
        h = P.point(*at(A, _axis(a, 1.0, centre)))
        P.query("4", *at(A, _axis(a, 0.8, centre)), target=h, note="canonical point on the high %s wall" % "xyz"[a])

    # class 10: the nearest point three times, the copies' indices far apart
    for where in (("early", "mid", "late"), ("mid", "late", "late")):
        A = anchors.pop()
        h = P.point(*at(A, centre), where=where[0])
        P.point(*at(A, centre), where=where[1])
        P.point(*at(A, centre), where=where[2])
        for u in ((0.3, 0.5), (-0.2, 0.5), (0.5, 1.25), (-0.1, -0.1)):
            P.query("10", *at(A, (u[0], u[1], centre[2])), target=h, note="three copies")

    # ---- class 9c: canonical points with NaN coordinates.  A NaN coordinate puts the point into cell 0 of that axis
    # (cell_of: the conversion of NaN gives 0), so the scenarios live where that cell is: NaN in x in the column x = 0, NaN
    # in y in the row y = 0, NaN in z in the layer z = 0, NaN in all three in cell (0, 0, 0).  Each kind with the NaN point
    # once in the cell of query and answer and once in a shell-1 neighbour the search has to read (the query 0.1 cells
    # from that wall, the answer 0.3 cells away), and with its index once below and once above the answer's.
    z0 = 0.5 if P.three_d else zr  # (in the layer z = 0)

    def nan_scenario(kind, cell, neighbour, below):
        """kind: the NaN axes; cell: of query and answer; neighbour: the finite axis along which the NaN point's cell
        is the next one, or None for the same cell"""
        c = np.asarray(cell, np.float64)
        rel = np.array([0.5, 0.5, z0 if cell[2] == 0 else zr])
        uq, ua, un = rel.copy(), rel.copy(), rel.copy()
        if neighbour is None:
            ua[0] += 0.2
        else:
            uq[neighbour], ua[neighbour], un[neighbour] = 0.9, 0.6, 1.3
        for a in kind:
            un[a] = nan
        if below is True:
            P.raw_point(c + un)
        h = P.point(*(c + ua))
        if below is False:
            P.raw_point(c + un, where="late")
        P.query("9c", *(c + uq), target=h, note="NaN in %s, the NaN point in %s, its index %s the answer's" % (
            "".join("xyz"[a] for a in kind), "the same cell" if neighbour is None else "the next cell along +" + "xyz"[neighbour],
            "below and above" if below is None else "below" if below else "above"))

    for i, (neighbour, below) in enumerate(((None, True), (None, False), (1, True), (1, False))):
        nan_scenario((0,), (0, 24 + 2 * i, zc), neighbour, below)
    for x, (neighbour, below) in zip((18, 20, 24, 26), ((None, True), (None, False), (0, True), (0, False))):
        nan_scenario((1,), (x, 0, zc), neighbour, below)
    for y, (neighbour, below) in zip((16, 18, 22, 4), ((None, True), (None, False), (0, True), (0, False))):
        nan_scenario((2,), (0, y, 0), neighbour, below)
    # NaN in all three: cell (0, 0, 0) holds the point of index 0 and one behind every other point
    P.raw_point((nan, nan, nan), where="late")
    nan_scenario((0, 1, 2), (0, 0, 0), None, None)
    h = P.point(1.4, 0.6, z0)
    P.query("9c", 1.1, 0.6, z0, target=h, note="NaN in xyz, the NaN point in the next cell along -x, its index below and above the answer's")

    # ---- class 6 (band y 13 .. 17): shells 0 and 1 find K 1.3 cells away, the answer T is 1.2 cells away in a cell outside
    # the block; alternately towards +x and -x, and once along y
    for i in range(6):
        cx, s = 2 + 4 * i, 1 if i % 2 == 0 else -1
        qx = cx + (0.9 if s > 0 else 0.1)
        P.point(qx - 1.3 * s, 14.5)
        h = P.point(qx + 1.2 * s, 14.5)
        for dy in (0.0, 0.2):
            P.query("6", qx, 14.5 + dy, target=h, note="answer two cells along %sx" % "+-"[s < 0])
    P.point(28.5, 14.9 - 1.3)
    h = P.point(28.5, 14.9 + 1.2)
    for dx in (0.0, 0.2):
        P.query("6", 28.5 + dx, 14.9, target=h, note="answer two cells along +y")

    # ---- class 7 (band y 17 .. 23.5): K in the far corner of the block, the answer three cells away along x
    dT = 3.0 if P.three_d else 2.4
    for i in range(4):
        cx, s = 4 + 7 * i, 1 if i % 2 == 0 else -1
        qx = cx + (0.1 if s > 0 else 0.9)
        kz = zc + 0.1 + 1.8 if P.three_d else zq
        qz = zc + 0.1 if P.three_d else zq
        P.point(qx + 1.8 * s, 20.1 + 1.8, kz)
        h = P.point(qx - dT * s, 20.1, qz)
        for dy in (0.0, -0.05):
            P.query("7", qx, 20.1 + dy, qz, target=h, note="answer three cells along %sx" % "-+"[s < 0])

    # ---- class 5 (y 23.5 .. 32): nothing in the block.  One point, queries 1.7 / 2.6 / 3.5 / 4.4 cells from it: the ball
    # of cells settles at its first radius (two cells), after one or two growths, or gives way to the shell walk
    pz = 0.45 if P.three_d else zq
    h5 = P.point(16.45, 27.5, pz)
    h5d = P.point(25.9, 24.9, 0.9 if P.three_d else zq)  # (in the corner of its cell: a diagonal leaves the block at once)
    for d in (1.7, 2.6, 3.5, 4.4):
        P.query("5", 16.45 + d, 27.5, pz, target=h5, note="%.1f cells along +x" % d)
        P.query("5", 16.45 - d, 27.5, pz, target=h5, note="%.1f cells along -x" % d)
        if P.three_d and d < 3:
            P.query("5", 16.45, 27.5, pz + d, target=h5, note="%.1f cells along +z" % d)
        if P.three_d and d > 2:
            e = d / np.sqrt(3.0)
            P.query("5", 25.9 + e, 24.9 + e, 0.9 + e, target=h5d, note="%.1f cells along the +x +y +z diagonal" % d)
        else:
            e = d / np.sqrt(2.0)
            P.query("5", 25.9 + e, 24.9 + e, 0.9 if P.three_d else zq, target=h5d, note="%.1f cells along the +x +y diagonal" % d)
    # the variant: the two-cell ball touches the cell of F, whose point (2.43 cells away) lies outside the ball — the ball
    # must grow and not return F; N (2.26 cells) is in a cell only the three-cell ball reaches
    P.point(4.5 + 2.4, 28.5 + 0.4)
    h = P.point(4.5 - 1.6, 28.5 - 1.6)
    P.query("5", 4.5, 28.5, target=h, note="variant: a point beyond the radius in a cell the ball touches")

    # ---- class 8: outside the grid, beside a point just inside the face
    P.point(0.25, 8.5), P.point(dimx - 0.25, 10.5), P.point(22.5, 0.25), P.point(8.5, dimy - 0.25)
    for d in (0.5, 3.0, 40.0):
        for pos, what in (((-d, 8.5, zq), "-x"), ((dimx + d, 10.5, zq), "+x"), ((22.5, -d, zq), "-y"), ((8.5, dimy + d, zq), "+y"),
                          ((29.5, 2.5, -d), "-z"), ((29.5, 2.5, dimz + d), "+z"), ((-d, -d, -d), "the minimum corner"),
                          ((dimx + d, dimy + d, dimz + d), "the maximum corner"), ((-d, dimy + d, zq), "the -x +y edge")):
            P.query("8", *pos, note="%.1f cells outside %s" % (d, what))

    # ---- class 9q: non-finite queries
    if name in NONFINITE_QUERY_GRIDS:
        inf = np.inf
        for pos in ((nan, 5.5, zq), (5.5, nan, zq), (5.5, 5.5, nan), (nan, nan, nan), (inf, 5.5, zq), (5.5, -inf, zq),
                    (5.5, 5.5, inf), (-inf, -inf, -inf), (inf, nan, zq), (inf, -inf, zq)):
            P.query("9q", *pos, note="non-finite query")
    return P


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """dict: canon (n_canon, 3), normals, queries (the base set, float32 (m, 3)) and their positions in cells, cls / note /
    target (the expected canonical index, -2: left to the statement) per query, grid, placed (the indices of the
    hand-placed points: everything but the filler)"""
    P = _build_plan(name)
    g = P.g
    early, mid, late = (np.stack(P.lists[k]) for k in ("early", "mid", "late"))
    n_fill = g.n_canon - len(early) - len(mid) - len(late)
    half = n_fill // 2
    assert n_fill > 0
    rng = np.random.default_rng(len(name) + g.n_canon)
    fill = np.stack([rng.integers(int(30.25 * 256), int(31.75 * 256) + 1, n_fill), rng.integers(4 * 256, 8 * 256, n_fill),
                     rng.integers(0, int(P.zspan * 256) + 1, n_fill)], -1) / 256.0
    cells = np.concatenate([early, fill[:half], mid, fill[half:], late])
    bmin = np.asarray(BMIN, np.float64)
    canon = (bmin + cells * g.cs).astype(f32)
    assert np.array_equal(canon[1:9].astype(np.float64), bmin + cells[1:9] * g.cs)  # (exact)
    qpos = np.stack([q.pos for q in P.queries])
    with np.errstate(all="ignore"):
        queries = (bmin + qpos * g.cs).astype(f32)
    base = {"early": 0, "mid": len(early) + half, "late": len(early) + n_fill + len(mid)}
    target = np.array([-2 if q.target is None else base[q.target[0]] + q.target[1] for q in P.queries], np.int64)
    nrm = rng.standard_normal((g.n_canon, 3)).astype(f32)
    return dict(name=name, grid=g, canon=canon, normals=nrm, queries=queries, query_cells=qpos,
                cls=np.array([q.cls for q in P.queries]), note=[q.note for q in P.queries], target=target,
                placed=np.r_[np.arange(len(early)), base["mid"] + np.arange(len(mid)), base["late"] + np.arange(len(late))])


# ------------------------------------------------------------------------------------------ wave composition
def orders(name):
    """the base queries in three orders (index arrays into case["queries"]):
    interleaved — consecutive queries cycle through the classes (shorter classes repeat): every wave of 64 holds them all;
    grouped — every class fills whole waves (its queries repeated up to a multiple of 64);
    ragged — the interleaved order cut to whole waves, then ONE query of a growing ball alone in a last wave."""
    c = grid_case(name)
    by = {k: np.flatnonzero(c["cls"] == k) for k in CLASSES}
    by = {k: v for k, v in by.items() if len(v)}
    longest = max(len(v) for v in by.values())
    inter = np.array([by[k][i % len(by[k])] for i in range(longest) for k in by])
    grouped = np.concatenate([np.resize(v, -(-len(v) // 64) * 64) for v in by.values()])
    growing = next(i for i in by["5"] if c["note"][i].startswith("2.6"))
    ragged = np.concatenate([np.resize(inter, -(-len(inter) // 64) * 64 + 64)[:len(inter) // 64 * 64 + 64], [growing]])
    for wave in range(0, len(inter), 64):
        assert len(set(c["cls"][inter[wave:wave + 64]])) >= 4
    assert len(ragged) % 64 == 1
    return dict(interleaved=inter, grouped=grouped, ragged=ragged)


def finite_queries(c):
    return np.isfinite(c["queries"]).all(1)


@functools.lru_cache(maxsize=None)
def expected(name):
    """nearest() of the base queries of a grid case, computed once: (idx, d2)"""
    c = grid_case(name)
    idx, d2 = S.nearest(c["canon"], c["queries"])
    idx.setflags(write=False), d2.setflags(write=False)
    return idx, d2


# ------------------------------------------------------------------------------------------ thresholds between the forms
# (n_canon, n_live, the form on this side)
THRESHOLDS = [(63, 65536, "scan"), (64, 65536, "node_grid"), (64, 65535, "scan"), (1023, 1, "scan"), (1024, 1, "node_grid"),
              (16383, 256, "node_grid"), (16384, 256, "point_grid"), (500000, 512, "point_grid"),
              (500001, 512, "point_grid_large")]


@functools.lru_cache(maxsize=None)
def threshold_case(n_canon, n_live):
    """random clouds; with 65 536 queries the canonical cloud is small, and the statement is compared on all of them"""
    rng = np.random.default_rng(n_canon + n_live)
    canon = rng.uniform(-1, 1, (n_canon, 3)).astype(f32)
    live = rng.uniform(-1.1, 1.1, (n_live, 3)).astype(f32)
    live[::7] = canon[rng.integers(0, n_canon, len(live[::7]))]  # exact hits
    for a in (canon, live):
        a.setflags(write=False)
    return canon, live


# ------------------------------------------------------------------------------------------ projective cases
def _ulp(x, k):
    """the float32 k ulps away from x"""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf))
    return x


@functools.lru_cache(maxsize=None)
def projective_case(cols, rows, principal="centre"):
    """dict: vertices, normals, vmap, nmap (rows, cols, 4), intr (fx, fy, cx, cy), dist_thresh, min_cosine, `edges`
    (name -> vertex index) and `expect` (name -> associated or not, with both normals and the normal map given).
    The focal lengths are powers of two and the principal point is an integer — the image centre, or -0.0 (the only
    principal point at which u = fmaf(fx, x / z, cx) can be -0.0) — so that the projection of the hand-made vertices is
    exact.  The map is a plane at z = 2 with a little relief; at the pixels the edge vertices land on it is exactly the
    pixel centre's ray at z = 2 with the normal (0, 0, -1)."""
    rng = np.random.default_rng(cols * 1000 + rows)
    negzero = principal == "negzero"
    fx, fy = 16.0, 8.0
    cx, cy = (-0.0, -0.0) if negzero else (float(cols // 2), float(rows // 2))
    jc, ic = int(cx), int(cy)
    dist_thresh, min_cosine = f32(0.125), f32(0.5)
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows))
    z = (2.0 + 0.01 * np.sin(jj) * np.cos(ii)).astype(f32)
    vmap = np.zeros((rows, cols, 4), f32)
    vmap[..., 0] = ((jj + 0.5 - cx) / fx * z).astype(f32)
    vmap[..., 1] = ((ii + 0.5 - cy) / fy * z).astype(f32)
    vmap[..., 2], vmap[..., 3] = z, 1.0
    nmap = np.zeros((rows, cols, 4), f32)
    nn = np.stack([0.1 * np.cos(jj), 0.1 * np.sin(ii), -np.ones(z.shape)], -1)
    nmap[..., :3] = (nn / np.linalg.norm(nn, axis=-1, keepdims=True)).astype(f32)
    verts, norms, edges, expect = [], [], {}, {}

    def pixel(j, i):  # the vertex on the ray through the centre of pixel (column j, row i) at z = 2: u = j + 0.5 exactly
        return [(j + 0.5 - cx) / fx * 2.0, (i + 0.5 - cy) / fy * 2.0, 2.0]

    def flat(j, i):
        vmap[i, j, :3] = np.asarray(pixel(j, i), f32)
        nmap[i, j, :3] = (0.0, 0.0, -1.0)
        return pixel(j, i)

    def add(name, v, ok, n=(0.0, 0.0, -1.0)):
        edges[name], expect[name] = len(verts), ok
        verts.append(np.asarray(v, f32)), norms.append(np.asarray(n, f32))

    # the image bounds.  (u = 0 lands 1/16 m beside the vertex of pixel 0, w = 0 exactly dist_thresh beside it: accepted.)
    for j, i in ((0, 1), (cols - 1, 1), (1, 0), (1, rows - 1)):
        flat(j, i)
    x0, x1, y0, y1 = -cx / fx * 2.0, (cols - cx) / fx * 2.0, -cy / fy * 2.0, (rows - cy) / fy * 2.0  # u = 0, cols; w = 0, rows
    xa, ya = pixel(1, 1)[0], pixel(1, 1)[1]
    add("u = 0", (x0, ya, 2.0), True)
    add("u just below 0", (_ulp(x0, -1) if x0 else -2.0 ** -100, ya, 2.0), False)  # (half the smallest denormal is -0.0)
    add("u just below cols", (_ulp(x1, -2), ya, 2.0), True)  # (one ulp below lands half-way and rounds to cols)
    add("u half an ulp below cols", (_ulp(x1, -1), ya, 2.0), negzero)
    add("u = cols", (x1, ya, 2.0), False)
    add("w = 0", (xa, y0, 2.0), True)
    add("w just below 0", (xa, _ulp(y0, -1) if y0 else -2.0 ** -100, 2.0), False)
    add("w just below rows", (xa, _ulp(y1, -2), 2.0), True)
    add("w half an ulp below rows", (xa, _ulp(y1, -1), 2.0), negzero)
    add("w = rows", (xa, y1, 2.0), False)
    if negzero:  # fmaf(fx, -0.0, -0.0) = -0.0: `u >= 0` holds, floor gives column 0
        add("u = -0.0", (-0.0, ya, 2.0), True)
        add("w = -0.0", (xa, -0.0, 2.0), True)
    add("z = 0", (0.0, 0.0, 0.0), False)
    add("z = -0.0", (0.0, 0.0, -0.0), False)
    add("z smallest denormal", (0.0, 0.0, np.float32(1e-45)), False)  # (in front of the camera; two metres off the map)
    add("z negative", (0.1, 0.1, -2.0), False)
    # the distance gate: the pixel's vertex moved along z only, by exactly dist_thresh (the squared distance is exactly
    # dist_thresh^2: passes)
    p = flat(jc + 1, ic + 1)
    add("distance = dist_thresh", (p[0], p[1], 2.125), True)
    # one float32 ulp (2^-29) above dist_thresh^2: the same 1/8 m along z and 1448 ulps of the coordinate along y,
    # a = 1448 * 2^-25 with a^2 just below 2^-29: fmaf(1/8, 1/8, a^2) rounds to the float32 after 2^-6
    add("squared distance one ulp above", (p[0], p[1] + 1448 * 2.0 ** -25, 2.125), False)
    add("distance one ulp of the depth above", (p[0], p[1], _ulp(2.125, 1)), False)  # (32 ulps of the squared distance)
    # the normal gate: the map normal is (0, 0, -1), the dot product is -nz
    half_less = _ulp(0.5, -1)
    add("cosine = min_cosine, negative dot", flat(jc + 2, ic + 1), True, n=(0.0, 0.0, 0.5))
    add("cosine = min_cosine, positive dot", flat(jc + 3, ic + 1), True, n=(0.0, 0.0, -0.5))
    add("cosine one ulp below, negative dot", flat(jc + 4, ic + 1), False, n=(0.0, 0.0, half_less))
    add("cosine one ulp below, positive dot", flat(jc + 5, ic + 1), False, n=(0.0, 0.0, -half_less))
    # NaN in the maps
    add("map vertex x NaN", flat(jc + 1, ic + 2), False)
    vmap[ic + 2, jc + 1, 0] = np.nan
    add("map vertex y NaN", flat(jc + 2, ic + 2), True)  # the gate reads x; the NaN distance is not `> dist_thresh^2`
    vmap[ic + 2, jc + 2, 1] = np.nan
    add("map normal x NaN", flat(jc + 3, ic + 2), False)
    nmap[ic + 2, jc + 3, 0] = np.nan
    add("exact hit", flat(jc + 4, ic + 2), True)
    add("vertex NaN", (np.nan, 0.0, 2.0), False)
    # a few hundred vertices around the surface, inside and outside every gate
    n_rand = 300
    jr, ir = rng.uniform(-1, cols + 1, n_rand), rng.uniform(-1, rows + 1, n_rand)
    zr = 2.0 + rng.uniform(-0.2, 0.2, n_rand)
    rv = np.stack([(jr - cx) / fx * zr, (ir - cy) / fy * zr, zr], -1)
    rn = rng.standard_normal((n_rand, 3))
    rn /= np.linalg.norm(rn, axis=1, keepdims=True)
    vertices = np.concatenate([np.stack(verts), rv]).astype(f32)
    normals = np.concatenate([np.stack(norms), rn]).astype(f32)
    for a in (vertices, normals, vmap, nmap):
        a.setflags(write=False)
    return dict(vertices=vertices, normals=normals, vmap=vmap, nmap=nmap, intr=(fx, fy, cx, cy), dist_thresh=float(dist_thresh),
                min_cosine=float(min_cosine), edges=edges, expect=expect, cols=cols, rows=rows)


PROJECTIVE_CASES = [(20, 12, "centre"), (64, 48, "centre"), (20, 12, "negzero"), (64, 48, "negzero")]
