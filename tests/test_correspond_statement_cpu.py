"""CPU tests of tests/correspond_statement.py and tests/correspond_cases.py: the numpy statement of dfa_correspond and
dfa_correspond_projective agrees with the C oracle and with warp_statement.knn, and every hand-placed query of the grid
cases sits where its class says — in the cell, at the distance from the walls and at the stage of knn_grid_query<1, TIGHT>
(csrc/knn_device.hpp) it is named for.  No GPU."""
import numpy as np
import pytest

import correspond_cases as Cc
import correspond_statement as S
import oracle as O
import warp_statement as W

f32 = np.float32
RB = 4  # knn_device.hpp: the widest ball of cells, in cells of reach


def _geometry(name):
    c = Cc.grid_case(name)
    geo = S.grid_geometry(c["canon"], len(c["queries"]))
    return c, geo


# ------------------------------------------------------------------------------------------ the grids are what the table says
@pytest.mark.parametrize("name", sorted(Cc.GRIDS))
def test_the_cap_term_decides_the_cell_size_and_the_grid_is_the_stated_one(name):
    c, geo = _geometry(name)
    g = c["grid"]
    assert len(c["canon"]) == g.n_canon
    assert S.search_form(g.n_canon, len(c["queries"])) == g.form
    for n_live in (len(o) for o in Cc.orders(name).values()):
        assert S.search_form(g.n_canon, n_live) == g.form
    assert geo.cap_term >= 1.05 * geo.volume_term and geo.cs == geo.cap_term  # (cbrtf's rounding cannot matter)
    assert geo.cs == f32(g.cs) and float(geo.inv_cs) == 1.0 / g.cs
    assert tuple(geo.dim) == g.dim
    assert np.array_equal(geo.bmin, np.asarray(Cc.BMIN, f32))
    # every coordinate is exact: the float32 positions ARE bmin + (a multiple of 1/256 cell) * cs
    fin = np.isfinite(c["queries"]).all(1)
    assert np.array_equal(c["queries"][fin].astype(np.float64), np.asarray(Cc.BMIN) + c["query_cells"][fin] * g.cs)
    cell, u = S.cell_coordinates(geo, c["queries"][fin])
    inside = ((c["query_cells"][fin] >= 0) & (c["query_cells"][fin] < np.asarray(g.dim))).all(1)
    assert np.array_equal((cell + u.astype(np.float64))[inside], c["query_cells"][fin][inside])


def _stages(name):
    """per finite base query: the quantities the stages of knn_grid_query decide on, in cells"""
    c, geo = _geometry(name)
    idx, d2 = Cc.expected(name)
    canon, g = c["canon"], c["grid"]
    placed = c["placed"][~np.isnan(canon[c["placed"]]).any(1)]
    pcell, _ = S.cell_coordinates(geo, canon[placed])
    fcell = np.unique(S.cell_coordinates(geo, np.delete(canon, c["placed"], 0))[0], axis=0)
    qcell, u = S.cell_coordinates(geo, c["queries"])
    out = []
    for i in range(len(c["queries"])):
        if not np.isfinite(c["queries"][i]).all():
            out.append(None)
            continue
        ui = u[i].astype(np.float64)
        m = min(ui.min(), (1 - ui).min())
        in_block = (np.abs(pcell - qcell[i]) <= 1).all(1)
        own = (pcell == qcell[i]).all(1)
        dist = np.sqrt((((c["queries"][i].astype(np.float64) - canon[placed].astype(np.float64)) / g.cs) ** 2).sum(1))
        out.append(dict(margin=max(m, 0.0), inside=m >= 0, u=ui, cell=qcell[i], d=float(np.sqrt(float(d2[i]))) / g.cs,
                        d_own=dist[own].min() if own.any() else np.inf, d_block=dist[in_block].min() if in_block.any() else np.inf,
                        answer_cell=S.cell_coordinates(geo, canon[idx[i]][None])[0][0],
                        filler_cells_away=np.abs(fcell - qcell[i]).max(1).min()))
    return c, geo, idx, out


def _reach(r, w):
    return int(r - w) + 1 if r > w else 0


@pytest.mark.parametrize("name", sorted(Cc.GRIDS))
def test_every_query_sits_where_its_class_says(name):
    c, geo, idx, st = _stages(name)
    three_d = c["grid"].dim[2] > 1
    # the answers are the ones the plan names
    known = c["target"] >= 0
    assert np.array_equal(idx[known], c["target"][known]), [c["note"][i] for i in np.flatnonzero(known & (idx != c["target"]))]
    counts = {k: int((c["cls"] == k).sum()) for k in Cc.CLASSES}
    for k in Cc.CLASSES:
        if (k == "1" and name == "node_thin") or (k == "9q" and name not in Cc.NONFINITE_QUERY_GRIDS):
            assert counts[k] == 0  # (the cloud is 1/8 cell thin: no query is 0.2 cells from every wall; walks cost too much)
        else:
            assert counts[k] >= 8, (k, counts[k])
    slack = 0.05
    ball_attempts = set()
    for i, s in enumerate(st):
        k, note = c["cls"][i], c["note"][i]
        if k == "9q":
            assert s is None
            continue
        walls = np.r_[s["u"], 1 - s["u"]]
        if k != "8":
            assert s["inside"], note
        if k not in ("8", "4", "9c", "5"):
            assert s["filler_cells_away"] >= 3
        own_answer = (s["answer_cell"] == s["cell"]).all()
        block_answer = (np.abs(s["answer_cell"] - s["cell"]) <= 1).all()
        if k == "1":  # shell 0 settles: nearer than the nearest wall of the own cell
            assert own_answer and s["d"] <= s["margin"] - slack, note
        elif k == "2":  # not shell 0; shell 1 settles; the own cell holds a point (the pruning is active)
            assert not own_answer and block_answer and np.isfinite(s["d_own"]) and s["d_own"] > s["d"] + slack, note
            assert s["d"] >= s["margin"] + slack and s["d"] <= 1 + s["margin"] - slack, note
        elif k == "3":  # two points at exactly the same float32 distance, the lower index is the answer
            d2 = S.nearest(c["canon"], c["queries"][i:i + 1])[1][0]
            q, cv = c["queries"][i], c["canon"]
            e = q - cv
            same = np.flatnonzero(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) == d2)
            assert len(same) == 2 and idx[i] == same.min(), note
            cells = S.cell_coordinates(geo, cv[same])[0]
            assert (cells == s["cell"]).all(1).sum() == 1, note  # one of the two in the own cell, one across
            assert own_answer == ("own cell" in note)
        elif k == "4":
            on_wall = (s["u"] == 0).any() or (s["u"] == 1).any() or "canonical point on" in note
            assert on_wall, note
            if "canonical point on" in note:  # the point's cell coordinate is an integer: it belongs to the upper cell
                a = "xyz".index(note.split()[-2])
                assert s["answer_cell"][a] == s["cell"][a] + 1
                pu = S.cell_coordinates(geo, c["canon"][idx[i]][None])[1][0]
                assert pu[a] == 0
            if "clamped" in note:
                assert (s["cell"] == np.asarray(c["grid"].dim) - 1).all() and (s["u"][:2] == 1).all()
        elif k == "5":  # nothing in the block
            assert not np.isfinite(s["d_block"]), note
            # the ball of cells: radius 2, 3, 4 cells while it is a ball (reach <= RB), settled when d <= rad sqrt(0.9999)
            attempt, rad = None, 2.0
            for a in range(RB):
                if max(_reach(rad, max(w - 1e-3, 0)) for w in walls) > RB:
                    break
                if s["d"] <= rad - slack:
                    attempt = a
                    break
                assert s["d"] >= rad + slack, note  # (never near the boundary between two radii)
                rad += 1.0
            ball_attempts.add(attempt)
            if "variant" in note:
                assert attempt == 1  # and the two-cell ball touches a cell whose only point is beyond the radius
                dF = np.sqrt(2.4 ** 2 + 0.4 ** 2)
                assert 2 + slack < s["d"] < dF - slack
            elif note.startswith("4.4"):
                assert attempt is None, note  # the shell walk
            else:
                assert attempt == {"1.7": 0, "2.6": 1, "3.5": 2}[note[:3]], note
        elif k in ("6", "7"):  # shells 0 and 1 find a point, do not settle; the answer is outside the block and nearer
            assert np.isfinite(s["d_block"]) and not block_answer and s["d"] <= s["d_block"] - slack, note
            assert s["d_block"] >= 1 + s["margin"] + slack, note
            reach = max(_reach(s["d_block"] * 1.0001, max(w - 1e-3, 0)) for w in walls)
            assert reach <= RB
            if k == "7":
                assert reach == (4 if three_d else 3), (note, reach)
        elif k == "8":
            out = np.maximum(-s["u"], s["u"] - 1).max()
            assert not s["inside"] and abs(out - float(note.split()[0])) < 1e-6, (note, out)
        elif k == "9c":  # NaN canonical points in the answer's cell or in a shell-1 neighbour that is read, below / above its index
            nanp = np.flatnonzero(np.isnan(c["canon"]).any(1))
            ncell = S.cell_coordinates(geo, c["canon"][nanp])[0]
            assert own_answer, note
            if note.startswith("NaN in"):
                kind = note.split()[2].rstrip(",")
                nan_axes = np.isnan(c["canon"][nanp])
                right_kind = (nan_axes == np.array([a in kind for a in "xyz"])).all(1)
                if "same cell" in note:
                    where = (ncell == s["cell"]).all(1)
                else:
                    a, sign = "xyz".index(note.split("along ")[1][1]), 1 if note.split("along ")[1][0] == "+" else -1
                    where = (ncell == s["cell"] + sign * np.eye(3, dtype=int)[a]).all(1)
                    # shell 0 does not settle, and the neighbour is not pruned: its wall is nearer than the answer
                    assert s["d"] >= s["margin"] + slack and (s["u"][a] if sign < 0 else 1 - s["u"][a]) + slack <= s["d"], note
                there = right_kind & where
                assert ("below" not in note or (there & (nanp < idx[i])).any()) and ("above" not in note or (there & (nanp > idx[i])).any()), note
                if "and" not in note:  # exactly the one NaN point of this scenario there
                    assert there.sum() == 1, note
            else:
                assert ((ncell == s["answer_cell"]).all(1) & (nanp < idx[i])).any(), note
        elif k == "10":
            same = np.flatnonzero((c["canon"] == c["canon"][idx[i]]).all(1))
            assert len(same) == 3 and idx[i] == same.min() and same.max() - same.min() > 16, note
    assert ball_attempts == {0, 1, 2, None}
    # class 2 covers every wall, four edges and (in three dimensions) four corners of different signs
    across = [n for k, n in zip(c["cls"], c["note"]) if k == "2"]
    n_axes = [len(n.split()) - 1 for n in across]
    assert n_axes.count(1) == (6 if three_d else 4) and n_axes.count(2) >= 4 and n_axes.count(3) == (4 if three_d else 0)
    assert len(set(across)) == len(across)


@pytest.mark.parametrize("name", sorted(Cc.GRIDS))
def test_wave_composition(name):
    c = Cc.grid_case(name)
    o = Cc.orders(name)
    base = set(range(len(c["queries"])))
    assert set(o["interleaved"]) == base and set(o["grouped"]) == base
    for wave in range(0, len(o["interleaved"]), 64):
        assert len(set(c["cls"][o["interleaved"][wave:wave + 64]])) >= 4
    assert len(o["grouped"]) % 64 == 0
    for wave in range(0, len(o["grouped"]), 64):
        assert len(set(c["cls"][o["grouped"][wave:wave + 64]])) == 1
    n = len(o["ragged"])
    assert n % 64 == 1 and n % 256 != 0
    last = o["ragged"][-1]
    assert c["cls"][last] == "5" and c["note"][last].startswith("2.6")  # one growing ball alone in the last wave


# ------------------------------------------------------------------------------------------ against the oracle and warp_statement
@pytest.mark.parametrize("name", sorted(Cc.GRIDS))
def test_nearest_equals_the_oracle_on_the_finite_queries(name):
    c = Cc.grid_case(name)
    idx, d2 = Cc.expected(name)
    fin = Cc.finite_queries(c)
    # (the oracle states nanoflann's insertion loop: a NaN distance ahead of the list is kept — put the NaN point of
    # index 0 behind a finite one for it; a NaN query is outside its contract, tests/test_warp_statement_cpu.py)
    assert np.isnan(c["canon"][0]).all() and (idx[fin] > 0).all()
    _, _, ridx = O.correspond(c["canon"][1:], None, c["queries"][fin], threads=8)
    assert np.array_equal(idx[fin], ridx + 1)
    assert (idx[~fin] == -1).sum() >= (0 if fin.all() else 5)
    if len(c["canon"]) <= 4096:  # (warp_statement.knn orders an infinite distance like a NaN one: finite queries only)
        assert np.array_equal(idx[fin], W.knn(c["canon"], c["queries"][fin], 1)[:, 0])
    v, n = S.gather(c["canon"], c["normals"], idx)
    assert np.array_equal(v[fin], c["canon"][idx[fin]]) and np.array_equal(n[fin], c["normals"][idx[fin]])
    assert np.array_equal(S.gather(c["canon"], None, np.array([-1]))[0].view(np.uint32), c["canon"][:1].view(np.uint32)) and S.gather(c["canon"], None, idx)[1] is None


def test_nearest_non_finite_contract():
    cv = np.array([[np.nan, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]], f32)
    lv = np.array([[0.1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, np.inf, 0], [0.9, 0, 0]], f32)
    idx, d2 = S.nearest(cv, lv, qchunk=2, cchunk=3)
    assert idx.tolist() == [1, -1, 1, 1, 2]  # an infinite distance is a neighbour, a NaN one never; ties to the lower index
    assert np.isnan(d2[1]) and np.isinf(d2[2]) and d2[0] == f32(0.1) * f32(0.1)
    assert S.nearest(cv[:1], lv)[0].tolist() == [-1] * 5  # every distance NaN
    inf_cv = np.array([[np.inf, 0, 0], [0, 0, 0]], f32)  # inf - inf is NaN: the finite point is the only neighbour
    assert S.nearest(inf_cv, lv[2:3])[0].tolist() == [1]
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 4, (700, 3)).astype(f32), rng.integers(0, 4, (300, 3)).astype(f32)  # massive ties
    assert np.array_equal(S.nearest(a, b, qchunk=64, cchunk=100)[0], W.knn(a, b, 1)[:, 0])


@pytest.mark.parametrize("n_canon,n_live,form", Cc.THRESHOLDS)
def test_search_form_on_both_sides_of_every_threshold(n_canon, n_live, form):
    assert S.search_form(n_canon, n_live) == form
    assert (S.search_form(n_canon, n_live) != "scan") == W.want_grid(n_canon, n_live)
    if n_canon <= 16384:
        canon, live = Cc.threshold_case(n_canon, n_live)
        m = min(n_live, 2000)
        assert np.array_equal(S.nearest(canon, live[:m])[0], O.correspond(canon, None, live[:m], threads=8)[2])


def test_fma32_is_the_fused_multiply_add():
    rng = np.random.default_rng(1)
    a, b, c = (rng.standard_normal(20000).astype(f32) * f32(10.0) ** rng.integers(-3, 4, 20000).astype(f32) for _ in range(3))
    from fractions import Fraction
    got = S.fma32(a, b, c)
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((float(got[i]), float(np.nextafter(got[i], f32(np.inf if exact > Fraction(float(got[i])) else -np.inf)))))
        assert Fraction(lo) <= exact <= Fraction(hi)
        other = hi if float(got[i]) == lo else lo
        assert abs(exact - Fraction(float(got[i]))) <= abs(exact - Fraction(other))
    # a product whose fp64 sum with c rounds onto a float32 tie: 1 + 2^-24 + 2^-60 must round up, not to even
    assert S.fma32(np.array([f32(1 + 2.0 ** -12)]), np.array([f32(1 + 2.0 ** -12)]), np.array([f32(2.0 ** -60)]))[0] > f32(1 + 2.0 ** -11)


# ------------------------------------------------------------------------------------------ projective
@pytest.mark.parametrize("cols,rows,principal", Cc.PROJECTIVE_CASES)
@pytest.mark.parametrize("with_normals,with_nmap", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("zero_thresh", [False, True])
def test_projective_equals_the_oracle_bit_for_bit(cols, rows, principal, with_normals, with_nmap, zero_thresh):
    c = Cc.projective_case(cols, rows, principal)
    args = (*c["intr"], 0.0 if zero_thresh else c["dist_thresh"], c["min_cosine"])
    nr, nm = c["normals"] if with_normals else None, c["nmap"] if with_nmap else None
    v, n, pix, tie = S.projective(c["vertices"], nr, c["vmap"], nm, *args)
    assert not tie.any()  # a condition on the inputs, not a tolerance
    rv, rn, rp = O.correspond_projective(c["vertices"], nr, c["vmap"], nm, *args)
    assert np.array_equal(pix, rp) and np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert (n is None) == (rn is None) == (not with_nmap)
    if with_nmap:
        assert np.array_equal(n.view(np.uint32), rn.view(np.uint32))
    assert np.isnan(v[pix < 0]).all() and (n is None or np.isnan(n[pix < 0]).all())
    e = c["edges"]
    for name, ok in c["expect"].items():
        if zero_thresh:
            ok = ok and name in ("exact hit", "map vertex y NaN") or (name.startswith("cosine =") and ok)
            if name.startswith("cosine one") or name == "map normal x NaN":
                ok = False
        if name.startswith("cosine one") and not (with_normals and with_nmap):
            ok = True
        if name == "map normal x NaN" and not with_nmap:
            ok = True
        assert (pix[e[name]] >= 0) == ok, (name, pix[e[name]])
    assert 5 < (pix[len(e):] >= 0).sum() < 300 - 5 or zero_thresh  # the random vertices fall on both sides of the gates
    # the distance gate's two edges are exactly on the threshold and exactly one float32 ulp of the squared distance above it
    t2 = f32(c["dist_thresh"]) * f32(c["dist_thresh"])
    jc, ic = int(c["intr"][2]) + 1, int(c["intr"][3]) + 1
    for name, want in (("distance = dist_thresh", t2), ("squared distance one ulp above", np.nextafter(t2, f32(np.inf)))):
        sd = c["vertices"][e[name]] - c["vmap"][ic, jc, :3]
        assert S.dot32(sd[None], sd[None])[0] == want, name
        assert pix[e[name]] in (-1, ic * cols + jc)
    # a pitched map: a column slice of a wider image is the same map
    wide_v, wide_n = (np.concatenate([m, np.full_like(m, 7.0)], 1) for m in (c["vmap"], c["nmap"]))
    pv, pn, pp, _ = S.projective(c["vertices"], nr, wide_v[:, :cols], None if nm is None else wide_n[:, :cols], *args)
    assert np.array_equal(pp, pix) and np.array_equal(pv.view(np.uint32), v.view(np.uint32))
