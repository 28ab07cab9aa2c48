"""-m gpu: the vertex mask of a north-star plan (dfa_solver6_set_vertex_mask).

A masked-out vertex takes the path of a vertex without association, so a masked solve must be, bit for bit, the solve of the
same problem whose masked vertices had their canonical normals set to zero before set_problem: those fail the cos_thresh gate
(0 < cos_thresh) and keep their place in the graphs and the block pattern.  Scenes are built as _scene of
test_gpu_solve6_normal_equations.py builds them (a copy of that helper: D = 24 nodes, N = 601 vertices — three workgroups of
the linearisation, the last one partly filled), k = 4 and k = 8 (the two K instantiations), one Gauss-Newton iteration for the
matrix checks and 2 x 3 with gn_tol > 0 for the decision path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from dynfu_amd import synth  # noqa: E402
from gpu_util import bits, dev, host  # noqa: E402
from test_gpu_solve6_normal_equations import PRM, ROWB, _check, _statement  # noqa: E402  (that test's comparison and budgets)

D, N = 24, 601
ONE = dict(num_iter=1, gn_iter=1, linear_iter=100, pcg_tol=1e-4, gn_tol=0.0)
DECIDE = dict(num_iter=2, gn_iter=3, linear_iter=64, pcg_tol=1e-3, pcg_tol_first=0.1, pcg_tol_adapt=0.9, gn_tol=1e-3)


@pytest.fixture(scope="module")
def A():
    import dynfu_amd
    dynfu_amd.load()
    return dynfu_amd


_SCENES = {}


def _scene(A, k, frame=6):
    """T0's scene with 24 nodes and 601 of its vertices (computed once per k, never changed)"""
    if (k, frame) not in _SCENES:
        cfg = dict(synth.CONFIGS["T0"], k=k, D=D)
        c = synth.canonical(cfg)
        intr = synth.intrinsics(cfg)
        P, Nm = A.compute_points_normals(dev(synth.depth_frame(cfg, frame)), *intr)
        # every 5th vertex from the 5th on: of the five such subsets the one with the fewest vertices within 1e-3 pixel of a
        # pixel boundary (2 — a property of the scene's projection alone, counted on the host).  The statement calls such
        # vertices ambiguous and the comparison it is used with caps them at 0.6 % of N: 3 of 601
        step = len(c["verts"]) // N
        verts, normals = c["verts"][step - 1::step][:N].copy(), c["normals"][step - 1::step][:N].copy()
        assert len(verts) == N and len(c["node_pos"]) == D
        _SCENES[(k, frame)] = dict(nodes=c["node_pos"], dq=c["node_dq"].copy(), w=c["node_w"], verts=verts, normals=normals,
                                   P=P, Nm=Nm, intr=intr, k=k)
    return _SCENES[(k, frame)]


def _half_mask(seed=3):
    return (np.random.default_rng(seed).random(N) < 0.5).astype(np.uint8)


def _plan(A, sc, normals=None):
    s = A.Solver6(D, N, sc["k"])
    s.set_problem(dev(sc["nodes"]), dev(sc["dq"]), dev(sc["w"]), dev(sc["verts"]), dev(sc["normals"] if normals is None else normals))
    return s


def _solve(A, s, sc, how, P=None, Nm=None):
    s.solve(sc["P"] if P is None else P, sc["Nm"] if Nm is None else Nm, *sc["intr"], A.Solve6Params(**dict(PRM, **how)))
    blocks, cols, cnt, g = (host(x).copy() for x in s.matrix())
    used = np.arange(ROWB)[None, :] < cnt[:, None]  # (slots past a row's count are undefined)
    dg, rg = (host(x).copy() for x in s.graphs())
    return dict(blocks=blocks, cols=cols, cnt=cnt, used=used, g=g, x=host(s.step()).copy(), dq=host(s.node_dq()).copy(), dg=dg,
                rg=rg, st=s.stats(), prm=dict(PRM), linear_iter=how["linear_iter"], tol=how["pcg_tol"])


def _same(a, b, what=""):
    assert np.array_equal(a["cnt"], b["cnt"]), what
    assert np.array_equal(a["cols"][a["used"]], b["cols"][b["used"]]), what
    assert np.array_equal(bits(a["blocks"][a["used"]]), bits(b["blocks"][b["used"]])), what
    for name in ("g", "x", "dq"):
        assert np.array_equal(bits(a[name]), bits(b[name])), (what, name)
    assert a["st"] == b["st"], (what, {n: (a["st"][n], b["st"][n]) for n in a["st"] if a["st"][n] != b["st"][n]})


def _run(A, sc, how, mask=None, normals=None, clear=False, P=None, Nm=None):
    s = _plan(A, sc, normals)
    if mask is not None:
        s.set_vertex_mask(dev(mask))
    if clear:
        s.set_vertex_mask(None)
    out = _solve(A, s, sc, how, P, Nm)
    s.close()
    return out


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("how", [ONE, DECIDE], ids=["one iteration", "2 x 3, gn_tol"])
def test_all_ones_and_a_cleared_mask_are_the_unmasked_solve(A, k, how):
    sc = _scene(A, k)
    plain = _run(A, sc, how)
    assert plain["st"]["valid_first"] > N // 4
    _same(_run(A, sc, how, mask=np.ones(N, np.uint8)), plain, "all ones")
    _same(_run(A, sc, how, mask=np.full(N, 255, np.uint8)), plain, "all 255: any non-zero byte")
    _same(_run(A, sc, how, mask=_half_mask(), clear=True), plain, "set, then cleared")


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("how", [ONE, DECIDE], ids=["one iteration", "2 x 3, gn_tol"])
def test_half_mask_is_the_solve_with_those_normals_zeroed(A, k, how):
    sc = _scene(A, k)
    mask = _half_mask()
    zeroed = sc["normals"].copy()
    zeroed[mask == 0] = 0.0
    masked = _run(A, sc, how, mask=mask)
    ref = _run(A, sc, how, normals=zeroed)
    _same(masked, ref, "half mask against zeroed normals")  # blocks, columns, gradient, step, node_dq, every stat
    for name in ("cost_hist", "valid_hist", "stop_hist"):
        assert masked["st"][name] == ref["st"][name] and len(masked["st"][name]) >= 1
    plain = _run(A, sc, how)
    # the mask took rows away, and not all of them
    assert 0 < masked["st"]["valid_first"] < plain["st"]["valid_first"]
    assert not np.array_equal(bits(masked["g"]), bits(plain["g"]))
    if how is DECIDE:  # every slot of the 2 x 3 loop has its decision, the same on both sides
        assert len(masked["st"]["stop_hist"]) >= 2 * 3 and masked["st"]["gn_solves"] >= 1


@pytest.mark.parametrize("k", [4, 8])
def test_masked_normal_equations_pass_the_fp64_statement(A, k):
    """Statement6 on the zeroed-normal problem, test_gpu_solve6_normal_equations.py's comparison and budgets unchanged"""
    sc = _scene(A, k)
    mask = _half_mask()
    zeroed = sc["normals"].copy()
    zeroed[mask == 0] = 0.0
    out = _run(A, sc, ONE, mask=mask)
    S = _statement(dict(sc, normals=zeroed), out)
    _check(S, out, f"masked, k {k}")
    assert not S.assoc[mask == 0].any() and 0 < S.valid < N


@pytest.mark.parametrize("k", [4, 8])
def test_all_zeros_leaves_no_data_term(A, k):
    import torch
    sc = _scene(A, k)
    none = _run(A, sc, DECIDE, mask=np.zeros(N, np.uint8))
    assert none["st"]["valid_first"] == 0 and none["st"]["valid_last"] == 0 and not any(none["st"]["valid_hist"])
    empty = torch.full_like(sc["P"], float("nan"))
    blind = _run(A, sc, DECIDE, P=empty, Nm=empty)
    _same(none, blind, "all zeros against live maps of NaN")
    assert none["st"]["cost_hist"] == blind["st"]["cost_hist"] and none["st"]["initial_cost"] == blind["st"]["initial_cost"]


@pytest.mark.parametrize("k", [4, 8])
def test_a_masked_vertex_still_warps(A, k):
    sc = _scene(A, k)
    mask = _half_mask()
    s = _plan(A, sc)
    s.set_vertex_mask(dev(mask))
    _solve(A, s, sc, DECIDE)
    wv, wn = s.warp()
    other = _plan(A, sc)  # an unmasked plan over the same nodes, which never solves
    ov, on = other.warp_with(s.node_dq())
    assert np.array_equal(bits(host(wv)), bits(host(ov))) and np.array_equal(bits(host(wn)), bits(host(on)))
    moved = np.abs(host(wv) - sc["verts"]).max(1) > 0
    assert moved[mask == 0].mean() > 0.9 and moved[mask != 0].mean() > 0.9
    s.close(), other.close()


@pytest.mark.parametrize("k", [4, 8])
def test_mask_survives_set_node_transforms_and_goes_with_set_problem(A, k):
    sc = _scene(A, k)
    mask = _half_mask()
    plain, masked = _run(A, sc, ONE), _run(A, sc, ONE, mask=mask)
    s = _plan(A, sc)
    s.set_vertex_mask(dev(mask))
    s.set_node_transforms(dev(sc["dq"]))
    _same(_solve(A, s, sc, ONE), masked, "after set_node_transforms")
    _same(_solve(A, s, sc, ONE), masked, "a second solve")
    s.set_problem(dev(sc["nodes"]), dev(sc["dq"]), dev(sc["w"]), dev(sc["verts"]), dev(sc["normals"]))
    _same(_solve(A, s, sc, ONE), plain, "after set_problem")
    s.close()


def test_mask_without_a_problem_raises(A):
    s = A.Solver6(D, N, 4)
    with pytest.raises(A.DynfuAmdError, match="dfa_solver6_set_vertex_mask: no problem set"):
        s.set_vertex_mask(dev(np.ones(N, np.uint8)))
    with pytest.raises(A.DynfuAmdError, match="no problem set"):
        s.set_vertex_mask(None)
    s.close()
