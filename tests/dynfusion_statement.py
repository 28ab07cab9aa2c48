"""The wiring of one reference-mode frame (DynFusion::frame with north_star = 0: the port of the reference's
dyn_fusion.cpp:48-145, with Warpfield::warpToLive / update and CombinedSolver), stage by stage, composed from the statements
the kernels are already held to.  No new arithmetic beyond the Tukey biweight (written from the reference's
opt_solver.cpp:204-231 and energy.t:50-55, not from csrc/solve_*.hip): every stage calls the existing statement module on the
inputs a RECORD holds (tests/dynfusion_cases.py: what the device left behind after a frame), so that a last-bit difference in
one stage does not cascade into the next.

    a  measured        dists, filtered depth, live volume (camera at the origin)            img_statement, tsdf_statement
    b  live cloud      the marching-cubes soup of the recorded live volume, its normals     mc_statement, tsdf_statement
    c  warped          getCanonicalWarpedToLive(): the canonical cloud under the transforms warp_statement.warp
                       from BEFORE the frame's solve (warpToLive runs before solveAll); one
                       k-NN search per warp, none where the cached graph serves (Warpfield::warpGraphSearches)
    d  correspondence  per live vertex the nearest warped vertex, ties to the lower index   correspond_statement
    e  solve           t recovered from the nodes; Tukey weights; initial and final cost    solve_statement.Statement
    f  fusion          the canonical volume through the solved D_before nodes               tsdf_warped_statement
    g  growth          the appended nodes: where, how heavy, from which transforms          warp_statement, oracle.voxel_grid

Stage e.  The solve's "canonical" cloud is the recorded corresponding frame, its data graph the k-NN of those points among the
nodes of `before`, its unknown starts at t = 0 and is composed DQ(0,0,0,t) * dg_se3 on the left: for every node the rotation
part after the frame is the one before it and the dual part differs by 1/2 (0, t) r, which recovers t.  The Tukey weight of a
row is the reference's: the corresponding point warped by calcDQB under the transforms before the solve, its distance to the
live vertex divided by tukeyOffset, (1 - d^2 / psi^2)^2 below psi_data and 0 from there on.  With those weights Statement.cost
at t = 0 is the device's initial cost.  SolveState::final_cost is booked by the closing linearisation (mode 2) that
dfa_solver_solve enqueues behind the last PCG, with the weights frozen: it belongs to the RECOVERED t (the translations the
nodes took), not to the last linearisation's — so the device's final cost is Statement.cost at the recovered t.

The cost bar (cost_budget) is first order in float32, summed over rows as Statement6.cost_bud is: per row the error of the
weight (4 (1 - d^2 / psi^2) d / psi^2 times the error of d, which is the float32 warp's KERNEL_BOUND L sqrt(3) / tukeyOffset),
of the residual (its inputs rounded once, k + 1 steps of the sum, the recovered t's last bits) and of the squares, plus, for the
rows whose d lies within that error of psi_data, the most they can carry: (1 - (1 - dd / psi)^2)^2 |e|^2.

frame(before, after, inputs, case) returns the list of failed checks, [] when the frame is as stated.  `defect=` plants one
of DEFECTS into the stated side.  compose_right cannot show on a sequence of this mode: seeds start at the identity, a solve
composes pure translations and calcDQB multiplies real parts that are all (1, 0, 0, 0), so every rotation stays the identity
and left and right composition are the same dual quaternion, bit for bit (the CPU test plants it on nodes that are rotated)."""
import numpy as np

import correspond_statement as CO
import dynfusion_cases as C
import img_statement as I
import kinfu_statement as K
import mc_statement as MS
import tsdf_statement as T
import tsdf_warped_statement as WST
import warp_statement as WS
from knn_field_statement import AMBIGUOUS_CAP
from solve_statement import U32, Statement, knn_graph, rbf_weights
from tsdf_warped6_check import check  # the comparison and undecided-voxel rule of test_gpu_tsdf_warped.py, max_weight a parameter

f32 = np.float32
same = C.same
STAGES = "abcdefg"
LEAF = 0.05  # Warpfield::update's voxel grid
SUPPORT_KNIFE = 1e-5
DQB_BAR = 2e-6  # tests/test_gpu_warp.py: calc_dqb against the statement (= warp_statement.KERNEL_BOUND rounded up)

# name -> (what the frame would do instead, the stages that show it, the case whose record shows it)
DEFECTS = {
    "warp_solved": ("the warp under the solved transforms", "c", "plain"),
    "stale_graph": ("the warp with the k-NN graph of the previous node count", "c", "fused_field_rigid"),
    "correspond_swapped": ("the correspondence direction swapped (canonical -> live)", "d", "plain"),
    "solve_unwarped": ("the solve fed the unwarped canonical cloud", "e", "plain"),
    "compose_right": ("t composed on the right: dg_se3 * DQ(t)", "e", "plain"),
    "t_from_previous": ("t started from the previous frame's translation", "e", "plain"),
    "fuse_start": ("the fusion through the start transforms", "f", "fused_search_skip"),
    "fuse_after_nodes": ("the fusion through the nodes after the growth", "f", "fused_field_rigid"),
    "mode_swapped": ("UnsupportedMode Skip and Rigid swapped", "f", "fused_search_skip"),
    "growth_solved": ("the growth from the cloud under the solved transforms", "g", "plain"),
    "weight_3eps": ("new nodes at weight 3 epsilon", "g", "plain"),
    "dqb_identity": ("new nodes' transforms from the identity", "g", "plain"),
}


# ------------------------------------------------------------------------------------------------------- helpers ----
def volume_to_camera(case):
    """camera^-1 * volume_pose with the camera at the origin, in the host's float32 (TsdfVolume::integrate / integrateWarped)"""
    return K.aff_mul(K.aff_inv(K.IDENTITY), case.kinfu.volume_pose)


_TABLES = []


def tables():
    if not _TABLES:
        from mc_util import default_tables
        _TABLES.extend(default_tables())
    return _TABLES


def same_nan(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)))


def coordinate_scale(*arrays):
    """L of tsdf_warped_statement: KERNEL_BOUND is the float32 warp's deviation at coordinates of order 1 and scales with them"""
    return max([1.0] + [float(np.abs(a).max()) for a in arrays if len(a)])


# ------------------------------------------------------------------------------------------------------- stages ----
def measured(depth, case):
    """stage a -> dict of arrays"""
    p = case.kinfu
    dists = T.compute_dists(depth, *p.intr)
    d0 = I.bilateral(depth, p.bilateral_kernel_size, p.bilateral_sigma_spatial, p.bilateral_sigma_depth)
    if p.icp_truncate_depth_dist > 0:
        d0 = I.truncate_depth(d0, p.icp_truncate_depth_dist)
    vol = T.integrate(T.clear(tuple(p.volume_dims[::-1])), dists, p.voxel_size, p.trunc, p.tsdf_max_weight, volume_to_camera(case), *p.intr)
    return dict(dists=dists, depth0=d0, live_volume=vol)


def surface(volume, case):
    """stage b: DynFusion::extractSurface -> (vertices (n, 3): xyz of the float4 soup; normals (n, 3): the TSDF gradient with
    mesh_normals, else default-constructed)"""
    p = case.kinfu
    tri, nv = tables()
    v, _ = MS.marching_cubes(volume, p.voxel_size, tri, nv)
    if case.mesh_normals:
        n = T.vertex_normals(volume, p.voxel_size, p.gradient_delta_factor, v)[:, :3]
    else:
        n = np.zeros((len(v), 3), np.float32)
    return np.ascontiguousarray(v[:, :3]), np.ascontiguousarray(n, np.float32)


def warped(before, after, case, defect=None):
    """stage c -> (vertices, normals) float64: the canonical cloud of `before` under its nodes and transforms"""
    pos, w, dq = before["node_pos"], before["node_w"], before["node_dq"]
    if defect == "warp_solved":
        dq = after["node_dq"][:before["D"]]
    verts, normals = before["canonical_v"], before["canonical_n"]
    if defect == "stale_graph":  # the graph searched when the field had the node count of the frame before
        idx = WS.knn(pos[:before["prev_D"]], verts, case.k)
        return WS.warp_graph(pos, dq, w, idx, verts, normals)
    return WS.warp(pos, dq, w, case.k, verts, normals)


def correspondence(after, defect=None):
    """stage d -> (vertices, normals) float32, from the recorded warped and live clouds"""
    if defect == "correspond_swapped":
        idx, _ = CO.nearest(after["live_v"], after["warped_v"])
        return CO.gather(after["live_v"], after["live_n"], idx)
    idx, _ = CO.nearest(after["warped_v"], after["live_v"])
    return CO.gather(after["warped_v"], after["warped_n"], idx)


def recover_t(dq_before, dq_after, right=False):
    """stage e: t with dq_after = DQ(0,0,0,t) * dq_before (right: dq_before * DQ(0,0,0,t)) -> (t (D, 3) float64, the scalar part
    2 (d' - d) r* should not have, the bits t can be off by: the roundings of the host's float32 product)"""
    b, a = np.asarray(dq_before, np.float64), np.asarray(dq_after, np.float64)
    conj = b[:, :4] * np.array([1.0, -1, -1, -1])
    diff = a[:, 4:] - b[:, 4:]
    q = 2.0 * (WS.qmul(conj, diff) if right else WS.qmul(diff, conj))
    dt = 8 * U32 * (np.abs(a[:, 4:]).max(1) + np.abs(b[:, 4:]).max(1) + 1e-30)
    return q[:, 1:], np.abs(q[:, 0]), dt


def tukey(node_pos, node_dq, node_w, k, canon, live, offset, psi):
    """CombinedSolver::updateTukeyBiweights / calcTukeyBiweight (opt_solver.cpp:204-231) -> (tau float64 (N,), d (N,): the scaled
    distance the cut-off is applied to).  The corresponding point is warped by calcDQB under the nodes' transforms — again:
    it already is a vertex of the warped cloud —, the error is live - warped, d = |error| / tukeyOffset."""
    wv, _ = WS.warp(node_pos, node_dq, node_w, k, canon)
    e = np.asarray(live, np.float32).astype(np.float64) - wv
    d = np.sqrt((e * e).sum(1)) / float(f32(offset))
    c = float(f32(psi))
    with np.errstate(all="ignore"):
        tau = np.where(d < c, (1.0 - d * d / (c * c)) ** 2, 0.0)
    return tau, d


def solve_statement(nodes, canon, live, case, t=None):
    """stage e, nodes = (positions, transforms, weights) -> (Statement at t, tau, d, data graph)"""
    pos, dq, w = nodes
    idx = WS.knn(pos, canon, case.k)
    tau, d = tukey(pos, dq, w, case.k, canon, live, case.tukeyOffset, case.psi_data)
    S = Statement(pos, w, case.k, canon, live, idx, tau, float(f32(case.lambda_)), t=t)
    return S, tau, d, idx


def cost_budget(nodes, canon, live, case, tau, d, idx, t, dt):
    """the first-order float32 bound on |cost_device - Statement.cost| described in the module's docstring -> (budget, rows
    within float32 resolution of the cut-off)"""
    pos, _, w = nodes
    k, N, D = case.k, len(canon), len(pos)
    c, off = float(f32(case.psi_data)), float(f32(case.tukeyOffset))
    L = coordinate_scale(canon, live, pos)
    dd = (WS.KERNEL_BOUND * L * np.sqrt(3.0) + 4 * U32 * L) / off + 2 * U32 * d  # of d: the float32 warp, the difference, root and divide
    t = np.zeros((D, 3)) if t is None else t
    dt = np.zeros(D) if dt is None else dt
    rw = rbf_weights(pos, w, canon, idx)
    j = np.maximum(idx, 0)
    arg = -np.log(np.maximum(rw, 1e-300))
    w_err = 8 * U32 * (1.0 + arg) * rw  # a float32 exp of a float32 argument
    wt = np.abs(rw[..., None] * t[j]).sum(1)
    b = np.asarray(live, np.float32).astype(np.float64) - np.asarray(canon, np.float32).astype(np.float64)
    e = b - (rw[..., None] * t[j]).sum(1)
    e_err = (U32 * np.abs(b) + (k + 1) * U32 * wt + U32 * np.abs(e) + (w_err[..., None] * np.abs(t[j])).sum(1)
             + (rw * dt[j])[..., None].sum(1))
    e2 = (e * e).sum(1)
    near = np.abs(d - c) <= dd
    with np.errstate(all="ignore"):
        dtau = np.where(d < c, 4.0 * (1.0 - d * d / (c * c)) * d / (c * c) * dd, 0.0) + 4 * U32 * tau
    x = np.minimum(dd / c, 1.0)
    edge = np.where(near, (1.0 - (1.0 - x) ** 2) ** 2 * e2, 0.0)
    data = (np.where(near, 0.0, dtau * e2) + tau * (2.0 * (np.abs(e) * e_err).sum(1) + 8 * U32 * e2) + edge).sum()
    # the regulariser: tau = w_reg^2 rounded (3 u), e = t_m - t_n of float32 translations
    reg = 0.0
    if t.any():
        ridx = knn_graph(pos, pos, k)
        n_of = np.repeat(np.arange(D), k)
        m_of = ridx.reshape(-1)
        keep = (m_of >= 0) & (m_of != n_of)
        er = t[m_of[keep]] - t[n_of[keep]]
        err = 2 * U32 * np.abs(er) + (dt[m_of[keep]] + dt[n_of[keep]])[:, None]
        reg = float(f32(case.lambda_)) / (D * k) * ((2.0 * np.abs(er) * err).sum() + 11 * U32 * (er * er).sum())
    return float(data + reg), int(near.sum())


def fusion(before, after, case, dq, defect=None):
    """stage f -> tsdf_warped_statement.integrate's dict"""
    p = case.kinfu
    mode = WST.RIGID if case.fuse_unsupported_rigid else WST.SKIP
    if defect == "mode_swapped":
        mode = WST.SKIP if mode == WST.RIGID else WST.RIGID
    nodes = (before["node_pos"], dq, before["node_w"])
    if defect == "fuse_after_nodes":
        nodes = (after["node_pos"], after["node_dq"], after["node_w"])
    return WST.integrate(before["canonical_volume"], after["dists"], p.voxel_size, p.trunc, p.tsdf_max_weight, volume_to_camera(case),
                         *p.intr, *nodes, case.k, mode)


def unsupported_in_band(after, case, ref):
    """stage f: the voxels no node supports that an integration where they stand would update (inside the image, before the
    surface or within the truncation distance behind it) — where Skip and Rigid differ"""
    p = case.kinfu
    free = ~ref["supported"].ravel()
    v = WST.voxel_positions(ref["supported"].shape, p.voxel_size)[free].astype(np.float64)
    a = np.asarray(volume_to_camera(case), np.float32).astype(np.float64)
    vc = v @ a[:9].reshape(3, 3).T + a[9:12]
    return int(WST.probe(vc.astype(np.float32), after["dists"], p.trunc, *p.intr)[0].sum())


def growth(before, after, case, defect=None):
    """stage g -> dict(seeds, weight, dq (float64), knife: a vertex the node set hinges on: a support quotient within
    SUPPORT_KNIFE of 1).  The north-star statement's stage j also sets aside a seed whose k-th and (k + 1)-th nearest nodes tie
    before it compares transforms; here calc_dqb's own k-NN contract (ties to the lower index) is held to as it stands, which
    errs on the strict side: on another scene a float32 tie could fail this stage spuriously, never pass it wrongly."""
    import oracle
    Db = before["D"]
    pos, w = before["node_pos"], before["node_w"]
    solved = after["node_dq"][:Db]
    verts = after["warped_v"]
    if defect == "growth_solved":
        verts = WS.warp(pos, solved, w, case.k, before["canonical_v"])[0].astype(np.float32)
    flags = WS.unsupported_flags(pos, w, case.k, verts)
    q = WST.support_quotients(pos, w, WS.knn(pos, verts, case.k), verts).astype(np.float64)
    knife = bool((np.abs(q - 1.0) <= SUPPORT_KNIFE).any())
    seeds = oracle.voxel_grid(np.ascontiguousarray(verts[flags == 1]), LEAF) if flags.any() else np.zeros((0, 3), np.float32)
    if defect == "dqb_identity":
        dq = np.tile(WS.IDENTITY, (len(seeds), 1))
    else:
        dq = WS.calc_dqb(pos, solved, w, case.k, seeds) if len(seeds) else np.zeros((0, 8))
    weight = f32(3 if defect == "weight_3eps" else 2) * f32(case.epsilon)
    return dict(seeds=seeds, weight=weight, dq=dq, knife=knife, unsupported=int(flags.sum()))


# ------------------------------------------------------------------------------------------------------ the frame ----
def _try(bad, label, fn, *a):
    try:
        fn(*a)
    except AssertionError as e:
        bad.append("%s: %s" % (label, e))


def frame(before, after, inputs, case, defect=None, stages=STAGES, info=None):
    """One frame's record `after` against the stages stated from `before` (None: the first frame) and the frame's inputs
    (dict: index, depth).  -> the failed checks; `info` (a dict) receives the figures of the write-up."""
    assert defect is None or defect in DEFECTS, defect
    info = {} if info is None else info
    bad = []
    i = inputs["index"]
    p = case.kinfu
    first = before is None
    tag = lambda s: "%s frame %d %s" % (case.name, i, s)

    if "a" in stages:
        want = measured(inputs["depth"], case)
        bad += [tag("a " + k) for k, v in want.items() if not same(v, after[k])]
        if bool(after["result"]) != (not first) or after["counter"] != i + 1:
            bad.append(tag("a result / counter"))

    if "b" in stages:
        v, n = surface(after["live_volume"], case)
        cloud = "canonical" if first else "live"  # frame 0's surface becomes the canonical frame
        if not same(after[cloud + "_v"], v):
            bad.append(tag("b %s cloud: %d vertices, statement %d" % (cloud, len(after[cloud + "_v"]), len(v))))
        elif not same_nan(after[cloud + "_n"], n):
            bad.append(tag("b %s normals" % cloud))
        info["vertices"] = len(v)

    if first:
        return bad + _first_frame(after, case, stages, tag, info)

    Db = before["D"]
    k = case.k
    if after["knn"] != k:
        bad.append(tag("the warp field's k is %d, not %d" % (after["knn"], k)))
    for name in ("canonical_v", "canonical_n"):
        if not same(after[name], before[name]):
            bad.append(tag("the canonical cloud changed (%s)" % name))

    # ---- c
    if "c" in stages:
        wv, wn = warped(before, after, case, defect)
        if len(after["warped_v"]) != len(wv):
            bad.append(tag("c size"))
        else:
            ev, en = WS.deviation(after["warped_v"], wv), WS.deviation(after["warped_n"], wn)
            # the graph cache's key is the cloud's device array, N, D and k: the cloud never changes, k is set once behind frame 0,
            # so a frame searches unless the frame before it appended no node (frame 1: nothing is cached yet)
            reuse = i >= 2 and before["prev_D"] == Db
            searched = after["warp_graph_searches"] - before["warp_graph_searches"]
            info["warped"] = dict(vertices=ev, normals=en, bound=WS.KERNEL_BOUND, reused_graph=bool(reuse), searched=searched)
            if ev > WS.KERNEL_BOUND or en > WS.KERNEL_BOUND:
                bad.append(tag("c warped cloud: vertices %.3g, normals %.3g over the bound %.3g" % (ev, en, WS.KERNEL_BOUND)))
            if searched != (0 if reuse else 1):
                bad.append(tag("c the warp ran %d k-NN searches where %s" % (searched, "the cached graph serves" if reuse else "the node set has grown")))

    # ---- d
    if "d" in stages:
        cv, cn = correspondence(after, defect)
        if not same(after["corresponding_v"], cv) or not same_nan(after["corresponding_n"], cn):
            differ = int((C.bits(after["corresponding_v"]) != C.bits(cv)).any(1).sum()) if cv.shape == after["corresponding_v"].shape else -1
            bad.append(tag("d corresponding frame: %d vertices differ" % differ))
        lv = np.ascontiguousarray(after["live_v"]).view(np.dtype((np.void, 12))).ravel()
        info["live_ties"] = 1.0 - len(np.unique(lv)) / max(len(lv), 1)

    # ---- e
    nd = (before["node_pos"], before["node_dq"], before["node_w"])
    solved = after["node_dq"][:Db]
    if "e" in stages:
        t, scalar, dt = recover_t(before["node_dq"], solved, right=defect == "compose_right")
        if not np.array_equal(solved[:, :4], before["node_dq"][:, :4]):
            bad.append(tag("e a node's rotation changed"))
        if not (scalar <= dt).all():
            bad.append(tag("e the dual parts did not change by a pure translation on the left: scalar part %.3g" % scalar.max()))
        if not same(after["node_pos"][:Db], before["node_pos"]) or not same(after["node_w"][:Db], before["node_w"]):
            bad.append(tag("e old nodes' positions or weights changed"))
        canon, live = after["corresponding_v"], after["live_v"]
        if defect == "solve_unwarped":
            idx, _ = CO.nearest(before["canonical_v"], live)
            canon = CO.gather(before["canonical_v"], None, idx)[0]
        t0 = None
        if defect == "t_from_previous":  # what the nodes that existed then took in the frame before
            t0 = np.zeros((Db, 3))
            t0[:before["prev_D"]] = recover_t(before["prev_node_dq"], before["node_dq"][:before["prev_D"]])[0]
        S0, tau, d, idx = solve_statement(nd, canon, live, case, t=t0)
        S1 = Statement(nd[0], nd[2], k, canon, live, idx, tau, float(f32(case.lambda_)), t=t)
        bud0, near = cost_budget(nd, canon, live, case, tau, d, idx, t0, None)
        bud1, _ = cost_budget(nd, canon, live, case, tau, d, idx, t, dt)
        info["cost"] = dict(initial=(after["initial_cost"], S0.cost, bud0), final=(after["final_cost"], S1.cost, bud1), near=near / len(canon),
                            zero=float((tau == 0).mean()), partial=float(((tau > 0) & (tau < 1)).mean()), tmax=float(np.abs(t).max()))
        if not abs(after["initial_cost"] - S0.cost) <= bud0:
            bad.append(tag("e initial cost %.9g, statement %.9g, budget %.3g" % (after["initial_cost"], S0.cost, bud0)))
        if not abs(after["final_cost"] - S1.cost) <= bud1:
            bad.append(tag("e final cost %.9g, statement %.9g, budget %.3g" % (after["final_cost"], S1.cost, bud1)))
        if not after["final_cost"] <= after["initial_cost"]:
            bad.append(tag("e the cost rose: %.9g -> %.9g" % (after["initial_cost"], after["final_cost"])))
        if near / len(canon) > AMBIGUOUS_CAP:
            bad.append(tag("e rows at the cut-off: share %.4f" % (near / len(canon))))

    # ---- f
    if "f" in stages and case.fuse_canonical:
        ref = fusion(before, after, case, before["node_dq"] if defect == "fuse_start" else solved, defect)
        c = dict(name=tag("f"), vol=before["canonical_volume"], trunc=p.trunc, ref=ref, max_weight=p.tsdf_max_weight)
        info["fusion"] = dict(undecided=float((~ref["decided"]).mean()), changed=float((after["canonical_volume"] != before["canonical_volume"]).mean()),
                              unsupported_updated=int((ref["updated"] & ~ref["supported"]).sum()),
                              unsupported_in_band=unsupported_in_band(after, case, ref))
        _try(bad, tag("f canonical volume"), check, after["canonical_volume"], c)
        if (~ref["decided"]).mean() > AMBIGUOUS_CAP:
            bad.append(tag("f undecided share %.4f" % (~ref["decided"]).mean()))
        if case.fuse_knn_field and (after["knn_field_nodes"] != Db or after["knn_field_k"] != k):
            bad.append(tag("f the k-NN field holds %d nodes at k = %d, not %d at %d" % (after["knn_field_nodes"], after["knn_field_k"], Db, k)))
        if not case.fuse_knn_field and after["knn_field_nodes"] != 0:
            bad.append(tag("f a k-NN field with the switch off"))
    elif "f" in stages and len(after["canonical_volume"]):
        bad.append(tag("f a canonical volume with the switch off"))

    # ---- g
    if "g" in stages:
        g = growth(before, after, case, defect)
        info["nodes"] = (Db, after["D"])
        info["growth_knife"] = g["knife"]
        if not same(after["node_pos"][:Db], before["node_pos"]) or not same(after["node_w"][:Db], before["node_w"]):
            bad.append(tag("g old nodes changed"))
        if after["D"] > Db and not (after["node_w"][Db:] == g["weight"]).all():
            bad.append(tag("g new weights"))
        if not g["knife"]:  # (a knife-edge vertex, the rule of the north-star statement's stage j: only the old nodes and the new weights)
            new_pos, new_dq = after["node_pos"][Db:], after["node_dq"][Db:]
            if not same(new_pos, g["seeds"]):
                bad.append(tag("g new positions: %d nodes, statement %d" % (len(new_pos), len(g["seeds"]))))
            else:
                err = np.abs(new_dq.astype(np.float64) - g["dq"])
                if len(err) and not (err <= DQB_BAR).all():
                    bad.append(tag("g new transforms: worst |dq - statement| %.3g (bar %.3g)" % (err.max(), DQB_BAR)))
    return bad


def _first_frame(after, case, stages, tag, info):
    """frame 0: the canonical cloud is the surface (stage b), every nodeStep-th vertex seeds a node, the canonical volume starts
    as the live one"""
    bad = []
    if "c" in stages and (not same(after["warped_v"], after["canonical_v"]) or not same_nan(after["warped_n"], after["canonical_n"])):
        bad.append(tag("c frame 0: the warped cloud is not the canonical cloud"))
    if "d" in stages and (len(after["live_v"]) or len(after["corresponding_v"])):
        bad.append(tag("d frame 0: a live or corresponding frame"))
    if "f" in stages:
        if case.fuse_canonical:
            if not same(after["canonical_volume"], after["live_volume"]):
                bad.append(tag("f frame 0: the canonical volume is not the live volume"))
            if after["knn_field_nodes"] != (after["D"] if case.fuse_knn_field else 0):
                bad.append(tag("f frame 0: the field holds %d of %d nodes" % (after["knn_field_nodes"], after["D"])))
        elif len(after["canonical_volume"]):
            bad.append(tag("f a canonical volume with the switch off"))
    if "g" in stages:
        seeds = after["canonical_v"][::case.nodeStep]
        info["nodes"] = (0, after["D"])
        if not same(after["node_pos"], seeds) or not (after["node_w"] == f32(3) * f32(case.epsilon)).all():
            bad.append(tag("g frame 0: the seeds are not every nodeStep-th vertex at weight 3 epsilon"))
        ident = np.zeros((after["D"], 8), np.float32)
        ident[:, 0] = 1
        if not same(after["node_dq"], ident):
            bad.append(tag("g frame 0: a seed's transform is not the identity"))
    return bad


# ------------------------------------------------------------------------------------------------------ the chain ----
def chain_records(case, depths):
    """The statement chain over a case's frames without the device: every stage forwards in numpy, the solve by the project's C
    oracle of the reference's (oracle.solve_ref, float64).  -> the records, as dynfusion_cases.read_records gives them"""
    import oracle
    p = case.kinfu
    lam = float(f32(case.lambda_))
    recs = []
    for i, depth in enumerate(depths):
        before = recs[-1] if recs else None
        searches = 0 if before is None else before["warp_graph_searches"] + (0 if i >= 2 and before["prev_D"] == before["D"] else 1)
        r = dict(result=before is not None, counter=i + 1, warp_graph_searches=searches, initial_cost=0.0, final_cost=0.0, knn_field_nodes=-1, knn_field_k=-1, knn=case.k,
                 canonical_volume=np.zeros(0, np.uint32))
        r.update(measured(depth, case))
        v, n = surface(r["live_volume"], case)
        e3 = np.zeros((0, 3), np.float32)
        if before is None:
            r.update(canonical_v=v, canonical_n=n, warped_v=v, warped_n=n, live_v=e3, live_n=e3, corresponding_v=e3, corresponding_n=e3)
            r["node_pos"] = v[::case.nodeStep].copy()
            r["D"] = len(r["node_pos"])
            r["node_w"] = np.full(r["D"], f32(3) * f32(case.epsilon), np.float32)
            r["node_dq"] = np.zeros((r["D"], 8), np.float32)
            r["node_dq"][:, 0] = 1
            if case.fuse_canonical:
                r["canonical_volume"] = r["live_volume"].copy()
                r["knn_field_nodes"], r["knn_field_k"] = (r["D"], 8) if case.fuse_knn_field else (0, 0)
        else:
            Db = before["D"]
            r.update(canonical_v=before["canonical_v"], canonical_n=before["canonical_n"], live_v=v, live_n=n)
            wv, wn = warped(before, r, case)
            r["warped_v"], r["warped_n"] = wv.astype(np.float32), wn.astype(np.float32)
            r["corresponding_v"], r["corresponding_n"] = correspondence(r)
            t, dq_out, st = oracle.solve_ref(before["node_pos"], before["node_dq"], before["node_w"], case.k, r["corresponding_v"], v,
                                             num_iter=case.one_pass, nonlinear_iter=case.solver_nonLinearIter,
                                             linear_iter=case.solver_linearIter, tukey_offset=case.tukeyOffset, psi_data=case.psi_data,
                                             lambda_=lam, psi_reg=case.psi_reg, threads=8)
            solved = before["node_dq"].copy()
            solved[:, 4:] = (before["node_dq"][:, 4:].astype(np.float64)
                             + 0.5 * WS.qmul(np.concatenate([np.zeros((Db, 1)), t.astype(np.float64)], 1), before["node_dq"][:, :4])).astype(np.float32)
            r.update(node_pos=before["node_pos"], node_w=before["node_w"], node_dq=solved, D=Db)
            nd = (before["node_pos"], before["node_dq"], before["node_w"])
            S0, tau, d, idx = solve_statement(nd, r["corresponding_v"], v, case)
            r["initial_cost"] = S0.cost
            r["final_cost"] = Statement(nd[0], nd[2], case.k, r["corresponding_v"], v, idx, tau, lam, t=recover_t(before["node_dq"], solved)[0]).cost
            r["oracle_costs"] = (st["initial_cost"], st["final_cost"])
            if case.fuse_canonical:
                r["canonical_volume"] = fusion(before, r, case, solved)["vol"]
                r["knn_field_nodes"], r["knn_field_k"] = (Db, case.k) if case.fuse_knn_field else (0, 0)
            g = growth(before, r, case)
            assert not g["knife"], "the chain's field growth hangs on a knife edge"
            m = len(g["seeds"])
            r["node_pos"] = np.concatenate([before["node_pos"], g["seeds"]]).astype(np.float32)
            r["node_w"] = np.concatenate([before["node_w"], np.full(m, g["weight"], np.float32)])
            r["node_dq"] = np.concatenate([solved, g["dq"].astype(np.float32).reshape(m, 8)])
            r["D"] = Db + m
        recs.append(r)
        C.link_records(recs)
    return recs
