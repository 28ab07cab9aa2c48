"""The wiring of one north-star frame (DynFusion::northStarFrame), stage by stage, composed from the statements the kernels
are already held to.  Written from DESIGN.md §4.1 and the comments of dynfu/dyn_fusion.hpp; no new arithmetic: every stage
calls the existing statement module on the inputs a RECORD holds (tests/northstar_cases.py: what the device left behind after
a frame), so that a last-bit difference in one stage does not cascade into the next.

    a  measured      dists, filtered depth, live maps, live volume                       img_statement, tsdf_statement
    b  levels        the regularisation hierarchy's node levels                          reg_hierarchy_statement
    c  rigid         the pre-alignment of the start-warped cloud against the live maps   rigid_loop_statement
    d  (composition  start = T o dq_before: seen through e and f)                        rigid_align_statement.compose_rigid
    e  visibility    the rasterised start-warped mesh, the flags of the start-warped cloud   raster_, visibility_statement
    f  solve         the solve's initial cost at the start transforms; dq stay unit      solve6_statement.Statement6
    g  warped        getCanonicalWarpedToLive(): the cloud under the solved transforms   Statement6.p / dp
    h  fusion        the canonical (and colour) volume through the solved D_before nodes tsdf_warped6_, tsdf_color_statement
    i  regrow        the re-extracted cloud, mesh, normals, colours                      mc_min_weight_, tsdf_, color_sample_
    j  growth        the appended nodes: where, how heavy, from which transforms         warp_statement, oracle.voxel_grid

frame(before, after, inputs, case) returns the list of failed checks, [] when the frame is as stated.  `defect=` plants one
of DEFECTS into the stated side; every one of them must make the list non-empty on its record."""
import numpy as np

import color_sample_statement as CS
import img_statement as I
import kinfu_statement as K
import mc_min_weight_statement as FS
import raster_statement as RA
import reg_hierarchy_statement as RH
import rigid_align_statement as RS
import rigid_loop_statement as RL
import tsdf_color_statement as CST
import tsdf_statement as T
import tsdf_warped6_statement as W6
import tsdf_warped_statement as WST
import visibility_statement as VS
import warp_statement as WS
from knn_field_statement import AMBIGUOUS_CAP
from northstar_cases import same
from solve6_statement import Statement6
from tsdf_color_check import check_colors
from tsdf_warped6_check import check

f32 = np.float32
STAGES = "abcefghij"
Z_NEAR = 0.05  # DynFuParams::model_view_z_near
LEAF = 0.05    # Warpfield::update's voxel grid
SUPPORT_KNIFE, TIE_KNIFE = 1e-5, 1e-6

# name -> (what the frame would do instead, the stage that shows it, the case whose record shows it)
DEFECTS = {
    "compose_right": ("T composed on the right: dq o T", "ef", "aligned_visible_fused"),
    "not_composed": ("T not composed: the solve starts from dq_before", "ef", "aligned_visible_fused"),
    "mask_from_before": ("the mask built from the model under dq_before", "e", "aligned_visible_fused"),
    "mask_ignored": ("the mask ignored in the cost", "f", "aligned_visible_fused"),
    "flat_reg": ("the flat regularisation graph where the hierarchy is on", "f", "aligned_visible_fused"),
    "fuse_start": ("the fusion through the start transforms", "h", "aligned_visible_fused"),
    "fuse_after_nodes": ("the fusion through the nodes after the growth", "h", "aligned_visible_fused"),
    "mode_swapped": ("UnsupportedMode Skip and Rigid swapped", "h", "aligned_visible_fused"),
    "field_after_growth": ("the k-NN field synced after the growth", "h", "aligned_visible_fused"),
    "warped_by_start": ("getCanonicalWarpedToLive() under the start transforms", "g", "aligned_visible_fused"),
    "floor_minus_one": ("the regrow at the weight floor minus one", "i", "regrow_colour"),
    "cloud_not_replaced": ("the field grown where the warped OLD cloud has no support", "j", "regrow_colour"),
    "dqb_under_regrow": ("new nodes from calcDQB under regrow", "j", "regrow_colour"),
    "offset0": ("colours sampled with lattice offset 0", "i", "regrow_colour"),
    "prev_color": ("the colour image of the previous frame fused", "h", "regrow_colour"),
}


# ------------------------------------------------------------------------------------------------------- helpers ----
def volume_to_camera(case):
    """DynFusion::volumeToCamera: camera^-1 * volume_pose with the camera at the origin, in the host's float32"""
    return K.aff_mul(K.aff_inv(K.IDENTITY), case.kinfu.volume_pose)


def transform_points(aff12, pts, is_point):
    """dfa_transform_points: ((R0 x + R1 y) + R2 z) + t per row, float32 (raster_statement's vertex arithmetic)"""
    R, t = RA._camera(aff12)
    pts = np.asarray(pts, np.float32)
    with np.errstate(all="ignore"):
        r = RA._rotate(R, [pts[:, 0], pts[:, 1], pts[:, 2]])
        return np.stack([(r[k] + t[k]).astype(np.float32) if is_point else r[k] for k in range(3)], 1)


def graph(node_pos, node_w, verts, k):
    """the k-NN graph of points over nodes and its normalised radial weights -> (idx, wn float64, wn float32)"""
    idx = WS.knn(node_pos, verts, k)
    w64 = WS.weights64(node_pos, node_w, verts, idx)
    nz = (idx >= 0) & (w64.astype(np.float32) > 0)
    tot = w64.sum(1)
    wn64 = np.where(nz, w64 / np.where(tot > 0, tot, 1.0)[:, None], 0.0)
    w32 = w64.astype(np.float32)
    t32 = np.zeros(len(idx), np.float32)
    for j in range(idx.shape[1]):
        t32 = t32 + w32[:, j]
    with np.errstate(all="ignore"):
        wn32 = np.where((t32 > 0)[:, None], w32 / np.where(t32 > 0, t32, f32(1))[:, None], f32(0)).astype(np.float32)
    return idx, wn64, wn32


def blend(dq, g, pts, normals=None, dtype=np.float64):
    """rigid_align_statement.blend_points over a graph(), and the normals the same way (n' = vec(a n a*) / |a|^2); a point no
    weight reaches stays where it is"""
    idx, wn64, wn32 = g
    wn = wn64 if dtype == np.float64 else wn32
    safe = np.maximum(idx, 0)
    with np.errstate(all="ignore"):
        p = RS.blend_points(np.asarray(dq, dtype), safe, wn, np.asarray(pts, dtype), dtype)
    dead = ~(wn != 0).any(1) | ~np.isfinite(p).all(1)
    p = np.where(dead[:, None], np.asarray(pts, dtype), p)
    if normals is None:
        return p
    with np.errstate(all="ignore"):
        n = RS.blend_points(_rot_only(dq, dtype), safe, wn, np.asarray(normals, dtype), dtype)
    n = np.where(dead[:, None], np.asarray(normals, dtype), n)
    return p, n


def _rot_only(dq, dtype):
    """the transforms with their dual parts zeroed: blend_points then rotates"""
    q = np.array(dq, dtype)
    q[:, 4:] = 0
    return q


def compose(dq, T12, defect=None):
    """stage d: the transforms the solve starts from, float32 as the nodes hold them"""
    dq = np.asarray(dq, np.float64)
    if defect == "not_composed" or same(np.asarray(T12, np.float32), K.IDENTITY):
        return dq.astype(np.float32)
    if defect == "compose_right":
        rT, dT = RS.dq_of(T12)
        r, d = dq[:, :4], dq[:, 4:]
        return np.concatenate([RS.qmul(r, rT[None]), RS.qmul(r, dT[None]) + RS.qmul(d, rT[None])], 1).astype(np.float32)
    return RS.compose_rigid(dq, T12).astype(np.float32)


def unit_checks(dq):
    """stage f's checks of the transforms a solve wrote: unit real part within 4 float32 ulps, real . dual = 0 at that scale"""
    dq = np.asarray(dq, np.float64)
    r, d = dq[:, :4], dq[:, 4:]
    norm = np.abs((r * r).sum(1) - 1.0)
    orth = np.abs((r * d).sum(1))
    scale = 1.0 + np.abs(d).sum(1)
    return float(norm.max()), float((orth / scale).max())


# ------------------------------------------------------------------------------------------------------- stages ----
def measured(depth, case, first):
    """stage a -> dict of arrays (the live maps only after the first frame)"""
    p = case.kinfu
    dists = T.compute_dists(depth, *p.intr)
    d0 = I.bilateral(depth, p.bilateral_kernel_size, p.bilateral_sigma_spatial, p.bilateral_sigma_depth)
    if p.icp_truncate_depth_dist > 0:
        d0 = I.truncate_depth(d0, p.icp_truncate_depth_dist)
    out = dict(dists=dists, depth0=d0,
               live_volume=T.integrate(T.clear(tuple(p.volume_dims[::-1])), dists, p.voxel_size, p.trunc, p.tsdf_max_weight,
                                       volume_to_camera(case), *p.intr))
    if not first:
        out["live_points"], out["live_normals"] = I.points_normals(d0, *p.intr)
    return out


def levels(before, case):
    """stage b -> the node levels of the frame's graph (empty with the switch off)"""
    if not case.north_star_reg_hierarchy or case.reg_levels < 2:
        return np.zeros(0, np.int32)
    return RH.node_levels(before["node_pos"], case.epsilon, case.beta, case.reg_levels).astype(np.int32)


def rigid(before, after, case):
    """stage c -> None with the switch off, else dict(pose64, pose32, e32, iters_run, matched, status) of the statement's loop
    on the device's live maps"""
    if not case.north_star_rigid_prealign:
        return None
    p = case.kinfu
    g = graph(before["node_pos"], before["node_w"], before["canonical_v"], case.k)
    v32, n32 = blend(before["node_dq"], g, before["canonical_v"], before["canonical_n"], np.float32)
    gates = dict(dist_thresh=case.distThresh, cos_thresh=case.cosThresh)
    if case.rigid_prealign_device:
        sched = dict(level_step=list(case.rigid_prealign_steps), level_iters=list(case.rigid_prealign_level_iters),
                     stop_rot=float(f32(case.rigid_prealign_stop[0])), stop_trans=float(f32(case.rigid_prealign_stop[1])))
    else:
        sched = dict(level_step=[1], level_iters=[case.rigid_prealign_iters])
    runs = [RL.run(v32, n32, K.IDENTITY, after["live_points"], after["live_normals"], p.intr, gates, fp64=fp64, **sched)
            for fp64 in (False, True)]
    e32 = float(np.abs(runs[0]["aff"].astype(np.float64) - runs[1]["aff"]).max())
    return dict(pose64=runs[1]["aff"], pose32=runs[0]["aff"], e32=e32, iters_run=runs[0]["iters_run"], status=runs[0]["status"],
                matched=(runs[0]["matched_first"], runs[0]["matched_last"]), cloud=(g, v32, n32))


def pose_tolerance(e32, pose):
    return 16.0 * max(e32, 2.0 ** -23 * (1.0 + float(np.abs(np.asarray(pose, np.float64)[9:]).max())))


def visibility(before, after, case, start, defect=None):
    """stage e -> dict(knife, wrong_side, too_far: raster_statement.compare's maps of the device's model map against the mesh
    under the start transforms; flags, undecided: visibility_statement on the device's model map and the start-warped cloud)"""
    p = case.kinfu
    dq = before["node_dq"] if defect == "mask_from_before" else start
    gm = graph(before["node_pos"], before["node_w"], before["mesh_v"][:, :3], case.k)
    mv = blend(dq, gm, before["mesh_v"][:, :3], None, np.float32)
    mesh = np.concatenate([mv, np.ones((len(mv), 1), np.float32)], 1)
    chk = RA.check64(mesh, before["mesh_i"], None, *(float(v) for v in p.intr), Z_NEAR, p.cols, p.rows)
    M = after["model_points"]
    hit = ~np.isnan(M[..., 0])
    zbuf = np.where(hit, np.ascontiguousarray(M[..., 2]).view(np.uint32).astype(np.uint64) << np.uint64(32), RA.MISS)
    knife, wrong, far = RA.compare(zbuf, chk)
    B = blended(before, after, case, dq)
    c64, S = B.p, B.dp
    z_tol = f32(2) * p.voxel_size.max()
    flags, _ = VS.visible_vertices(c64.astype(np.float32), M, *p.intr, z_tol)
    undecided = np.zeros(len(flags), bool)
    for s in np.ndindex(3, 3, 3):
        if s != (1, 1, 1):
            f2, _ = VS.visible_vertices((c64 + S[:, None] * (np.array(s, np.float64) - 1)).astype(np.float32), M, *p.intr, z_tol)
            undecided |= f2 != flags
    return dict(knife=knife, wrong_side=wrong, too_far=far, flags=flags, undecided=undecided)


def blended(before, after, case, dq):
    """Statement6 at transforms dq over the cloud before the frame, for its blend alone: p, dp (the float32 error of p it
    budgets, (40 + 2k) u pmag / min(1, |a|^2)), nw, dn (the same for the normals: the budget of its cos gate)"""
    g = graph(before["node_pos"], before["node_w"], before["canonical_v"], case.k)
    none = np.full((len(before["node_pos"]), case.k), -1, np.int32)
    return Statement6(before["node_pos"], dq, before["node_w"], before["canonical_v"], before["canonical_n"], after["live_points"],
                      after["live_normals"], case.kinfu.intr, case.solve_params, g[0], none, wn=g[1])


def reg_graph(before, case, lv, defect=None):
    """the regularisation graph of the frame: flat (the k nearest other nodes), or the hierarchy's rows"""
    pos, k = before["node_pos"], case.k
    if case.north_star_reg_hierarchy and case.reg_levels >= 2 and defect != "flat_reg":
        return RH.rows(pos, lv, list(case.reg_level_slots[:case.reg_levels]), k)
    idx = WS.knn(pos, pos, k + 1)
    out = np.full((len(pos), k), -1, np.int32)
    for n in range(len(pos)):
        out[n, :] = np.concatenate([[j for j in idx[n] if j != n and j >= 0], [-1] * k])[:k]
    return out


def solve_start(before, after, case, start, flags, lv, defect=None):
    """stage f -> Statement6 at the start transforms with the device's flags as the mask (a masked vertex's normal zeroed: it
    fails the cos gate and takes no data row, tests/test_gpu_solve6_vertex_mask.py)"""
    p = case.kinfu
    g = graph(before["node_pos"], before["node_w"], before["canonical_v"], case.k)
    cn = np.array(before["canonical_n"], np.float32)
    if flags is not None and defect != "mask_ignored":
        cn[np.asarray(flags) == 0] = 0
    return Statement6(before["node_pos"], start, before["node_w"], before["canonical_v"], cn, after["live_points"],
                      after["live_normals"], p.intr, case.solve_params, g[0], reg_graph(before, case, lv, defect), wn=g[1])


def warped(before, after, case, dq):
    """stage g -> (p, dp, n', dn) of the cloud before the frame under transforms dq: Statement6's blend and its budgets"""
    B = blended(before, after, case, dq)
    return B.p, B.dp, B.nw, B.dn


def fusion(before, after, case, inputs, dq, defect=None):
    """stage h -> (ref of tsdf_warped6_statement.integrate, cref of tsdf_color_statement.integrate or None, args)"""
    p = case.kinfu
    mode = W6.RIGID if case.fuse_unsupported_rigid else W6.SKIP
    if defect == "mode_swapped":
        mode = W6.SKIP if mode == W6.RIGID else W6.RIGID
    nodes = (before["node_pos"], dq, before["node_w"])
    if defect == "fuse_after_nodes":
        nodes = (after["node_pos"], after["node_dq"], after["node_w"])
    vol2node, node2cam = volume_to_camera(case), K.aff_mul(K.aff_inv(K.IDENTITY), K.IDENTITY)
    args = (vol2node, node2cam, *p.intr, *nodes, case.k, mode)
    ref = W6.integrate(before["canonical_volume"], after["dists"], p.voxel_size, p.trunc, p.tsdf_max_weight, *args)
    cref = None
    if case.north_star_fuse_color:
        image = inputs["prev_color"] if defect == "prev_color" else inputs["color"]
        cref = CST.integrate(before["color_volume"], image, after["dists"], p.voxel_size, p.trunc, case.canonical_max_color_weight, *args)
        cref["image"] = image
    return ref, cref


def first_colors(after, case, inputs):
    """stage h, frame 0: the colours-only call with no nodes, every voxel where it stands"""
    p = case.kinfu
    return CST.integrate(np.zeros_like(after["canonical_volume"]), inputs["color"], after["dists"], p.voxel_size, p.trunc,
                         case.canonical_max_color_weight, volume_to_camera(case), K.aff_mul(K.aff_inv(K.IDENTITY), K.IDENTITY), *p.intr,
                         None, None, None, case.k, W6.RIGID)


_TABLES = []


def tables():
    if not _TABLES:
        from mc_util import default_tables
        _TABLES.extend(default_tables())
    return _TABLES


def welded_model(volume, case, min_weight):
    """stage i: DynFusion::extractWeldedModel -> (mesh vertices (n, 4) in the camera frame, indices, normals (n, 3))"""
    p = case.kinfu
    tri, nv = tables()
    if min_weight == 0:  # (the floor below 1: a voxel no frame has touched counts as observed too)
        volume = np.where(volume >> 16 == 0, volume | np.uint32(1 << 16), volume).astype(np.uint32)
        min_weight = 1
    v, idx, _ = FS.indexed_min_weight(volume, p.voxel_size, tri, nv, min_weight)
    aff = volume_to_camera(case)
    n4 = T.vertex_normals(volume, p.voxel_size, p.gradient_delta_factor, v)
    vc = transform_points(aff, v[:, :3], True)
    return np.concatenate([vc, np.ones((len(vc), 1), np.float32)], 1), idx, transform_points(aff, n4[:, :3], False)


def soup_model(volume, case):
    """frame 0 without regrow: DynFusion::extractSurface's triangle soup with gradient normals, carried to the camera frame
    -> (vertices (n, 3), normals (n, 3))"""
    import mc_statement as MS
    p = case.kinfu
    tri, nv = tables()
    v, _ = MS.marching_cubes(volume, p.voxel_size, tri, nv)
    aff = volume_to_camera(case)
    n4 = T.vertex_normals(volume, p.voxel_size, p.gradient_delta_factor, v)
    return transform_points(aff, v[:, :3], True), transform_points(aff, n4[:, :3], False)


def model_colors(colors, case, verts, defect=None):
    """stage i: TsdfVolume::sampleColors at lattice offset 0.5 -> color_sample_statement.sample's dict"""
    p = case.kinfu
    to_volume = K.aff_mul(K.aff_inv(p.volume_pose), K.IDENTITY)
    off = f32(0.0 if defect == "offset0" else 0.5)
    for a in range(3):
        to_volume[9 + a] = to_volume[9 + a] - off * p.voxel_size[a]
    delta = CS.deviation(verts, p.voxel_size, to_volume, p.volume_dims)
    return CS.sample(colors, p.voxel_size, verts, to_volume, delta)


def blend_seed(pos, w, dq, k, seeds):
    """stage j with regrow: what dyn_fusion.hpp states for a node appended under north_star_regrow_canonical — the north-star
    blend (Statement6's: the k nearest nodes that existed before, radial weights, every transform in the hemisphere of the
    nearest, real and dual parts summed and divided by the real part's norm) at the seed, in float64 -> (dq (n, 8) float64,
    tie (n,) bool: the k-th and (k + 1)-th node within TIE_KNIFE).  The weights are taken relative to the largest, which the
    division cancels.  The host forms it in double and rounds once, hence growth()'s bar of one float32 ulp per component."""
    pos, w, dq = np.asarray(pos, np.float64), np.asarray(w, np.float64), np.asarray(dq, np.float64)
    s = np.asarray(seeds, np.float64)
    d2 = ((s[:, None, :] - pos[None]) ** 2).sum(2)
    order = np.argsort(d2, axis=1, kind="stable")
    k = min(k, len(pos))
    near = order[:, :k]
    dn = np.take_along_axis(d2, order, 1)
    tie = np.zeros(len(s), bool) if len(pos) <= k else np.abs(dn[:, k] - dn[:, k - 1]) <= TIE_KNIFE * np.maximum(dn[:, k - 1], 1e-300)
    e = -np.take_along_axis(d2, near, 1) / (2 * w[near] ** 2)
    wt = np.exp(e - e.max(1, keepdims=True))
    q = dq[near]
    sg = np.where((q[..., :4] * q[:, :1, :4]).sum(-1) < 0, -1.0, 1.0)
    a = ((wt * sg)[..., None] * q[..., :4]).sum(1)
    b = ((wt * sg)[..., None] * q[..., 4:]).sum(1)
    norm = np.linalg.norm(a, axis=1, keepdims=True)
    return np.concatenate([a / norm, b / norm], 1), tie


def growth(before, after, case, defect=None):
    """stage j -> dict(seeds, weight, dq (float64), bar (per component), knife: a vertex or seed the node set hinges on)"""
    Db = before["D"]
    regrow = bool(case.north_star_regrow_canonical)
    verts = after["canonical_v"] if regrow and defect != "cloud_not_replaced" else after["warped_v"]
    pos, w = before["node_pos"], before["node_w"]
    flags = WS.unsupported_flags(pos, w, case.warp_knn, verts)
    idx = WS.knn(pos, verts, case.warp_knn)
    q = WST.support_quotients(pos, w, idx, verts).astype(np.float64)
    knife = bool((np.abs(q - 1.0) <= SUPPORT_KNIFE).any())
    import oracle
    seeds = oracle.voxel_grid(np.ascontiguousarray(verts[flags == 1]), LEAF) if flags.any() else np.zeros((0, 3), np.float32)
    dq_solved = after["node_dq"][:Db]
    if regrow and defect != "dqb_under_regrow":
        dq, tie = blend_seed(pos, w, dq_solved, case.k, seeds) if len(seeds) else (np.zeros((0, 8)), np.zeros(0, bool))
        bar = np.spacing(np.abs(dq).astype(np.float32)).astype(np.float64)  # double arithmetic rounded once: one float32 ulp
        knife |= bool(tie.any())
    else:
        dq = WS.calc_dqb(pos, dq_solved, w, case.warp_knn, seeds) if len(seeds) else np.zeros((0, 8))
        bar = np.full(dq.shape, 2e-6)  # tests/test_gpu_warp.py: calc_dqb against the statement
    return dict(seeds=seeds, weight=f32(2) * f32(case.epsilon), dq=dq, bar=bar, knife=knife, unsupported=int(flags.sum()))


# ------------------------------------------------------------------------------------------------------ the frame ----
def _try(bad, label, fn, *a):
    try:
        fn(*a)
    except AssertionError as e:
        bad.append("%s: %s" % (label, e))


def frame(before, after, inputs, case, defect=None, stages=STAGES, info=None):
    """One frame's record `after` against the stages stated from `before` (None: the first frame) and the frame's inputs
    (dict: index, depth, color, prev_color).  -> the failed checks; `info` (a dict) receives the figures of the write-up."""
    assert defect is None or defect in DEFECTS, defect
    info = {} if info is None else info
    bad = []
    i = inputs["index"]
    p = case.kinfu
    first = before is None
    tag = lambda s: "%s frame %d %s" % (case.name, i, s)

    if "a" in stages:
        want = measured(inputs["depth"], case, first)
        bad += [tag("a " + k) for k, v in want.items() if not same(v, after[k])]
        if bool(after["result"]) != (not first) or after["counter"] != i + 1:
            bad.append(tag("a result / counter"))

    if first:
        return bad + _first_frame(after, inputs, case, stages, tag, info)

    Db = before["D"]
    # ---- b
    lv = levels(before, case)
    if "b" in stages:
        if not np.array_equal(lv, after["node_levels"]):
            bad.append(tag("b node levels"))
        if case.north_star_reg_hierarchy and after["level_counts"] != np.bincount(lv, minlength=case.reg_levels).tolist():
            bad.append(tag("b level counts"))
        info["levels"] = np.bincount(lv).tolist() if len(lv) else []

    # ---- c
    T_dev = after["rigid_pose"]
    if "c" in stages and case.north_star_rigid_prealign:
        r = rigid(before, after, case)
        skipped = after["rigid_skipped"] - before["rigid_skipped"]
        if r["status"]:
            if not same(T_dev, K.IDENTITY) or skipped != 1:
                bad.append(tag("c a singular system leaves the identity and counts one skipped frame"))
        else:
            tol = pose_tolerance(r["e32"], r["pose64"])
            gap = float(np.abs(T_dev.astype(np.float64) - r["pose64"]).max())
            info["rigid"] = dict(e32=r["e32"], gap=gap, tol=tol, iters=r["iters_run"], matched=r["matched"])
            print(tag("c: e32 %.3e, |T_device - T_statement| %.3e, tol %.3e" % (r["e32"], gap, tol)))
            if gap > tol:
                bad.append(tag("c pose: gap %.3e > tol %.3e" % (gap, tol)))
            if skipped != 0:
                bad.append(tag("c skipped counter"))
            if case.rigid_prealign_device:
                if list(after["rigid_iters"]) != list(r["iters_run"]):
                    bad.append(tag("c iterations per level %s, statement %s" % (after["rigid_iters"], r["iters_run"])))
                if tuple(after["rigid_matched"]) != tuple(r["matched"]):
                    bad.append(tag("c matched %s, statement %s" % (after["rigid_matched"], r["matched"])))
    elif "c" in stages and not same(T_dev, K.IDENTITY):
        bad.append(tag("c the pose is not the identity with the switch off"))

    # ---- d: the start transforms, from the device's own T
    start = compose(before["node_dq"], T_dev, defect)

    # ---- e
    masked = bool(case.north_star_visible_only)
    if "e" in stages and masked:
        v = visibility(before, after, case, start, defect)
        px = v["knife"].size
        share = float(v["knife"].sum()) / px
        info["raster_knife"] = share
        if v["wrong_side"].any() or v["too_far"].any():
            bad.append(tag("e model map: %d pixels on the wrong side, %d too far" % (v["wrong_side"].sum(), v["too_far"].sum())))
        if share > AMBIGUOUS_CAP:
            bad.append(tag("e raster knife-edge share %.4f" % share))
        dev_flags = after["visible_flags"]
        if len(dev_flags) != len(v["flags"]):
            bad.append(tag("e flags: %d, cloud %d" % (len(dev_flags), len(v["flags"]))))
        else:
            dec = ~v["undecided"]
            info["flags_undecided"] = float(v["undecided"].mean())
            info["hidden"] = float((dev_flags == 0).mean())
            if not np.array_equal((dev_flags != 0)[dec], (v["flags"] != 0)[dec]):
                bad.append(tag("e flags: %d decided vertices differ" % ((dev_flags != 0)[dec] != (v["flags"] != 0)[dec]).sum()))
            if v["undecided"].mean() > AMBIGUOUS_CAP:
                bad.append(tag("e undecided flags share %.4f" % v["undecided"].mean()))
            if after["visible_count"] != int((dev_flags != 0).sum()):
                bad.append(tag("e count"))
    elif "e" in stages and (len(after["visible_flags"]) or after["visible_count"] != -1):
        bad.append(tag("e flags with the switch off"))

    # ---- f
    if "f" in stages:
        S = solve_start(before, after, case, start, after["visible_flags"] if masked else None, lv, defect)
        gap = abs(after["initial_cost"] - S.cost)
        info["cost"] = dict(device=after["initial_cost"], statement=S.cost, budget=S.cost_bud, amb=S.n_amb / S.N)
        print(tag("f: initial cost %.9g, statement %.9g, budget %.3g, ambiguous %d of %d" %
                  (after["initial_cost"], S.cost, S.cost_bud, S.n_amb, S.N)))
        if not gap <= S.cost_bud:
            bad.append(tag("f initial cost %.9g, statement %.9g, budget %.3g" % (after["initial_cost"], S.cost, S.cost_bud)))
        if S.n_amb / S.N > AMBIGUOUS_CAP:
            bad.append(tag("f knife-edge share %.4f" % (S.n_amb / S.N)))
        nrm, orth = unit_checks(after["node_dq"][:Db])
        if nrm > 4 * 2.0 ** -23 * 2 or orth > 4 * 2.0 ** -23 * 2:  # |r|^2 - 1 = 2 (|r| - 1)
            bad.append(tag("f transforms: | |r|^2 - 1 | %.3e, |r . d| %.3e" % (nrm, orth)))
        if not same(after["node_pos"][:Db], before["node_pos"]) or not same(after["node_w"][:Db], before["node_w"]):
            bad.append(tag("f / j old nodes' positions or weights changed"))

    # ---- g
    solved = after["node_dq"][:Db]
    if "g" in stages:
        pw, dp, nw, dn = warped(before, after, case, start if defect == "warped_by_start" else solved)
        if len(after["warped_v"]) != len(pw):
            bad.append(tag("g size"))
        else:
            ev = np.abs(after["warped_v"].astype(np.float64) - pw).max(1)
            fin = np.isfinite(nw).all(1)
            en = np.abs(after["warped_n"].astype(np.float64) - nw)[fin].max(1) if fin.any() else np.zeros(1)
            info["warped"] = dict(ratio=float((ev / dp).max()), nratio=float((en / dn[fin]).max()) if fin.any() else 0.0)
            if not (ev <= dp).all():
                bad.append(tag("g warped cloud: %d vertices beyond dp, worst ratio %.3g" % ((ev > dp).sum(), (ev / dp).max())))
            if fin.any() and not (en <= dn[fin]).all():
                bad.append(tag("g warped normals: worst ratio %.3g" % (en / dn[fin]).max()))

    # ---- h
    if "h" in stages and case.north_star_fuse_canonical:
        dq_fuse = start if defect == "fuse_start" else solved
        ref, cref = fusion(before, after, case, inputs, dq_fuse, defect)
        c = dict(name=tag("h"), vol=before["canonical_volume"], trunc=p.trunc, ref=ref, max_weight=p.tsdf_max_weight)
        info["fusion_undecided"] = float((~ref["decided"]).mean())
        _try(bad, tag("h canonical volume"), check, after["canonical_volume"], c)
        if (~ref["decided"]).mean() > AMBIGUOUS_CAP:
            bad.append(tag("h undecided share %.4f" % (~ref["decided"]).mean()))
        if cref is not None:
            cc = dict(name=tag("h colours"), cref=cref, image=cref["image"], max_color_weight=case.canonical_max_color_weight)
            _try(bad, tag("h colour volume"), check_colors, after["color_volume"], cref["colors"], before["color_volume"], cc)
            info["colour_undecided"] = float((~cref["decided"]).mean())
            if (~cref["decided"]).mean() > AMBIGUOUS_CAP:
                bad.append(tag("h undecided colour voxels: share %.4f" % (~cref["decided"]).mean()))
        if case.fuse_knn_field:
            want_nodes = after["D"] if defect == "field_after_growth" else Db
            if after["knn_field_nodes"] != want_nodes:
                bad.append(tag("h k-NN field holds %d nodes, not %d" % (after["knn_field_nodes"], want_nodes)))
    elif "h" in stages and len(after["canonical_volume"]):
        bad.append(tag("h a canonical volume with the switch off"))

    # ---- i
    if "i" in stages:
        if case.north_star_regrow_canonical:
            floor = case.canonical_min_weight - (1 if defect == "floor_minus_one" else 0)
            mv, mi, mn = welded_model(after["canonical_volume"], case, floor)
            if len(mv) == 0:
                if after["regrow_skipped"] != before["regrow_skipped"] + 1 or not same(after["canonical_v"], before["canonical_v"]):
                    bad.append(tag("i an empty extraction keeps the cloud and counts"))
            else:
                if not same(after["mesh_v"], mv) or not np.array_equal(after["mesh_i"], mi):
                    bad.append(tag("i mesh: %d vertices, statement %d" % (len(after["mesh_v"]), len(mv))))
                if not same(after["canonical_v"], mv[:, :3]):
                    bad.append(tag("i cloud"))
                if not _same_nan(after["canonical_n"], mn):
                    bad.append(tag("i normals"))
                if after["regrow_skipped"] != before["regrow_skipped"]:
                    bad.append(tag("i skipped counter"))
        else:
            for k in ("canonical_v", "canonical_n", "mesh_v", "mesh_i"):
                if not same(after[k], before[k]):
                    bad.append(tag("i %s changed without the switch" % k))
        if case.north_star_fuse_color:
            bad += _colors(after, case, tag, defect, info)

    # ---- j
    if "j" in stages:
        g = growth(before, after, case, defect)
        info["nodes"] = (Db, after["D"])
        info["growth_knife"] = g["knife"]
        if not same(after["node_pos"][:Db], before["node_pos"]) or not same(after["node_w"][:Db], before["node_w"]):
            bad.append(tag("j old nodes changed"))
        if g["knife"]:
            print(tag("j: a knife-edge vertex or seed: only the old nodes and the new weights are compared"))
            if not (after["node_w"][Db:] == g["weight"]).all():
                bad.append(tag("j new weights"))
        else:
            new_pos, new_dq = after["node_pos"][Db:], after["node_dq"][Db:]
            if not same(new_pos, g["seeds"]):
                bad.append(tag("j new positions: %d nodes, statement %d" % (len(new_pos), len(g["seeds"]))))
            else:
                if not (after["node_w"][Db:] == g["weight"]).all():
                    bad.append(tag("j new weights"))
                err = np.abs(new_dq.astype(np.float64) - g["dq"])
                if len(err) and not (err <= g["bar"]).all():
                    bad.append(tag("j new transforms: worst |dq - statement| %.3g (bar %.3g)" % (err.max(), g["bar"].max())))
    return bad


def _same_nan(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)))


def _colors(after, case, tag, defect, info):
    bad = []
    for name, verts in (("canonical_colors", after["canonical_v"]), ("mesh_colors", after["mesh_v"][:, :3])):
        if name == "mesh_colors" and not case.model_view:
            continue
        r = model_colors(after["color_volume"], case, verts, defect)
        got = after[name].view(np.uint8).reshape(-1, 4)
        if len(got) != len(verts):
            bad.append(tag("i %s: %d entries for %d vertices" % (name, len(got), len(verts))))
            continue
        dec = r["decided"]
        info[name + "_undecided"] = float((~dec).mean())
        if (~dec).mean() > AMBIGUOUS_CAP:
            bad.append(tag("i %s: undecided share %.4f" % (name, (~dec).mean())))
        err = np.abs(got[:, :3].astype(np.float64) - r["bgr"])
        info[name + "_err"] = float((err[dec] / r["bound"][dec, None]).max()) if dec.any() else 0.0
        if not np.array_equal(got[dec, 3], r["a"][dec]) or not np.all(err[dec] <= r["bound"][dec, None]):
            bad.append(tag("i %s: worst |byte - statement| %.3g over the bound %.3g" % (name, err[dec].max(), r["bound"].max())))
    return bad


def _first_frame(after, inputs, case, stages, tag, info):
    """frame 0: the canonical model and volume as frame 0 leaves them"""
    bad = []
    p = case.kinfu
    if "h" in stages and case.north_star_fuse_canonical:
        if not same(after["canonical_volume"], after["live_volume"]):
            bad.append(tag("h frame 0: the canonical volume is not the live volume"))
        if case.north_star_fuse_color:
            cref = first_colors(after, case, inputs)
            cc = dict(name=tag("h colours"), cref=cref, image=inputs["color"], max_color_weight=case.canonical_max_color_weight)
            _try(bad, tag("h frame 0 colour volume"), check_colors, after["color_volume"], cref["colors"],
                 np.zeros_like(after["color_volume"]), cc)
            if (~cref["decided"]).mean() > AMBIGUOUS_CAP:
                bad.append(tag("h frame 0 undecided colour voxels: share %.4f" % (~cref["decided"]).mean()))
        if case.fuse_knn_field and after["knn_field_nodes"] != after["D"]:
            bad.append(tag("h frame 0: the field holds %d of %d nodes" % (after["knn_field_nodes"], after["D"])))
    if "i" in stages:
        if case.north_star_regrow_canonical or case.model_view:
            mv, mi, mn = welded_model(after["live_volume"], case, 1)
            if case.model_view and (not same(after["mesh_v"], mv) or not np.array_equal(after["mesh_i"], mi)):
                bad.append(tag("i frame 0 mesh"))
            if case.north_star_regrow_canonical and (not same(after["canonical_v"], mv[:, :3]) or not _same_nan(after["canonical_n"], mn)):
                bad.append(tag("i frame 0 cloud"))
        if not case.north_star_regrow_canonical:
            cv, cn = soup_model(after["live_volume"], case)
            if not same(after["canonical_v"], cv) or not _same_nan(after["canonical_n"], cn):
                bad.append(tag("i frame 0 cloud: the marching-cubes soup with gradient normals, in the camera frame"))
        if case.north_star_fuse_color and case.north_star_regrow_canonical:
            bad += _colors(after, case, tag, None, info)
    if "j" in stages:
        seeds = after["canonical_v"][::case.nodeStep]
        info["nodes"] = (0, after["D"])
        if not same(after["node_pos"], seeds) or not (after["node_w"] == f32(3) * f32(case.epsilon)).all():
            bad.append(tag("j frame 0: the seeds are not every nodeStep-th vertex at weight 3 epsilon"))
        ident = np.zeros((after["D"], 8), np.float32)
        ident[:, 0] = 1
        if not same(after["node_dq"], ident):
            bad.append(tag("j frame 0: a seed's transform is not the identity"))
        if not same(after["warped_v"], after["canonical_v"]):
            bad.append(tag("g frame 0: the warped cloud is not the canonical cloud"))
    return bad


# ------------------------------------------------------------------------------------------------------ the chain ----
def _bytes(r):
    """color_sample_statement.sample's dict as the kernel's b, g, r, a bytes (channels rounded to nearest)"""
    out = np.zeros((len(r["a"]), 4), np.uint8)
    out[:, :3] = np.rint(r["bgr"]).astype(np.uint8)
    out[:, 3] = r["a"]
    return out.view(np.uint32).reshape(-1)


def expect_visibility(before, case, start):
    """stage e forwards: the rasterised start-warped mesh and the flags of the start-warped cloud"""
    p = case.kinfu
    gm = graph(before["node_pos"], before["node_w"], before["mesh_v"][:, :3], case.k)
    mv = blend(start, gm, before["mesh_v"][:, :3], None, np.float32)
    mesh = np.concatenate([mv, np.ones((len(mv), 1), np.float32)], 1)
    _, points, normals = RA.rasterize32(mesh, None, before["mesh_i"], None, *p.intr, Z_NEAR, p.cols, p.rows)
    gc = graph(before["node_pos"], before["node_w"], before["canonical_v"], case.k)
    cloud = blend(start, gc, before["canonical_v"], None, np.float32)
    flags, count = VS.visible_vertices(cloud, points, *p.intr, f32(2) * p.voxel_size.max())
    return points, normals, flags, count


def chain_records(case, depths, colors, solved_of):
    """The statement chain over a case's frames, no device and no solve: solved_of(i) gives the rigid motion (12 numbers) every
    node that exists before frame i holds after it.  -> the records, as northstar_cases.read_records gives them"""
    p = case.kinfu
    e = lambda *shape, dtype=np.float32: np.zeros(shape, dtype)
    recs = []
    for i, depth in enumerate(depths):
        before = recs[-1] if recs else None
        m = measured(depth, case, before is None)
        r = dict(result=before is not None, counter=i + 1, rigid_pose=K.IDENTITY.copy(), rigid_iters=[], rigid_matched=(0, 0),
                 rigid_skipped=0, regrow_skipped=0, visible_flags=e(0, dtype=np.uint8), visible_count=-1, node_levels=e(0, dtype=np.int32),
                 level_counts=[], initial_cost=0.0, model_points=e(0), model_normals=e(0), live_points=e(0), live_normals=e(0),
                 canonical_volume=e(0, dtype=np.uint32), color_volume=e(0, dtype=np.uint32), canonical_colors=e(0, dtype=np.uint32),
                 mesh_colors=e(0, dtype=np.uint32), mesh_v=e(0, 4), mesh_i=e(0, dtype=np.int32), knn_field_nodes=-1, knn=case.k)
        r.update(m)
        if before is None:
            if case.north_star_regrow_canonical or case.model_view:
                mv, mi, mn = welded_model(r["live_volume"], case, 1)
                if case.model_view:
                    r["mesh_v"], r["mesh_i"] = mv, mi
            if case.north_star_regrow_canonical:
                r["canonical_v"], r["canonical_n"] = mv[:, :3].copy(), mn
            else:
                r["canonical_v"], r["canonical_n"] = soup_model(r["live_volume"], case)
            r["node_pos"] = r["canonical_v"][::case.nodeStep].copy()
            r["D"] = len(r["node_pos"])
            r["node_w"] = np.full(r["D"], f32(3) * f32(case.epsilon), np.float32)
            r["node_dq"] = np.zeros((r["D"], 8), np.float32)
            r["node_dq"][:, 0] = 1
            r["warped_v"], r["warped_n"] = r["canonical_v"], r["canonical_n"]
            if case.north_star_fuse_canonical:
                r["canonical_volume"] = r["live_volume"].copy()
                r["knn_field_nodes"] = r["D"] if case.fuse_knn_field else 0
            if case.north_star_fuse_color:
                r["color_volume"] = first_colors(r, case, dict(color=colors[i]))["colors"]
        else:
            Db = before["D"]
            r["rigid_skipped"], r["regrow_skipped"] = before["rigid_skipped"], before["regrow_skipped"]
            lv = levels(before, case)
            r["node_levels"] = lv
            r["level_counts"] = np.bincount(lv, minlength=case.reg_levels).tolist() if case.north_star_reg_hierarchy else []
            if case.north_star_rigid_prealign:
                rg = rigid(before, r, case)
                if rg["status"]:
                    r["rigid_skipped"] += 1
                else:
                    r["rigid_pose"] = rg["pose32"]
                r["rigid_iters"] = rg["iters_run"] if case.rigid_prealign_device else []
                r["rigid_matched"] = rg["matched"]
            start = compose(before["node_dq"], r["rigid_pose"])
            if case.north_star_visible_only:
                r["model_points"], r["model_normals"], r["visible_flags"], r["visible_count"] = expect_visibility(before, case, start)
            S = solve_start(before, r, case, start, r["visible_flags"] if case.north_star_visible_only else None, lv)
            r["initial_cost"] = S.cost
            motion = solved_of(i)
            ident = np.zeros((Db, 8))
            ident[:, 0] = 1
            solved = start if motion is None else RS.compose_rigid(ident, motion).astype(np.float32)
            pw, _, nw, _ = warped(before, r, case, solved)
            r["warped_v"], r["warped_n"] = pw.astype(np.float32), nw.astype(np.float32)
            r["node_pos"], r["node_w"], r["node_dq"], r["D"] = before["node_pos"], before["node_w"], solved, Db
            for k in ("canonical_v", "canonical_n", "mesh_v", "mesh_i", "canonical_volume", "color_volume"):
                r[k] = before[k]
            if case.north_star_fuse_canonical:
                ref, cref = fusion(before, r, case, dict(color=colors[i]), solved)
                r["canonical_volume"] = ref["vol"]
                r["knn_field_nodes"] = Db if case.fuse_knn_field else 0
                if cref is not None:
                    r["color_volume"] = cref["colors"]
            if case.north_star_regrow_canonical:
                mv, mi, mn = welded_model(r["canonical_volume"], case, case.canonical_min_weight)
                if len(mv):
                    r["canonical_v"], r["canonical_n"] = mv[:, :3].copy(), mn
                    if case.model_view:
                        r["mesh_v"], r["mesh_i"] = mv, mi
                else:
                    r["regrow_skipped"] += 1
            g = growth(before, r, case)
            assert not g["knife"], "the chain's field growth hangs on a knife edge"
            n = len(g["seeds"])
            r["node_pos"] = np.concatenate([before["node_pos"], g["seeds"]]).astype(np.float32)
            r["node_w"] = np.concatenate([before["node_w"], np.full(n, g["weight"], np.float32)])
            r["node_dq"] = np.concatenate([solved, g["dq"].astype(np.float32).reshape(n, 8)])
            r["D"] = Db + n
        if case.north_star_fuse_color:
            r["canonical_colors"] = _bytes(model_colors(r["color_volume"], case, r["canonical_v"]))
            if case.model_view:
                r["mesh_colors"] = _bytes(model_colors(r["color_volume"], case, r["mesh_v"][:, :3]))
        r["canonical_vertices"] = len(r["canonical_v"])
        recs.append(r)
    return recs
