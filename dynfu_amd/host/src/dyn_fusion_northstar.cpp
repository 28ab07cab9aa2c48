// dyn_fusion_northstar.cpp — DynFusion's frame in north-star mode (DynFuParams::north_star): the frame
// function and its stages, one per switch, in the order they run.
#include <dynfu/dyn_fusion.hpp>

#include <algorithm>
#include <cmath>

#include <dfa_host/device.hpp>

#include "../../../include/dynfu_amd.h"
#include "stage_clock.hpp"

// The same frame sequence with the north-star solve in the middle: the live side of the solve is the depth frame itself
// (vertex / normal maps of the filtered depth, as KinFu builds them for its tracker, kinfu.cpp:150-175), so neither the
// live marching-cubes cloud nor the nearest-neighbour correspondence is on the path; everything the solve sees is in
// the camera frame.
bool DynFusion::northStarFrame(const kfusion::cuda::Depth& depth) {
    if (frame_counter_ == 0) return northStarFirstFrame();
    const kfusion::KinFuParams& p = params_;
    const dfa::Affine3f camera;  // the camera stays at the origin, as in the reference's operator() (:100-105)
    dfa::StageClock clk;
    tsdf().clearAndIntegrate(dists_, camera, p.intr);
    addLiveFrame(frame_counter_, extractSurface(frame_counter_, dynfuParams.mesh_normals));  // for getLiveFrame() / getMesh()
    clk.mark("pre-process + fuse + marching cubes");
    NorthStarSolver solver(*warpfield, dynfuParams.northStarParams, dynfuParams.tukeyOffset, dynfuParams.psi_data,
                           dynfuParams.lambda, dynfuParams.psi_reg);
    buildNorthStarProblem(solver, clk);
    const bool prealigned = prealignRigid(solver, clk);
    maskHiddenVertices(solver, clk);
    if (!prealigned) kfusion::cuda::computePointNormals(p.intr, curr_.depth_pyr[0], live_points_, live_normals_);
    solveNorthStar(solver, clk);
    fuseThroughSolvedField(clk);
    canonicalFrameWarpedToLive = solver.warpCanonicalToLive();  // the cloud the solve used
    growModelAndField(clk);
    return ++frame_counter_, true;
}

void DynFusion::volumeToCamera(float aff[12]) {
    const dfa::Affine3f camera;
    (camera.inv() * tsdf().getPose()).to12(aff);
}

// Frame 0: the fused volume's surface, in the camera frame, is the canonical cloud; the nodes are seeded on it
bool DynFusion::northStarFirstFrame() {
    tsdf().integrate(dists_, dfa::Affine3f(), params_.intr);
    float aff[12];
    volumeToCamera(aff);
    if (dynfuParams.north_star_regrow_canonical) {
        // the canonical cloud is the WELDED vertex set (frame 0 holds weight 1 only: no floor), and with model_view the
        // kept mesh is the cloud's mesh; every later frame replaces both from the canonical volume
        kfusion::cuda::MarchingCubes::IndexedMesh mesh;
        auto welded = extractWeldedModel(tsdf(), 1, aff, mesh);
        if (!welded) throw dfa::Error(DFA_ERR_INVALID, "DynFusion (north-star mode): the first frame has no surface");
        initFromFrame(welded);
        if (dynfuParams.model_view) setCanonicalMesh(welded, mesh);
        createCanonicalVolume();
        fuseFirstFrameColors();
        sampleModelColors();
        return ++frame_counter_, false;
    }
    auto vol_frame = extractSurface(0, true);  // volume frame, normals from the TSDF gradient
    const size_t n = vol_frame->size();
    if (n == 0) throw dfa::Error(DFA_ERR_INVALID, "DynFusion (north-star mode): the first frame has no surface");
    const dynfu::Frame::DeviceView v = vol_frame->device();
    dfa::DeviceArray<float> cv(3 * n), cn(3 * n);
    dfa::check(dfa_transform_points(v.vertices, (int)n, aff, 1, cv.ptr(), nullptr), "DynFusion: canonical vertices to the camera frame");
    dfa::check(dfa_transform_points(v.normals, (int)n, aff, 0, cn.ptr(), nullptr), "DynFusion: canonical normals to the camera frame");
    initFromFrame(dynfu::Frame::fromDevice(0, cv, cn, n));
    if (dynfuParams.model_view) keepCanonicalMesh(aff);
    if (dynfuParams.north_star_fuse_canonical) createCanonicalVolume();
    fuseFirstFrameColors();
    return ++frame_counter_, false;
}

// The graphs of the frame over the canonical cloud; north_star_reg_hierarchy: multi-level, and the levels' report
void DynFusion::buildNorthStarProblem(NorthStarSolver& solver, dfa::StageClock& clk) {
    const bool hierarchy = dynfuParams.north_star_reg_hierarchy;
    const int levels     = dynfuParams.regLevels();
    if (hierarchy)
        solver.setRegHierarchy(std::vector<int>(dynfuParams.reg_level_slots.begin(), dynfuParams.reg_level_slots.begin() + levels),
                               dynfuParams.epsilon, dynfuParams.beta);
    solver.initializeProblemInstance(canonicalFrame);
    if (hierarchy) {
        report_.reg_node_levels = solver.nodeLevels();
        report_.reg_level_counts.assign((size_t)levels, 0);
        for (int lv : report_.reg_node_levels) ++report_.reg_level_counts[(size_t)lv];
    }
    clk.mark("  initializeProblemInstance");
}

// north_star_rigid_prealign — the global rigid motion first: the start transforms and the shared nodes come out composed with
// it, so everything after it — the model view, the visibility test, the solve, the fusion — sees the aligned field
bool DynFusion::prealignRigid(NorthStarSolver& solver, dfa::StageClock& clk) {
    const DynFuParams& d = dynfuParams;
    if (!d.north_star_rigid_prealign || !(d.rigid_prealign_device || d.rigid_prealign_iters > 0)) return false;
    const kfusion::KinFuParams& p = params_;
    kfusion::cuda::computePointNormals(p.intr, curr_.depth_pyr[0], live_points_, live_normals_);
    bool aligned;
    if (d.rigid_prealign_device) {
        NorthStarSolver::RigidSchedule schedule;
        schedule.steps = d.rigid_prealign_steps, schedule.iters = d.rigid_prealign_level_iters;
        schedule.stopRot = d.rigid_prealign_stop_rot, schedule.stopTrans = d.rigid_prealign_stop_trans;
        aligned                 = solver.alignRigid(live_points_, live_normals_, p.intr, schedule, report_.rigid_pose);
        report_.rigid_iters_run = solver.rigidIterationsRun();
    } else {
        aligned = solver.alignRigid(live_points_, live_normals_, p.intr, d.rigid_prealign_iters, report_.rigid_pose);
    }
    if (!aligned) ++report_.rigid_skipped;
    report_.rigid_matched_first = solver.rigidMatchedFirst(), report_.rigid_matched_last = solver.rigidMatchedLast();
    clk.mark("  alignRigid");
    return true;
}

// north_star_visible_only — the model as the solve finds it: mesh and cloud warped by the transforms the solve starts from,
// the mesh rasterised from this frame's camera; a vertex behind the rasterised surface takes no data row
void DynFusion::maskHiddenVertices(NorthStarSolver& solver, dfa::StageClock& clk) {
    if (!dynfuParams.north_star_visible_only) return;
    rasterizeWarpedModel();
    const dfa::DeviceArray<float> start = solver.warpCanonicalByStart();
    float z_tol = dynfuParams.visibility_z_tol;
    if (z_tol == 0.f) {
        const kfusion::Vec3f vs = tsdf().getVoxelSize();
        z_tol = 2.f * std::max(vs[0], std::max(vs[1], vs[2]));
    }
    kfusion::cuda::visibleVertices(start.ptr(), 3, canonicalFrame->size(), model_points_, params_.intr, z_tol, visible_flags_,
                                   &report_.visible_count);
    solver.setVertexMask(visible_flags_);
    report_.visible_counted = true;
    clk.mark("  visible vertices");
}

void DynFusion::solveNorthStar(NorthStarSolver& solver, dfa::StageClock& clk) {
    solver.solveAll(live_points_, live_normals_, params_.intr);
    clk.mark("  solveAll");
    report_.initial_cost = solver.initialCost(), report_.final_cost = solver.finalCost(), report_.valid_rows = solver.validRows();
    report_.pcg_iters = solver.pcgIterations(), report_.gn_solves = solver.gnSolves();
}

// north_star_fuse_canonical — this frame's depth into the canonical volume through the solved field: the nodes hold the solved
// transforms now, and the field has not grown yet.  The node frame is frame 0's camera — `camera`: it stays at the origin
void DynFusion::fuseThroughSolvedField(dfa::StageClock& clk) {
    if (!dynfuParams.north_star_fuse_canonical) return;
    const dfa::Affine3f camera;
    if (dynfuParams.fuse_knn_field) syncKnnField();
    const Warpfield::DeviceNodeView nodes = warpfield->deviceNodes();
    if (dynfuParams.north_star_fuse_color) {  // the one fused call: the same voxels, and the frame's colours
        canonical_volume_->integrateWarped6Color(dists_, *frame_color_, camera, params_.intr, camera, nodes.pos, nodes.dq, nodes.w, nodes.D,
                                                 northStarKnn(warpfield->getKnn()), unsupportedMode(), true,
                                                 dynfuParams.canonical_max_color_weight);
        model_colors_current_ = false;
        clk.mark("integrateWarped6Color");
        return;
    }
    canonical_volume_->integrateWarped6(dists_, camera, params_.intr, camera, nodes.pos, nodes.dq, nodes.w, nodes.D,
                                        northStarKnn(warpfield->getKnn()), unsupportedMode());
    clk.mark("integrateWarped6");
}

// north_star_fuse_color, frame 0 — the canonical volume is a copy of the live one: only its colours are missing.  One
// colours-only call with no nodes, every voxel where it stands (Rigid): what integrate() saw of each voxel, its texel's colour
void DynFusion::fuseFirstFrameColors() {
    if (!dynfuParams.north_star_fuse_color) return;
    const dfa::Affine3f camera;
    canonical_volume_->createColors();
    canonical_volume_->integrateWarped6Color(dists_, *frame_color_, camera, params_.intr, camera, nullptr, nullptr, nullptr, 0,
                                             northStarKnn(warpfield->getKnn()), kfusion::cuda::TsdfVolume::UnsupportedMode::Rigid, false,
                                             dynfuParams.canonical_max_color_weight);
    model_colors_current_ = false;
}

// north_star_fuse_color — the colours of the canonical cloud (camera frame of frame 0: the origin) and, with model_view, of
// the kept mesh's vertices, from the canonical volume's colours as they are now.  Both are marching-cubes vertices: half a voxel
// off the lattice the colours were fused on (TsdfVolume::sampleColors: lattice_offset)
void DynFusion::sampleModelColors() {
    if (!dynfuParams.north_star_fuse_color) return;
    const dfa::Affine3f camera;
    const dynfu::Frame::DeviceView v = canonicalFrame->device();
    cloud_colors_ = canonical_volume_->sampleColors(v.vertices, (int)canonicalFrame->size(), 3, camera, 0.5f);
    mesh_colors_  = dfa::DeviceArray<kfusion::RGB>();
    if (dynfuParams.model_view && canonical_mesh_.vertices.size() > 0)
        mesh_colors_ = canonical_volume_->sampleColors((const float*)canonical_mesh_.vertices.ptr(), (int)canonical_mesh_.vertices.size(), 4, camera, 0.5f);
    model_colors_current_ = true;
}

dfa::DeviceArray<kfusion::RGB> DynFusion::canonicalColors() {
    if (!dynfuParams.north_star_fuse_color || !canonical_volume_)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion::canonicalColors: north_star_fuse_color is off, or no frame has run");
    if (!model_colors_current_) sampleModelColors();
    return cloud_colors_;
}

dfa::DeviceArray<kfusion::RGB> DynFusion::canonicalMeshColors() {
    if (!dynfuParams.north_star_fuse_color || !canonical_volume_ || !dynfuParams.model_view)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion::canonicalMeshColors: north_star_fuse_color or model_view is off, or no frame has run");
    if (!model_colors_current_) sampleModelColors();
    return mesh_colors_;
}

// The field grows where the warped cloud has no support.  north_star_regrow_canonical — the canonical model grows first: the
// cloud (and the kept mesh) of the next frame is the canonical volume's surface as it is now, from the voxels seen
// canonical_min_weight times, and the field is extended where THAT cloud — in canonical space — has no support.  An empty
// extraction keeps the old model.
void DynFusion::growModelAndField(dfa::StageClock& clk) {
    if (!dynfuParams.north_star_regrow_canonical) {
        warpfield->update(canonicalFrameWarpedToLive);
        clk.mark("warp + warpfield->update");
        return;
    }
    float aff[12];
    volumeToCamera(aff);
    kfusion::cuda::MarchingCubes::IndexedMesh mesh;
    if (auto grown = extractWeldedModel(*canonical_volume_, dynfuParams.canonical_min_weight, aff, mesh)) {
        canonicalFrame = grown;
        if (dynfuParams.model_view) setCanonicalMesh(grown, mesh);
    } else {
        ++report_.regrow_skipped;
    }
    sampleModelColors();  // north_star_fuse_color: the colours of the model as it is now
    clk.mark("warp + regrow");
    const size_t nodes_before = warpfield->nodesRef().size();
    warpfield->update(canonicalFrame);
    startNewNodesFromBlend(nodes_before);
    clk.mark("warpfield->update");
}

// north_star_regrow_canonical: the transforms the nodes Warpfield::update has just appended start from.  update gives a new
// node calcDQB of the field before it — the reference's blend, a PRODUCT of the k neighbours' weighted transforms, which
// composes them: harmless for the translations of a few millimetres it was written for and for seeds at the edge of the
// support, but a seed of the regrown cloud may lie half a model away from the nearest node, and the north-star nodes hold
// whole rigid transforms: k of them composed threw the new part of the model a metre off on the half-sphere sequence of
// tests/cpp/test_host_regrow.cpp.  Here a new node takes what the north-star blend (csrc/blend6_device.hpp) gives a point
// at its position from the nodes that existed before: the k nearest, radial basis weights normalised, every transform in the
// hemisphere of the nearest, real and dual parts summed and divided by the real part's norm.  Host arithmetic in double over
// the handful of new nodes; the weights are taken relative to the nearest node's, so that no distance underflows them all.
void DynFusion::startNewNodesFromBlend(size_t nodes_before) {
    const auto& nodes = warpfield->nodesRef();
    if (nodes_before == 0 || nodes.size() <= nodes_before) return;
    std::vector<float> pos, w, dq;
    warpfield->hostArrays(pos, w, dq);
    const int k = (int)std::min<size_t>((size_t)northStarKnn(warpfield->getKnn()), nodes_before);
    std::vector<std::pair<double, size_t>> near(nodes_before);
    for (size_t i = nodes_before; i < nodes.size(); ++i) {
        for (size_t j = 0; j < nodes_before; ++j) {
            const double dx = (double)pos[3 * i] - pos[3 * j], dy = (double)pos[3 * i + 1] - pos[3 * j + 1],
                         dz = (double)pos[3 * i + 2] - pos[3 * j + 2];
            near[j] = {dx * dx + dy * dy + dz * dz, j};
        }
        std::partial_sort(near.begin(), near.begin() + k, near.end());  // ascending distance, ties to the lower index
        double e[8], e_max = -1e300, a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
        for (int q = 0; q < k; ++q) {
            const double r = (double)w[near[q].second];
            e[q] = -near[q].first / (2 * r * r), e_max = std::max(e_max, e[q]);
        }
        const float* first = &dq[8 * near[0].second];
        for (int q = 0; q < k; ++q) {
            const float* t = &dq[8 * near[q].second];
            const double dot = (double)t[0] * first[0] + (double)t[1] * first[1] + (double)t[2] * first[2] + (double)t[3] * first[3];
            const double wt = std::exp(e[q] - e_max) * (dot < 0 ? -1.0 : 1.0);
            for (int c = 0; c < 4; ++c) a[c] += wt * t[c], b[c] += wt * t[4 + c];
        }
        const double norm = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
        if (!(norm > 0)) continue;  // (opposite rotations cancelling exactly: the node keeps update's transform)
        nodes[i]->setTransformation(std::make_shared<DualQuaternion<float>>(
            dfa::quaternion<float>((float)(a[0] / norm), (float)(a[1] / norm), (float)(a[2] / norm), (float)(a[3] / norm)),
            dfa::quaternion<float>((float)(b[0] / norm), (float)(b[1] / norm), (float)(b[2] / norm), (float)(b[3] / norm))));
    }
}
