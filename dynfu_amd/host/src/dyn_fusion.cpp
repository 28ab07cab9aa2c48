// dyn_fusion.cpp — DynFusion's warp-field sequence on the dynfu_amd C ABI
// (reference: src/dynfu/dyn_fusion.cpp:6-31,147-242).
#include <dynfu/dyn_fusion.hpp>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <filesystem>

#include <dfa_host/device.hpp>

#include "../../../include/dynfu_amd.h"

kfusion::KinFuParams kfusion::KinFuParams::default_params() {  // src/kfusion/kinfu.cpp:10-44
    KinFuParams p;
    p.cols = 640, p.rows = 480;
    p.intr        = Intr(525.f, 525.f, p.cols / 2 - 0.5f, p.rows / 2 - 0.5f);
    p.volume_dims = Vec3i::all(512);
    p.volume_size = Vec3f::all(3.f);
    p.volume_pose = Affine3f().translate(Vec3f(-p.volume_size[0] / 2, -p.volume_size[1] / 2, 0.5f));
    p.bilateral_sigma_depth = 0.04f, p.bilateral_sigma_spatial = 4.5f, p.bilateral_kernel_size = 7;
    p.icp_truncate_depth_dist = 0.f;
    p.icp_dist_thres = 0.1f, p.icp_angle_thres = 30.f * 0.017453293f, p.icp_iter_num = {10, 5, 4, 0};
    p.tsdf_min_camera_movement = 0.f;
    p.tsdf_trunc_dist = 0.04f, p.tsdf_max_weight = 64;
    p.raycast_step_factor = 0.75f, p.gradient_delta_factor = 0.5f;
    p.light_pose = Vec3f::all(0.f);  // :41
    return p;
}

DynFuParams DynFuParams::defaultParams() {  // dyn_fusion.cpp:6-31
    DynFuParams p;
    p.kinfuParams             = kfusion::KinFuParams::default_params();
    p.kinfuParams.volume_dims = kfusion::Vec3i::all(128);  // :10
    p.intr        = p.kinfuParams.intr;
    p.tukeyOffset = 4.652f;
    p.lambda      = 200.f;
    p.psi_data    = 0.01f;
    p.psi_reg     = 1e-4f;
    p.L           = 4;
    p.beta        = 4;
    p.epsilon     = 0.1f;
    return p;
}

DynFusion::DynFusion(const DynFuParams& params) : kfusion::KinFu(params.kinfuParams), dynfuParams(params) {  // dyn_fusion.cpp:33
    if (params.fuse_canonical && params.north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: fuse_canonical is a reference-mode extension (north_star blends otherwise, in the camera frame: north_star_fuse_canonical)");
    if (params.north_star_fuse_canonical && !params.north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_fuse_canonical needs north_star (reference mode: fuse_canonical)");
    if (params.fuse_knn_field && !params.fuse_canonical && !params.north_star_fuse_canonical)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: fuse_knn_field serves the canonical fusion (fuse_canonical or north_star_fuse_canonical)");
    if (params.north_star_visible_only && !(params.north_star && params.model_view))
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_visible_only needs north_star and model_view (the rasterised canonical mesh is what hides a vertex)");
    if (params.fuse_unsupported_rigid && !params.fuse_canonical && !params.north_star_fuse_canonical)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: fuse_unsupported_rigid serves the canonical fusion (fuse_canonical or north_star_fuse_canonical)");
    if (params.north_star_regrow_canonical && !params.north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_regrow_canonical needs north_star (reference mode keeps frame 0's cloud)");
    if (params.north_star_regrow_canonical && !params.north_star_fuse_canonical)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_regrow_canonical needs north_star_fuse_canonical (the canonical volume is what the cloud is re-extracted from)");
    if (params.north_star_regrow_canonical && (params.canonical_min_weight < 1 || params.canonical_min_weight > 65535))
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: canonical_min_weight outside 1..65535");
    if (params.north_star_rigid_prealign && !params.north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_rigid_prealign needs north_star (reference mode has no rigid step: KinFu tracks rigidly)");
    if (params.north_star_rigid_prealign && params.rigid_prealign_iters < 0)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: negative rigid_prealign_iters");
    if (params.rigid_prealign_device) {
        if (!params.north_star_rigid_prealign)
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: rigid_prealign_device needs north_star_rigid_prealign (it is that step's loop, on the device)");
        const std::vector<int>&st = params.rigid_prealign_steps, &it = params.rigid_prealign_level_iters;
        long total = 0;
        for (int n : it) total += n;
        bool ok = !st.empty() && st.size() <= 4 && st.size() == it.size() && total <= 64;
        for (int v : st) ok = ok && v >= 1;
        for (int n : it) ok = ok && n >= 0;
        if (!ok)
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: rigid_prealign_steps / rigid_prealign_level_iters: 1 to 4 levels, steps >= 1, iterations >= 0 and at most 64 in all");
        if (!(params.rigid_prealign_stop_rot >= 0.f) || !(params.rigid_prealign_stop_trans >= 0.f))
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: negative or NaN rigid_prealign_stop_rot / rigid_prealign_stop_trans");
    }
    if (params.north_star_reg_hierarchy) {
        if (!params.north_star)
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_reg_hierarchy needs north_star (the reference-mode solve keeps its flat graph)");
        const int levels = regLevels();
        long sum         = 0;
        bool ok = levels >= 1 && levels <= 8 && params.reg_level_slots[0] >= 1 && params.beta >= 2 && params.epsilon > 0.f;
        for (int l = 0; l < levels; ++l) ok = ok && params.reg_level_slots[l] >= 0, sum += params.reg_level_slots[l];
        if (!ok || sum > std::min(KNN, 8))  // (the field is created with KNN neighbours; a k set later is checked by the frame)
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_reg_hierarchy: 1 to 8 levels (min(L + 1, reg_level_slots.size())), reg_level_slots[0] >= 1, no negative slot, a slot sum of at most the warp field's k (and 8), beta >= 2, epsilon > 0");
    }
    solverParams.numIter       = 24;  // dyn_fusion.cpp:183-189
    solverParams.nonLinearIter = 16;
    solverParams.linearIter    = 256;
    solverParams.useOpt        = true;
    solverParams.useOptLM      = false;
    solverParams.earlyOut      = true;
}
DynFusion::~DynFusion() = default;

DynFuParams& DynFusion::params() { return dynfuParams; }

int DynFusion::regLevels() const {
    return (int)std::min<size_t>((size_t)std::max(dynfuParams.L + 1, 0), dynfuParams.reg_level_slots.size());
}

kfusion::cuda::TsdfVolume::UnsupportedMode DynFusion::unsupportedMode() const {
    return dynfuParams.fuse_unsupported_rigid ? kfusion::cuda::TsdfVolume::UnsupportedMode::Rigid
                                              : kfusion::cuda::TsdfVolume::UnsupportedMode::Skip;
}

void DynFusion::init(dfa::PointCloud<dfa::PointXYZ>& canonicalVertices, dfa::PointCloud<dfa::Normal>& canonicalNormals) {
    initCanonicalFrame(canonicalVertices, canonicalNormals);
    seedNodes(canonicalVertices.points);
}

// :147-168 — a node at every nodeStep-th canonical vertex
void DynFusion::seedNodes(const std::vector<dfa::PointXYZ>& canonicalVertices) {
    std::vector<std::shared_ptr<Node>> seeds;
    const float dg_w = 3 * dynfuParams.epsilon;  // :158
    for (size_t i = 0; i < canonicalVertices.size(); i += (size_t)nodeStep)
        seeds.push_back(std::make_shared<Node>(
            canonicalVertices[i], std::make_shared<DualQuaternion<float>>(0.f, 0.f, 0.f, 0.f, 0.f, 0.f), dg_w));
    warpfield = std::make_shared<Warpfield>();
    warpfield->init(dynfuParams.epsilon, seeds);
}

void DynFusion::initCanonicalFrame(dfa::PointCloud<dfa::PointXYZ>& vertices, dfa::PointCloud<dfa::Normal>& normals) {
    canonicalFrame             = std::make_shared<dynfu::Frame>(0, vertices, normals);
    canonicalFrameWarpedToLive = std::make_shared<dynfu::Frame>(0, vertices, normals);
}

// frame 0 of operator(): the canonical frame is the device-resident marching-cubes cloud; only the seeding reads it
// on the host (once, through the const accessor: the device arrays stay the master)
void DynFusion::initFromFrame(std::shared_ptr<dynfu::Frame> frame) {
    dfa::DeviceArray<float> v3, n3;
    frame->deviceArrays(v3, n3);
    canonicalFrame             = frame;
    canonicalFrameWarpedToLive = dynfu::Frame::fromDevice(0, v3, n3, frame->size());  // a second Frame, as :171-175
    seedNodes(frame->vertices().points);
}

void DynFusion::addLiveFrame(int frameID, std::shared_ptr<dynfu::Frame> frame) {
    (void)frameID;
    liveFrame = frame;
}

void DynFusion::addLiveFrame(int frameID, dfa::PointCloud<dfa::PointXYZ>& vertices,
                             dfa::PointCloud<dfa::Normal>& normals) {
    liveFrame = std::make_shared<dynfu::Frame>(frameID, vertices, normals);
}

namespace {
// DFA_HOST_PROFILE=1: wall time of the stages of a frame (device synchronised at every mark) on stderr
struct StageClock {
    bool on = dfa::host_switch("DFA_HOST_PROFILE");
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char* what) {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[dfa host] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};
}  // namespace

void DynFusion::warpCanonicalToLiveOpt(dfa::Affine3f affine) {
    if (!warpfield || !canonicalFrame || !liveFrame)
        throw dfa::Error(DFA_ERR_INVALID, "warpCanonicalToLiveOpt before init / addLiveFrame");
    StageClock clk;
    CombinedSolver combinedSolver(*warpfield, solverParams, dynfuParams.tukeyOffset, dynfuParams.psi_data,
                                  dynfuParams.lambda, dynfuParams.psi_reg);
    clk.mark("  CombinedSolver ctor");
    canonicalFrameWarpedToLive = warpfield->warpToLive(canonicalFrame);  // :196
    clk.mark("  warpToLive");
    auto corresponding         = findCorrespondingFrame(canonicalFrameWarpedToLive, liveFrame);
    clk.mark("  findCorrespondingFrame");
    combinedSolver.initializeProblemInstance(corresponding, liveFrame, affine);  // :206
    clk.mark("  initializeProblemInstance");
    combinedSolver.solveAll();                                                   // :207
    clk.mark("  solveAll");
}

std::shared_ptr<dynfu::Frame> DynFusion::findCorrespondingFrame(dfa::PointCloud<dfa::PointXYZ> canonicalVertices,
                                                                dfa::PointCloud<dfa::Normal> canonicalNormals,
                                                                dfa::PointCloud<dfa::PointXYZ> liveVertices) {
    return findCorrespondingFrame(std::make_shared<dynfu::Frame>(0, std::move(canonicalVertices), std::move(canonicalNormals)),
                                  std::make_shared<dynfu::Frame>(0, std::move(liveVertices), dfa::PointCloud<dfa::Normal>()));
}

// :212-242 on frames: both clouds are read where they are (HBM for the adaptor's own frames), the result stays there
std::shared_ptr<dynfu::Frame> DynFusion::findCorrespondingFrame(std::shared_ptr<dynfu::Frame> canonical,
                                                                std::shared_ptr<dynfu::Frame> live) {
    const size_t nc = canonical->size(), nl = live->size();
    if (nl == 0) return std::make_shared<dynfu::Frame>(0, dfa::PointCloud<dfa::PointXYZ>(), dfa::PointCloud<dfa::Normal>());
    if (nc == 0) throw dfa::Error(DFA_ERR_INVALID, "findCorrespondingFrame: empty canonical cloud");
    const dynfu::Frame::DeviceView c = canonical->device(), l = live->device();
    dfa::DeviceArray<float> dov(3 * nl), don(3 * nl);
    dfa::check(dfa_correspond(c.vertices, c.normals, (int)nc, l.vertices, (int)nl, dov.ptr(), don.ptr(), nullptr, nullptr),
               "DynFusion::findCorrespondingFrame");
    return dynfu::Frame::fromDevice(0, dov, don, nl);
}

std::shared_ptr<dynfu::Frame> DynFusion::getCanonicalWarpedToLive() { return canonicalFrameWarpedToLive; }

void DynFusion::fuse(const kfusion::cuda::Depth& depth, kfusion::cuda::TsdfVolume& volume,
                     const dfa::Affine3f& camera_pose) {
    kfusion::cuda::computeDists(depth, dists_, dynfuParams.intr);       // :58
    volume.clearAndIntegrate(dists_, camera_pose, dynfuParams.intr);   // :113-114
}

// ------------------------------------------------------------------------- the per-frame sequence

std::shared_ptr<dynfu::Frame> DynFusion::extractSurface(int frame_id, bool with_normals) {
    auto triangles = mc_->run(tsdf(), mc_buffer_);  // :73-75 / :119-121 (one host sync: the vertex count)
    // convertToMesh (:76 / :122) on demand, in getMesh(): the float4 triangle soup stays in mc_buffer_ until then
    mesh_source_ = triangles, mesh_.reset(), mesh_triangles_.clear(), mesh_downloaded_ = false;
    const size_t nv = triangles.size();
    if (nv == 0) return std::make_shared<dynfu::Frame>(frame_id, dfa::PointCloud<dfa::PointXYZ>(), dfa::PointCloud<dfa::Normal>());
    // pcl::fromPCLPointCloud2 / copyPointCloud (:80-88): the vertices as a cloud of their own — packed N x 3 in HBM
    dfa::DeviceArray<float> v3(3 * nv), n3(3 * nv);
    dfa::check(dfa_repack_points((const float*)triangles.ptr(), 4, v3.ptr(), 3, (int)nv, 0.f, nullptr), "DynFusion: vertices");
    if (with_normals) {  // extension: gradient of the TSDF at the vertices
        dfa::DeviceArray<dfa::Normal> dn;
        mc_->computeNormals(tsdf(), triangles, dn);
        dfa::check(dfa_repack_points((const float*)dn.ptr(), 4, n3.ptr(), 3, (int)nv, 0.f, nullptr), "DynFusion: normals");
    } else {
        // pcl::copyPointCloud<PointXYZ, Normal> (:87-88 / :133-134) copies the fields the two types share — none:
        // the normals are default-constructed, one per vertex
        if (hipMemsetAsync(n3.ptr(), 0, 3 * nv * sizeof(float), nullptr) != hipSuccess)
            throw dfa::Error(DFA_ERR_HIP, "DynFusion::extractSurface: hipMemsetAsync");
    }
    return dynfu::Frame::fromDevice(frame_id, v3, n3, nv);
}

std::shared_ptr<dfa::PolygonMesh> DynFusion::getMesh() {  // KinFu::getMesh (kinfu.cpp:262)
    if (!mesh_) {
        if (!mesh_downloaded_) {
            mesh_triangles_.clear();
            if (!mesh_source_.empty()) mesh_source_.download(mesh_triangles_);
            mesh_downloaded_ = true;
        }
        mesh_ = std::make_shared<dfa::PolygonMesh>(dfa::convertToMesh(mesh_triangles_));
    }
    return mesh_;
}

// frame 0 with a fusion switch on: the canonical volume starts as what frame 0 saw
void DynFusion::createCanonicalVolume() {
    canonical_volume_ = std::make_shared<kfusion::cuda::TsdfVolume>(tsdf().getDims());
    canonical_volume_->setSize(tsdf().getSize()), canonical_volume_->setPose(tsdf().getPose());
    canonical_volume_->setTruncDist(tsdf().getTruncDist()), canonical_volume_->setMaxWeight(tsdf().getMaxWeight());
    canonical_volume_->setRaycastStepFactor(tsdf().getRaycastStepFactor());
    canonical_volume_->setGradientDeltaFactor(tsdf().getGradientDeltaFactor());
    canonical_volume_->copyVoxelsFrom(tsdf());
    knn_field_dropped_ = false;
    if (dynfuParams.fuse_knn_field) syncKnnField();
}

// fuse_knn_field, before a warped integrate (and at frame 0): the canonical volume's k-NN field over the nodes as they are
// now — built when there is none yet, appended to when the warp field has grown (Warpfield::update only appends).  Beyond
// fuse_knn_field_max_bytes the field is dropped for good and the integrations search.
void DynFusion::syncKnnField() {
    if (knn_field_dropped_) return;
    const Warpfield::DeviceNodeView nodes = warpfield->deviceNodes(false);
    kfusion::cuda::TsdfVolume& vol        = *canonical_volume_;
    bool ok = true;
    if (!vol.knnField()) {
        const dfa::Affine3f camera;  // north-star mode: the node frame is frame 0's camera, which stays at the origin
        ok = vol.buildKnnField(nodes.pos, nodes.w, nodes.D, dynfuParams.north_star ? std::min(warpfield->getKnn(), 8) : warpfield->getKnn(),
                               dynfuParams.north_star ? &camera : nullptr, dynfuParams.fuse_knn_field_max_bytes);
    } else if (vol.knnFieldNodes() < nodes.D) {
        ok = vol.appendKnnField(nodes.pos, nodes.w, nodes.D);
    }
    if (!ok) knn_field_dropped_ = true;
}

bool DynFusion::operator()(const kfusion::cuda::Depth& depth) {
    const kfusion::KinFuParams& p = params_;                                                       // :51
    kfusion::cuda::Depth& depth_filtered_ = curr_.depth_pyr[0];
    kfusion::cuda::computeDists(depth, dists_, p.intr);                                            // :58
    kfusion::cuda::depthBilateralFilter(depth, depth_filtered_, p.bilateral_kernel_size, p.bilateral_sigma_spatial,
                                        p.bilateral_sigma_depth);                                  // :60-61
    if (p.icp_truncate_depth_dist > 0) kfusion::cuda::depthTruncation(depth_filtered_, p.icp_truncate_depth_dist);  // :64-66
    if (dynfuParams.north_star) return northStarFrame(depth);
    const dfa::Affine3f camera;  // poses_.back(): the rigid tracker is skipped, the camera stays at the origin (:100-105)
    if (frame_counter_ == 0) {
        tsdf().integrate(dists_, camera, p.intr);  // :71
        initFromFrame(extractSurface(0, dynfuParams.mesh_normals));  // :73-95
        if (dynfuParams.model_view) keepCanonicalMesh(nullptr);
        if (dynfuParams.fuse_canonical) createCanonicalVolume();
        return ++frame_counter_, false;
    }
    StageClock clk;
    tsdf().clearAndIntegrate(dists_, camera, p.intr);  // :113-114 as one sweep
    clk.mark("pre-process + fuse");
    auto live = extractSurface(frame_counter_, dynfuParams.mesh_normals);
    clk.mark("marching cubes -> live frame");
    addLiveFrame(frame_counter_, live);  // :137
    warpCanonicalToLiveOpt(camera);      // :140
    clk.mark("warpCanonicalToLiveOpt");
    if (dynfuParams.fuse_canonical) {  // step 4 of :39-47: this frame's depth into the canonical volume, through the solved field
        if (dynfuParams.fuse_knn_field) syncKnnField();
        const Warpfield::DeviceNodeView nodes = warpfield->deviceNodes();
        canonical_volume_->integrateWarped(dists_, camera, p.intr, nodes.pos, nodes.dq, nodes.w, nodes.D, warpfield->getKnn(), unsupportedMode());
        clk.mark("integrateWarped");
    }
    warpfield->update(getCanonicalWarpedToLive());    // :142
    clk.mark("warpfield->update");
    return ++frame_counter_, true;
}

// The same frame sequence with the north-star solve in the middle: the live side of the solve is the depth frame itself
// (vertex / normal maps of the filtered depth, as KinFu builds them for its tracker, kinfu.cpp:150-175), so neither the
// live marching-cubes cloud nor the nearest-neighbour correspondence is on the path; everything the solve sees is in
// the camera frame.
bool DynFusion::northStarFrame(const kfusion::cuda::Depth& depth) {
    const kfusion::KinFuParams& p = params_;
    kfusion::cuda::Depth& depth_filtered_ = curr_.depth_pyr[0];
    const dfa::Affine3f camera;  // the camera stays at the origin, as in the reference's operator() (:100-105)
    if (frame_counter_ == 0) {
        tsdf().integrate(dists_, camera, p.intr);
        if (dynfuParams.north_star_regrow_canonical) {
            // the canonical cloud is the WELDED vertex set (frame 0 holds weight 1 only: no floor), and with model_view the
            // kept mesh is the cloud's mesh; every later frame replaces both from the canonical volume
            float aff[12];
            (camera.inv() * tsdf().getPose()).to12(aff);
            kfusion::cuda::MarchingCubes::IndexedMesh mesh;
            auto welded = extractWeldedModel(tsdf(), 1, aff, mesh);
            if (!welded) throw dfa::Error(DFA_ERR_INVALID, "DynFusion (north-star mode): the first frame has no surface");
            initFromFrame(welded);
            if (dynfuParams.model_view) canonical_mesh_frame_ = welded, canonical_mesh_ = mesh;
            createCanonicalVolume();
            return ++frame_counter_, false;
        }
        auto vol_frame = extractSurface(0, true);  // volume frame, normals from the TSDF gradient
        const size_t n = vol_frame->size();
        if (n == 0) throw dfa::Error(DFA_ERR_INVALID, "DynFusion (north-star mode): the first frame has no surface");
        // volume frame -> camera frame: camera_pose^-1 * volume_pose, the inverse of what integrate() applies (tsdf_volume.cpp:83)
        float aff[12];
        (camera.inv() * tsdf().getPose()).to12(aff);
        const dynfu::Frame::DeviceView v = vol_frame->device();
        dfa::DeviceArray<float> cv(3 * n), cn(3 * n);
        dfa::check(dfa_transform_points(v.vertices, (int)n, aff, 1, cv.ptr(), nullptr), "DynFusion: canonical vertices to the camera frame");
        dfa::check(dfa_transform_points(v.normals, (int)n, aff, 0, cn.ptr(), nullptr), "DynFusion: canonical normals to the camera frame");
        initFromFrame(dynfu::Frame::fromDevice(0, cv, cn, n));
        if (dynfuParams.model_view) keepCanonicalMesh(aff);
        if (dynfuParams.north_star_fuse_canonical) createCanonicalVolume();
        return ++frame_counter_, false;
    }
    StageClock clk;
    tsdf().clearAndIntegrate(dists_, camera, p.intr);
    addLiveFrame(frame_counter_, extractSurface(frame_counter_, dynfuParams.mesh_normals));  // for getLiveFrame() / getMesh()
    clk.mark("pre-process + fuse + marching cubes");
    NorthStarSolver solver(*warpfield, dynfuParams.northStarParams, dynfuParams.tukeyOffset, dynfuParams.psi_data,
                           dynfuParams.lambda, dynfuParams.psi_reg);
    if (dynfuParams.north_star_reg_hierarchy)
        solver.setRegHierarchy(std::vector<int>(dynfuParams.reg_level_slots.begin(), dynfuParams.reg_level_slots.begin() + regLevels()),
                               dynfuParams.epsilon, dynfuParams.beta);
    solver.initializeProblemInstance(canonicalFrame);
    if (dynfuParams.north_star_reg_hierarchy) {
        reg_node_levels_ = solver.nodeLevels();
        reg_level_counts_.assign((size_t)regLevels(), 0);
        for (int lv : reg_node_levels_) ++reg_level_counts_[(size_t)lv];
    }
    clk.mark("  initializeProblemInstance");
    const bool prealign = dynfuParams.north_star_rigid_prealign && (dynfuParams.rigid_prealign_device || dynfuParams.rigid_prealign_iters > 0);
    if (prealign) {
        // the global rigid motion first: the start transforms and the shared nodes come out composed with it, so everything
        // below — the model view, the visibility test, the solve, the fusion — sees the aligned field
        kfusion::cuda::computePointNormals(p.intr, depth_filtered_, live_points_, live_normals_);
        bool aligned;
        if (dynfuParams.rigid_prealign_device) {
            NorthStarSolver::RigidSchedule schedule;
            schedule.steps = dynfuParams.rigid_prealign_steps, schedule.iters = dynfuParams.rigid_prealign_level_iters;
            schedule.stopRot = dynfuParams.rigid_prealign_stop_rot, schedule.stopTrans = dynfuParams.rigid_prealign_stop_trans;
            aligned          = solver.alignRigid(live_points_, live_normals_, p.intr, schedule, rigid_pose_);
            rigid_iters_run_ = solver.rigidIterationsRun();
        } else {
            aligned = solver.alignRigid(live_points_, live_normals_, p.intr, dynfuParams.rigid_prealign_iters, rigid_pose_);
        }
        if (!aligned) ++rigid_skipped_;
        rigid_matched_first_ = solver.rigidMatchedFirst(), rigid_matched_last_ = solver.rigidMatchedLast();
        clk.mark("  alignRigid");
    }
    if (dynfuParams.north_star_visible_only) {
        // the model as the solve finds it: mesh and cloud warped by the transforms the solve starts from, the mesh rasterised
        // from this frame's camera; a vertex behind the rasterised surface takes no data row
        rasterizeWarpedModel();
        const dfa::DeviceArray<float> start = solver.warpCanonicalByStart();
        float z_tol = dynfuParams.visibility_z_tol;
        if (z_tol == 0.f) {
            const kfusion::Vec3f vs = tsdf().getVoxelSize();
            z_tol = 2.f * std::max(vs[0], std::max(vs[1], vs[2]));
        }
        kfusion::cuda::visibleVertices(start.ptr(), 3, canonicalFrame->size(), model_points_, p.intr, z_tol, visible_flags_, &visible_count_);
        solver.setVertexMask(visible_flags_);
        visible_counted_ = true;
        clk.mark("  visible vertices");
    }
    if (!prealign) kfusion::cuda::computePointNormals(p.intr, depth_filtered_, live_points_, live_normals_);
    solver.solveAll(live_points_, live_normals_, p.intr);
    clk.mark("  solveAll");
    ns_initial_cost_ = solver.initialCost(), ns_final_cost_ = solver.finalCost(), ns_valid_rows_ = solver.validRows();
    ns_pcg_iters_ = solver.pcgIterations(), ns_gn_solves_ = solver.gnSolves();
    if (dynfuParams.north_star_fuse_canonical) {
        // this frame's depth into the canonical volume through the solved field: the nodes hold the solved transforms now, and
        // the field has not grown yet.  The node frame is frame 0's camera — `camera`: it stays at the origin
        if (dynfuParams.fuse_knn_field) syncKnnField();
        const Warpfield::DeviceNodeView nodes = warpfield->deviceNodes();
        canonical_volume_->integrateWarped6(dists_, camera, p.intr, camera, nodes.pos, nodes.dq, nodes.w, nodes.D,
                                            std::min(warpfield->getKnn(), 8), unsupportedMode());
        clk.mark("integrateWarped6");
    }
    canonicalFrameWarpedToLive = solver.warpCanonicalToLive();  // the cloud the solve used
    if (dynfuParams.north_star_regrow_canonical) {
        // the canonical model grows: the cloud (and the kept mesh) of the next frame is the canonical volume's surface as it is
        // now, from the voxels seen canonical_min_weight times, and the field is extended where THAT cloud — in canonical
        // space — has no support.  An empty extraction keeps the old model.
        float aff[12];
        (camera.inv() * tsdf().getPose()).to12(aff);
        kfusion::cuda::MarchingCubes::IndexedMesh mesh;
        if (auto grown = extractWeldedModel(*canonical_volume_, dynfuParams.canonical_min_weight, aff, mesh)) {
            canonicalFrame = grown;
            if (dynfuParams.model_view) canonical_mesh_frame_ = grown, canonical_mesh_ = mesh, mesh_plan_stale_ = true;
        } else {
            ++regrow_skipped_;
        }
        clk.mark("warp + regrow");
        const size_t nodes_before = warpfield->nodesRef().size();
        warpfield->update(canonicalFrame);
        startNewNodesFromBlend(nodes_before);
        clk.mark("warpfield->update");
        return ++frame_counter_, true;
    }
    warpfield->update(canonicalFrameWarpedToLive);
    clk.mark("warp + warpfield->update");
    return ++frame_counter_, true;
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
    const int k = (int)std::min<size_t>((size_t)std::min(warpfield->getKnn(), 8), nodes_before);
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

// ------------------------------------------------------------------------- the view of the canonical model

// frame 0, model_view: the volume just fused as a welded mesh with normals from the TSDF gradient, moved to the frame of the
// canonical cloud exactly as the cloud is (north-star mode: the camera frame)
void DynFusion::keepCanonicalMesh(const float* to_canonical_frame) {
    kfusion::cuda::MarchingCubes::IndexedMesh mesh;
    auto frame = extractWeldedModel(tsdf(), 1, to_canonical_frame, mesh);
    if (!frame) throw dfa::Error(DFA_ERR_INVALID, "DynFusion (model_view): the first frame has no surface");
    canonical_mesh_frame_ = frame;
    canonical_mesh_       = mesh;
}

// `volume` as a welded mesh (views of mesh_vertex_buffer_ / mesh_index_buffer_: the mesh extracted before is overwritten) from
// the voxels of weight >= min_weight, and its vertices with normals from the TSDF gradient as a frame, both moved by
// `to_frame` (12 floats, or null).  Null when the volume has no such surface: the buffers are then untouched.
std::shared_ptr<dynfu::Frame> DynFusion::extractWeldedModel(const kfusion::cuda::TsdfVolume& volume, int min_weight,
                                                            const float* to_frame,
                                                            kfusion::cuda::MarchingCubes::IndexedMesh& mesh) {
    mesh = mc_->runIndexed(volume, mesh_vertex_buffer_, mesh_index_buffer_, min_weight);
    if (mesh.vertices.empty() && mc_->totalUniqueVertices() > 0) {  // it did not fit the default buffers: size them and run again
        mesh_vertex_buffer_.create((size_t)mc_->totalUniqueVertices());
        mesh_index_buffer_.create((size_t)mc_->totalVertices());
        mesh = mc_->runIndexed(volume, mesh_vertex_buffer_, mesh_index_buffer_, min_weight);
    }
    const size_t n = mesh.vertices.size();
    if (n == 0) return nullptr;
    dfa::DeviceArray<dfa::Normal> normals4;
    mc_->computeNormals(volume, mesh.vertices, normals4);
    dfa::DeviceArray<float> v3(3 * n), n3(3 * n);
    dfa::check(dfa_repack_points((const float*)mesh.vertices.ptr(), 4, v3.ptr(), 3, (int)n, 0.f, nullptr), "DynFusion: mesh vertices");
    dfa::check(dfa_repack_points((const float*)normals4.ptr(), 4, n3.ptr(), 3, (int)n, 0.f, nullptr), "DynFusion: mesh normals");
    if (to_frame) {
        dfa::check(dfa_transform_points(v3.ptr(), (int)n, to_frame, 1, v3.ptr(), nullptr), "DynFusion: mesh vertices to the camera frame");
        dfa::check(dfa_transform_points(n3.ptr(), (int)n, to_frame, 0, n3.ptr(), nullptr), "DynFusion: mesh normals to the camera frame");
        // the float4 vertices getCanonicalMesh() hands out follow (in place: the buffer is this object's)
        dfa::check(dfa_repack_points(v3.ptr(), 3, (float*)mesh.vertices.ptr(), 4, (int)n, 1.f, nullptr), "DynFusion: mesh vertices");
    }
    return dynfu::Frame::fromDevice(0, v3, n3, n);
}

// The mesh moves as the canonical cloud does: by the blend of the solve that fitted the transforms.  Reference mode:
// Warpfield::warpToLive.  North-star mode: the solve's own warp (solve6_update.hip, s6_warp) on a plan that holds the mesh as its
// cloud and never solves — the frame's plan is not touched, so a frame cannot notice the view.
std::shared_ptr<dynfu::Frame> DynFusion::warpCanonicalMesh() {
    if (!dynfuParams.model_view) throw dfa::Error(DFA_ERR_INVALID, "DynFusion::renderWarpedModel: DynFuParams::model_view is off");
    if (!canonical_mesh_frame_ || !warpfield) throw dfa::Error(DFA_ERR_INVALID, "DynFusion::renderWarpedModel before the first frame");
    if (!dynfuParams.north_star) return warpfield->warpToLive(canonical_mesh_frame_);
    std::vector<float> pos, w, dq;
    warpfield->hostArrays(pos, w, dq);
    const int D = (int)w.size();
    const size_t n = canonical_mesh_frame_->size();
    if (D == 0) throw dfa::Error(DFA_ERR_INVALID, "DynFusion::renderWarpedModel: the warp field has no nodes");
    mesh_node_dq_.upload(dq);
    // (mesh_plan_stale_: north_star_regrow_canonical has replaced the mesh — the plan holds the old one's vertices)
    if (!mesh_plan_ || mesh_plan_stale_ || pos != mesh_nodes_built_pos_ || w != mesh_nodes_built_w_) {
        if (!mesh_plan_ || D > mesh_plan_D_ || n > mesh_plan_N_) {
            mesh_plan_.reset();
            dfa_solver6* plan = nullptr;
            const int cap = D + D / 4 + 16;  // (room for the nodes Warpfield::update adds, as NorthStarSolver sizes its plan)
            // (... and, where the mesh grows from frame to frame, for the vertices the next extractions add)
            const size_t cap_n = dynfuParams.north_star_regrow_canonical ? n + n / 4 + 1024 : n;
            dfa::check(dfa_solver6_create(cap, (int)cap_n, std::min(warpfield->getKnn(), 8), &plan), "DynFusion (model_view): dfa_solver6_create");
            mesh_plan_ = std::shared_ptr<dfa_solver6>(plan, dfa_solver6_destroy);
            mesh_plan_D_ = cap, mesh_plan_N_ = cap_n;
        }
        // fresh arrays: the plan borrows them until the next set_problem
        mesh_node_pos_ = dfa::DeviceArray<float>(), mesh_node_w_ = dfa::DeviceArray<float>();
        mesh_node_pos_.upload(pos), mesh_node_w_.upload(w);
        const dynfu::Frame::DeviceView m = canonical_mesh_frame_->device();
        dfa::check(dfa_solver6_set_problem(mesh_plan_.get(), mesh_node_pos_.ptr(), mesh_node_dq_.ptr(), mesh_node_w_.ptr(), D, m.vertices,
                                           m.normals, (int)n, nullptr),
                   "DynFusion (model_view): dfa_solver6_set_problem");
        mesh_nodes_built_pos_ = pos, mesh_nodes_built_w_ = w, mesh_plan_stale_ = false;
    }
    dfa::DeviceArray<float> ov(3 * n), on(3 * n);
    dfa::check(dfa_solver6_warp_with(mesh_plan_.get(), mesh_node_dq_.ptr(), ov.ptr(), on.ptr(), nullptr), "DynFusion (model_view): dfa_solver6_warp_with");
    return dynfu::Frame::fromDevice(0, ov, on, n);
}

long long DynFusion::northStarVisibleVertices() const {
    if (!visible_counted_) return -1;
    std::vector<int> n;
    visible_count_.download(n);  // (a blocking copy on the default stream: behind the frame's work)
    return n.empty() ? -1 : n[0];
}

void DynFusion::rasterizeWarpedModel() {
    const auto warped = warpCanonicalMesh();
    const kfusion::KinFuParams& p = params_;
    const dynfu::Frame::DeviceView w = warped->device();
    if (w.n != canonical_mesh_frame_->size()) throw dfa::Error(DFA_ERR_INVALID, "DynFusion::renderWarpedModel: the warp field has no nodes");
    if (warped_vertices_.size() != w.n) warped_vertices_.create(w.n), warped_normals_.create(w.n);
    dfa::check(dfa_repack_points(w.vertices, 3, (float*)warped_vertices_.ptr(), 4, (int)w.n, 1.f, nullptr), "DynFusion: warped vertices");
    dfa::check(dfa_repack_points(w.normals, 3, (float*)warped_normals_.ptr(), 4, (int)w.n, 0.f, nullptr), "DynFusion: warped normals");
    // north-star mode keeps the model in the camera frame; otherwise it is in the volume's frame, as the canonical cloud is
    const dfa::Affine3f world2cam = dynfuParams.north_star ? dfa::Affine3f() : getCameraPose().inv() * tsdf().getPose();
    kfusion::cuda::rasterizeMesh(warped_vertices_, warped_normals_, canonical_mesh_.indices, world2cam, p.intr, p.cols, p.rows,
                                 dynfuParams.model_view_z_near, model_points_, model_normals_, model_zbuffer_);
}

void DynFusion::renderWarpedModel(kfusion::cuda::Image& image, int flag) {
    rasterizeWarpedModel();
    const kfusion::KinFuParams& p = params_;
    image.create(p.rows, flag != 3 ? p.cols : p.cols * 2);  // as KinFu::renderImage
    if (flag == 2) kfusion::cuda::renderTangentColors(model_normals_, image);
    else if (flag != 3) kfusion::cuda::renderImage(model_points_, model_normals_, p.intr, p.light_pose, image);
    else {
        kfusion::cuda::Image i1(p.rows, p.cols, image.ptr(), image.step()), i2(p.rows, p.cols, image.ptr() + p.cols, image.step());
        kfusion::cuda::renderImage(model_points_, model_normals_, p.intr, p.light_pose, i1);
        kfusion::cuda::renderTangentColors(model_normals_, i2);
    }
}

SequenceReport runSequence(DynFusion& dynfu, const std::string& dir, int max_frames) {
    const dfa::io::SequenceFiles files = dfa::io::listSequence(dir);  // demo.cpp:39-55
    if (files.images.size() < files.depths.size())
        throw dfa::Error(1, "fewer colour images than depth frames in " + dir);  // the demo indexes images[i]
    const std::string out = dir + "/out";                                      // demo.cpp:58-66
    std::filesystem::create_directory(out);
    SequenceReport rep;
    kfusion::cuda::Depth depth_device;
    const size_t n = max_frames < 0 ? files.depths.size() : std::min(files.depths.size(), (size_t)max_frames);
    for (size_t i = 0; i < n; ++i) {
        const dfa::io::DepthImage depth = dfa::io::readDepthPng(files.depths[i]);  // demo.cpp:81
        depth_device.upload(depth.data.data(), (size_t)depth.cols * sizeof(uint16_t), depth.rows, depth.cols);  // :90
        const auto t0        = std::chrono::steady_clock::now();
        const bool has_image = dynfu(depth_device);  // :94
        rep.frame_ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        rep.dynfu_ms += rep.frame_ms.back();
        ++rep.frames;
        if (has_image) {  // :115-118
            dfa::io::savePCDFileASCII(out + "/pcl_canonical_to_live" + std::to_string(i) + ".pcd",
                                      dynfu.getCanonicalWarpedToLive()->vertices());
            dfa::io::saveVTKFile(out + "/" + std::to_string(i) + "_tsdf_mesh.vtk", *dynfu.getMesh());
            if (i + 1 < n) dynfu.dropMesh();  // the demo's mesh pointer goes out of scope here, outside the timed call
            ++rep.saved;
        }
    }
    return rep;
}
