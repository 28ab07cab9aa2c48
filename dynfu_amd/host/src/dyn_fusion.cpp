// dyn_fusion.cpp — DynFusion's warp-field sequence on the dynfu_amd C ABI
// (reference: src/dynfu/dyn_fusion.cpp:6-31,147-242).
#include <dynfu/dyn_fusion.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <filesystem>

#include <dfa_host/device.hpp>

#include "../../../include/dynfu_amd.h"
#include "stage_clock.hpp"

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

int DynFuParams::regLevels() const { return (int)std::min<size_t>((size_t)std::max(L + 1, 0), reg_level_slots.size()); }

void DynFuParams::validate() const {
    if (fuse_canonical && north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: fuse_canonical is a reference-mode extension (north_star blends otherwise, in the camera frame: north_star_fuse_canonical)");
    if (north_star_fuse_canonical && !north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_fuse_canonical needs north_star (reference mode: fuse_canonical)");
    if (north_star_fuse_color && !north_star_fuse_canonical)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_fuse_color needs north_star_fuse_canonical (colour rides on that fusion's sweep)");
    if (north_star_fuse_color && (canonical_max_color_weight < 1 || canonical_max_color_weight > 255))
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_fuse_color: canonical_max_color_weight outside 1..255");
    if (fuse_knn_field && !fuse_canonical && !north_star_fuse_canonical)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: fuse_knn_field serves the canonical fusion (fuse_canonical or north_star_fuse_canonical)");
    if (north_star_visible_only && !(north_star && model_view))
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_visible_only needs north_star and model_view (the rasterised canonical mesh is what hides a vertex)");
    if (fuse_unsupported_rigid && !fuse_canonical && !north_star_fuse_canonical)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: fuse_unsupported_rigid serves the canonical fusion (fuse_canonical or north_star_fuse_canonical)");
    if (north_star_regrow_canonical && !north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_regrow_canonical needs north_star (reference mode keeps frame 0's cloud)");
    if (north_star_regrow_canonical && !north_star_fuse_canonical)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_regrow_canonical needs north_star_fuse_canonical (the canonical volume is what the cloud is re-extracted from)");
    if (north_star_regrow_canonical && (canonical_min_weight < 1 || canonical_min_weight > 65535))
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: canonical_min_weight outside 1..65535");
    if (north_star_rigid_prealign && !north_star)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_rigid_prealign needs north_star (reference mode has no rigid step: KinFu tracks rigidly)");
    if (north_star_rigid_prealign && rigid_prealign_iters < 0)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: negative rigid_prealign_iters");
    if (rigid_prealign_device) {
        if (!north_star_rigid_prealign)
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: rigid_prealign_device needs north_star_rigid_prealign (it is that step's loop, on the device)");
        const std::vector<int>&st = rigid_prealign_steps, &it = rigid_prealign_level_iters;
        long total = 0;
        for (int n : it) total += n;
        bool ok = !st.empty() && st.size() <= 4 && st.size() == it.size() && total <= 64;
        for (int v : st) ok = ok && v >= 1;
        for (int n : it) ok = ok && n >= 0;
        if (!ok)
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: rigid_prealign_steps / rigid_prealign_level_iters: 1 to 4 levels, steps >= 1, iterations >= 0 and at most 64 in all");
        if (!(rigid_prealign_stop_rot >= 0.f) || !(rigid_prealign_stop_trans >= 0.f))
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: negative or NaN rigid_prealign_stop_rot / rigid_prealign_stop_trans");
    }
    if (north_star_reg_hierarchy) {
        if (!north_star)
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_reg_hierarchy needs north_star (the reference-mode solve keeps its flat graph)");
        // (the field is created with KNN neighbours; a k set later is checked by the frame)
        const std::vector<int> slots(reg_level_slots.begin(), reg_level_slots.begin() + regLevels());
        if (!NorthStarSolver::regHierarchyAccepted(slots, epsilon, beta, northStarKnn(KNN)))
            throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_reg_hierarchy: 1 to 8 levels (min(L + 1, reg_level_slots.size())), reg_level_slots[0] >= 1, no negative slot, a slot sum of at most the warp field's k (and 8), beta >= 2, epsilon > 0");
    }
}

DynFusion::DynFusion(const DynFuParams& params) : kfusion::KinFu(params.kinfuParams), dynfuParams(params) {  // dyn_fusion.cpp:33
    params.validate();
    solverParams.numIter       = 24;  // dyn_fusion.cpp:183-189
    solverParams.nonLinearIter = 16;
    solverParams.linearIter    = 256;
    solverParams.useOpt        = true;
    solverParams.useOptLM      = false;
    solverParams.earlyOut      = true;
}
DynFusion::~DynFusion() = default;

DynFuParams& DynFusion::params() { return dynfuParams; }

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

void DynFusion::warpCanonicalToLiveOpt(dfa::Affine3f affine) {
    if (!warpfield || !canonicalFrame || !liveFrame)
        throw dfa::Error(DFA_ERR_INVALID, "warpCanonicalToLiveOpt before init / addLiveFrame");
    dfa::StageClock clk;
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
    correspondingFrame  = corresponding;
    solve_initial_cost_ = combinedSolver.initialCost(), solve_final_cost_ = combinedSolver.finalCost();
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

// ------------------------------------------------------------------------- the per-frame sequence (north-star mode:
// dyn_fusion_northstar.cpp; the view of the canonical model: dyn_fusion_model_view.cpp)

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
    const int k = dynfuParams.north_star ? northStarKnn(warpfield->getKnn()) : warpfield->getKnn();
    // (a field of another k — Warpfield::setKnn after frame 0 built it — serves no integration: it is built again)
    if (!vol.knnField() || vol.knnFieldK() != k) {
        const dfa::Affine3f camera;  // north-star mode: the node frame is frame 0's camera, which stays at the origin
        ok = vol.buildKnnField(nodes.pos, nodes.w, nodes.D, k, dynfuParams.north_star ? &camera : nullptr, dynfuParams.fuse_knn_field_max_bytes);
    } else if (vol.knnFieldNodes() < nodes.D) {
        ok = vol.appendKnnField(nodes.pos, nodes.w, nodes.D);
    }
    if (!ok) knn_field_dropped_ = true;
}

bool DynFusion::operator()(const kfusion::cuda::Depth& depth) {
    if (dynfuParams.north_star_fuse_color)
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: north_star_fuse_color is on: a frame needs its colour image, operator()(depth, color)");
    return frame(depth);
}

bool DynFusion::operator()(const kfusion::cuda::Depth& depth, const kfusion::cuda::Image& color) {
    if (!dynfuParams.north_star_fuse_color) return frame(depth);  // (the image is not read)
    if (color.rows() != depth.rows() || color.cols() != depth.cols())
        throw dfa::Error(DFA_ERR_INVALID, "DynFusion: the colour image is not the depth frame's size (north_star_fuse_color takes registered frames)");
    frame_color_ = &color;
    try {
        const bool tracked = frame(depth);
        frame_color_ = nullptr;
        return tracked;
    } catch (...) {
        frame_color_ = nullptr;
        throw;
    }
}

bool DynFusion::frame(const kfusion::cuda::Depth& depth) {
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
    dfa::StageClock clk;
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
