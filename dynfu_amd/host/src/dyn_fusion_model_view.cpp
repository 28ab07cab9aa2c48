// dyn_fusion_model_view.cpp — DynFusion's view of the canonical model (DynFuParams::model_view): the kept
// welded mesh, its warp by the mode's blend, the rasterised maps and the shaded images.
#include <dynfu/dyn_fusion.hpp>

#include <dfa_host/device.hpp>
#include <dfa_host/plan_cache.hpp>

#include "../../../include/dynfu_amd.h"

// North-star mode: a dfa_solver6 plan of the view's own that holds the mesh as its cloud and never solves — the frame's plan
// (NorthStarSolver's, and its cache) is not touched, so a frame cannot notice the view.  Its graphs are rebuilt when the node
// positions or weights differ from those they were built from, or the mesh was replaced; the plan is reallocated when either
// outgrows its capacity.
class DynFusion::MeshWarpPlan {
public:
    void meshReplaced() { stale_ = true; }  // the plan holds the old mesh's vertices
    // `mesh` warped by the transforms `dq` of the nodes (pos, w), blending k of them; mesh_grows: capacity for the vertices
    // the next extractions add
    std::shared_ptr<dynfu::Frame> warp(const std::vector<float>& pos, const std::vector<float>& w, const std::vector<float>& dq,
                                       int k, const dynfu::Frame& mesh, bool mesh_grows) {
        const int D    = (int)w.size();
        const size_t n = mesh.size();
        node_dq_.upload(dq);
        if (!plan_ || stale_ || pos != built_pos_ || w != built_w_) {
            if (!plan_ || D > cap_D_ || n > cap_N_) {
                plan_.reset();
                dfa_solver6* plan = nullptr;
                cap_D_ = dfa::grown_node_capacity(D), cap_N_ = mesh_grows ? dfa::grown_vertex_capacity(n) : n;
                dfa::check(dfa_solver6_create(cap_D_, (int)cap_N_, k, &plan), "DynFusion (model_view): dfa_solver6_create");
                plan_ = std::shared_ptr<dfa_solver6>(plan, dfa_solver6_destroy);
            }
            // fresh arrays: the plan borrows them until the next set_problem
            node_pos_ = dfa::DeviceArray<float>(), node_w_ = dfa::DeviceArray<float>();
            node_pos_.upload(pos), node_w_.upload(w);
            const dynfu::Frame::DeviceView m = mesh.device();
            dfa::check(dfa_solver6_set_problem(plan_.get(), node_pos_.ptr(), node_dq_.ptr(), node_w_.ptr(), D, m.vertices, m.normals,
                                               (int)n, nullptr),
                       "DynFusion (model_view): dfa_solver6_set_problem");
            built_pos_ = pos, built_w_ = w, stale_ = false;
        }
        dfa::DeviceArray<float> ov(3 * n), on(3 * n);
        dfa::check(dfa_solver6_warp_with(plan_.get(), node_dq_.ptr(), ov.ptr(), on.ptr(), nullptr), "DynFusion (model_view): dfa_solver6_warp_with");
        return dynfu::Frame::fromDevice(0, ov, on, n);
    }

private:
    std::shared_ptr<dfa_solver6> plan_;
    int cap_D_    = 0;
    size_t cap_N_ = 0;
    bool stale_   = false;
    dfa::DeviceArray<float> node_pos_, node_w_, node_dq_;  // what the plan borrows
    std::vector<float> built_pos_, built_w_;               // the node set its graphs were built from
};

// frame 0, model_view: the volume just fused as a welded mesh with normals from the TSDF gradient, moved to the frame of the
// canonical cloud exactly as the cloud is (north-star mode: the camera frame)
void DynFusion::keepCanonicalMesh(const float* to_canonical_frame) {
    kfusion::cuda::MarchingCubes::IndexedMesh mesh;
    auto frame = extractWeldedModel(tsdf(), 1, to_canonical_frame, mesh);
    if (!frame) throw dfa::Error(DFA_ERR_INVALID, "DynFusion (model_view): the first frame has no surface");
    setCanonicalMesh(frame, mesh);
}

void DynFusion::setCanonicalMesh(std::shared_ptr<dynfu::Frame> frame, const kfusion::cuda::MarchingCubes::IndexedMesh& mesh) {
    canonical_mesh_frame_ = frame;
    canonical_mesh_       = mesh;
    if (mesh_warp_) mesh_warp_->meshReplaced();
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
// Warpfield::warpToLive.  North-star mode: the solve's own warp (solve6_update.hip, s6_warp) on the view's plan.
std::shared_ptr<dynfu::Frame> DynFusion::warpCanonicalMesh() {
    if (!dynfuParams.model_view) throw dfa::Error(DFA_ERR_INVALID, "DynFusion::renderWarpedModel: DynFuParams::model_view is off");
    if (!canonical_mesh_frame_ || !warpfield) throw dfa::Error(DFA_ERR_INVALID, "DynFusion::renderWarpedModel before the first frame");
    if (!dynfuParams.north_star) return warpfield->warpToLive(canonical_mesh_frame_);
    std::vector<float> pos, w, dq;
    warpfield->hostArrays(pos, w, dq);
    if (w.empty()) throw dfa::Error(DFA_ERR_INVALID, "DynFusion::renderWarpedModel: the warp field has no nodes");
    if (!mesh_warp_) mesh_warp_ = std::make_shared<MeshWarpPlan>();
    return mesh_warp_->warp(pos, w, dq, northStarKnn(warpfield->getKnn()), *canonical_mesh_frame_, dynfuParams.north_star_regrow_canonical);
}

long long DynFusion::northStarVisibleVertices() const {
    if (!report_.visible_counted) return -1;
    std::vector<int> n;
    report_.visible_count.download(n);  // (a blocking copy on the default stream: behind the frame's work)
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
