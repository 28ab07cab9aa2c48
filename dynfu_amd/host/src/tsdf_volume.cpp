// tsdf_volume.cpp — kfusion::cuda::TsdfVolume on the dynfu_amd C ABI
// (host logic follows src/kfusion/tsdf_volume.cpp:18-129; kernels are in libdynfu_amd.so).
#include <algorithm>
#include <cstring>

#include <hip/hip_runtime.h>
#include <kfusion/cuda/tsdf_volume.hpp>

#include "../../../include/dynfu_amd.h"

using namespace kfusion;
using namespace kfusion::cuda;

void kfusion::cuda::computeDists(const Depth& depth, Dists& dists, const Intr& intr) {
    dists.create(depth.rows(), depth.cols());  // imgproc.cpp:39
    dfa::check(dfa_compute_dists(depth.ptr(), (int)depth.step(), dists.ptr(), (int)dists.step(), depth.cols(),
                                 depth.rows(), intr.fx, intr.fy, intr.cx, intr.cy, nullptr),
               "computeDists");
}

float TsdfVolume::Entry::half2float(half) { throw "Not implemented"; }               // tsdf_volume.cpp:9
TsdfVolume::Entry::half TsdfVolume::Entry::float2half(float) { throw "Not implemented"; }  // :11-13

void TsdfVolume::create(const Vec3i& dims) {  // :32-38
    cfg_.dims = dims;
    blob_.create((size_t)dims[0] * dims[1] * dims[2] * sizeof(int));
    occ_.create(dfa_tsdf_occupancy_bytes(dims[0], dims[1], dims[2]));
    setTruncDist(cfg_.trunc);
    clear();
}

void TsdfVolume::clear() {  // :74-80
    dfa::check(dfa_tsdf_clear_occ(blob_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], occ_.ptr<uint8_t>(), nullptr),
               "TsdfVolume::clear");
    occ_known_ = soleOwner();  // (a handle that is alive now may write the voxels later: no promise then)
}

void TsdfVolume::integrate(const Dists& dists, const Affine3f& camera_pose, const Intr& intr) {  // :82-93
    Affine3f vol2cam = camera_pose.inv() * cfg_.pose;
    float aff[12];
    vol2cam.to12(aff);
    const Vec3f vsz = getVoxelSize();
    if (mapTrusted())  // (the accumulating sweep only ADDS to the map: it has to be right before)
        dfa::check(dfa_tsdf_integrate_occ(dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), blob_.ptr<uint32_t>(),
                                          cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, cfg_.trunc, cfg_.max_weight, aff, intr.fx,
                                          intr.fy, intr.cx, intr.cy, occ_.ptr<uint8_t>(), nullptr),
                   "TsdfVolume::integrate");
    else
        dfa::check(dfa_tsdf_integrate(dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), blob_.ptr<uint32_t>(),
                                      cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, cfg_.trunc, cfg_.max_weight, aff, intr.fx,
                                      intr.fy, intr.cx, intr.cy, nullptr),
                   "TsdfVolume::integrate");
    dfa::device_synchronize();  // the reference's device::integrate blocks (tsdf_volume.cu:120)
}

void TsdfVolume::integrateWarped(const Dists& dists, const Affine3f& camera_pose, const Intr& intr, const float* node_pos,
                                 const float* node_dq, const float* node_w, int D, int k, UnsupportedMode mode) {
    Affine3f vol2cam = camera_pose.inv() * cfg_.pose;  // as integrate() forms it
    float aff[12];
    vol2cam.to12(aff);
    const Vec3f vsz = getVoxelSize();
    const int unsupported = mode == UnsupportedMode::Rigid ? DFA_WARPED_RIGID : DFA_WARPED_SKIP;
    // (the call only ADDS to the map, as the accumulating sweep does: it has to be right before)
    if (const dfa_knn_field* field = matchingField(k, D, nullptr))  // the neighbours are known: no search
        dfa::check(dfa_tsdf_integrate_warped_field(dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), blob_.ptr<uint32_t>(),
                                                   cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], mapTrusted() ? occ_.ptr<uint8_t>() : nullptr,
                                                   vsz.v, cfg_.trunc, cfg_.max_weight, aff, intr.fx, intr.fy, intr.cx, intr.cy, node_pos,
                                                   node_dq, node_w, D, k, unsupported, field, nullptr),
                   "TsdfVolume::integrateWarped (k-NN field)");
    else
        dfa::check(dfa_tsdf_integrate_warped(dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), blob_.ptr<uint32_t>(), cfg_.dims[0],
                                             cfg_.dims[1], cfg_.dims[2], mapTrusted() ? occ_.ptr<uint8_t>() : nullptr, vsz.v, cfg_.trunc,
                                             cfg_.max_weight, aff, intr.fx, intr.fy, intr.cx, intr.cy, node_pos, node_dq, node_w, D, k,
                                             unsupported, nullptr),
                   "TsdfVolume::integrateWarped");
    dfa::device_synchronize();  // (as integrate())
}

void TsdfVolume::integrateWarped6(const Dists& dists, const Affine3f& camera_pose, const Intr& intr, const Affine3f& node_frame_pose,
                                  const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                                  UnsupportedMode mode) {
    // the volume's frame -> the node frame -> this frame's camera; together camera_pose^-1 * pose_, as integrate() forms it
    float vol2node[12], node2cam[12];
    (node_frame_pose.inv() * cfg_.pose).to12(vol2node);
    (camera_pose.inv() * node_frame_pose).to12(node2cam);
    const Vec3f vsz = getVoxelSize();
    const int unsupported = mode == UnsupportedMode::Rigid ? DFA_WARPED_RIGID : DFA_WARPED_SKIP;
    // (the call only ADDS to the map, as the accumulating sweep does: it has to be right before)
    if (const dfa_knn_field* field = matchingField(k, D, vol2node))  // the neighbours are known: no search
        dfa::check(dfa_tsdf_integrate_warped6_field(dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), blob_.ptr<uint32_t>(),
                                                    cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], mapTrusted() ? occ_.ptr<uint8_t>() : nullptr,
                                                    vsz.v, cfg_.trunc, cfg_.max_weight, vol2node, node2cam, intr.fx, intr.fy, intr.cx,
                                                    intr.cy, node_pos, node_dq, node_w, D, k, unsupported, field, nullptr),
                   "TsdfVolume::integrateWarped6 (k-NN field)");
    else
        dfa::check(dfa_tsdf_integrate_warped6(dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), blob_.ptr<uint32_t>(), cfg_.dims[0],
                                              cfg_.dims[1], cfg_.dims[2], mapTrusted() ? occ_.ptr<uint8_t>() : nullptr, vsz.v, cfg_.trunc,
                                              cfg_.max_weight, vol2node, node2cam, intr.fx, intr.fy, intr.cx, intr.cy, node_pos, node_dq,
                                              node_w, D, k, unsupported, nullptr),
                   "TsdfVolume::integrateWarped6");
    dfa::device_synchronize();  // (as integrate())
}

// ---- colour
void TsdfVolume::createColors() {
    colors_.create((size_t)cfg_.dims[0] * cfg_.dims[1] * cfg_.dims[2] * sizeof(uint32_t));
    if (hipMemset(colors_.ptr<void>(), 0, colors_.sizeBytes()) != hipSuccess)
        throw dfa::Error(DFA_ERR_HIP, "TsdfVolume::createColors: hipMemset");
}

void TsdfVolume::integrateWarped6Color(const Dists& dists, const Image& image, const Affine3f& camera_pose, const Intr& intr,
                                       const Affine3f& node_frame_pose, const float* node_pos, const float* node_dq,
                                       const float* node_w, int D, int k, UnsupportedMode mode, bool update_tsdf, int max_color_weight) {
    if (colors_.empty()) throw dfa::Error(DFA_ERR_INVALID, "TsdfVolume::integrateWarped6Color: the volume has no colours (createColors)");
    if (image.rows() != dists.rows() || image.cols() != dists.cols())
        throw dfa::Error(DFA_ERR_INVALID, "TsdfVolume::integrateWarped6Color: the colour image is not the depth frame's size");
    float vol2node[12], node2cam[12];  // as integrateWarped6 forms them
    (node_frame_pose.inv() * cfg_.pose).to12(vol2node);
    (camera_pose.inv() * node_frame_pose).to12(node2cam);
    const Vec3f vsz = getVoxelSize();
    const int unsupported = mode == UnsupportedMode::Rigid ? DFA_WARPED_RIGID : DFA_WARPED_SKIP;
    const dfa_knn_field* field = matchingField(k, D, vol2node);  // (null: the call searches)
    dfa::check(dfa_tsdf_integrate_warped6_color(dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), (const uint8_t*)image.ptr(),
                                                (int)image.step(), update_tsdf ? blob_.ptr<uint32_t>() : nullptr, colors_.ptr<uint32_t>(),
                                                cfg_.dims[0], cfg_.dims[1], cfg_.dims[2],
                                                update_tsdf && mapTrusted() ? occ_.ptr<uint8_t>() : nullptr, vsz.v, cfg_.trunc,
                                                cfg_.max_weight, max_color_weight, vol2node, node2cam, intr.fx, intr.fy, intr.cx, intr.cy,
                                                node_pos, node_dq, node_w, D, k, unsupported, field, nullptr),
               field ? "TsdfVolume::integrateWarped6Color (k-NN field)" : "TsdfVolume::integrateWarped6Color");
    dfa::device_synchronize();  // (as integrate())
}

dfa::DeviceArray<RGB> TsdfVolume::sampleColors(const float* vertices, int N, int stride, const Affine3f& frame_pose,
                                               float lattice_offset) const {
    if (colors_.empty()) throw dfa::Error(DFA_ERR_INVALID, "TsdfVolume::sampleColors: the volume has no colours (createColors)");
    dfa::DeviceArray<RGB> out((size_t)N);
    float to_volume[12];
    (cfg_.pose.inv() * frame_pose).to12(to_volume);
    const Vec3f vsz = getVoxelSize();
    for (int a = 0; a < 3; ++a) to_volume[9 + a] -= lattice_offset * vsz[a];  // onto the lattice of the sweeps
    dfa::check(dfa_color_sample(colors_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, vertices, stride, N, to_volume,
                                (uint8_t*)out.ptr(), nullptr),
               "TsdfVolume::sampleColors");
    return out;
}

// ---- the k-NN field
bool TsdfVolume::buildKnnField(const float* node_pos, const float* node_w, int D, int k, const Affine3f* node_frame_pose, size_t max_bytes) {
    KnnFieldState f;
    f.dims = cfg_.dims, f.voxel = getVoxelSize(), f.k = k, f.has_frame = node_frame_pose != nullptr;
    if (node_frame_pose) (node_frame_pose->inv() * cfg_.pose).to12(f.vol2node);  // as integrateWarped6 forms it
    dfa_knn_field* h = nullptr;
    dfa::check(dfa_knn_field_create(f.dims[0], f.dims[1], f.dims[2], f.voxel.v, k, f.has_frame ? f.vol2node : nullptr, max_bytes, &h),
               "TsdfVolume::buildKnnField");
    f.handle.reset(h, dfa_knn_field_destroy);
    field_ = KnnFieldState();
    const int rc = dfa_knn_field_build(h, node_pos, node_w, D, nullptr);
    if (rc == DFA_ERR_CAPACITY) return false;  // (the field is dropped: the integrations search)
    dfa::check(rc, "TsdfVolume::buildKnnField");
    field_ = f;
    return true;
}

bool TsdfVolume::appendKnnField(const float* node_pos, const float* node_w, int D_new) {
    if (!field_.handle) throw dfa::Error(DFA_ERR_INVALID, "TsdfVolume::appendKnnField: the volume has no k-NN field");
    const int rc = dfa_knn_field_append(field_.handle.get(), node_pos, node_w, D_new, nullptr);
    if (rc == DFA_ERR_CAPACITY) return dropKnnField(), false;
    dfa::check(rc, "TsdfVolume::appendKnnField");
    return true;
}

int TsdfVolume::knnFieldNodes() const {
    if (!field_.handle) return 0;
    dfa_knn_field_desc d;
    dfa::check(dfa_knn_field_info(field_.handle.get(), &d), "TsdfVolume::knnFieldNodes");
    return d.D;
}

const dfa_knn_field* TsdfVolume::matchingField(int k, int D, const float* vol2node) const {
    const KnnFieldState& f = field_;
    const Vec3f vsz        = getVoxelSize();
    if (!f.handle || f.k != k || f.has_frame != (vol2node != nullptr) || knnFieldNodes() != D) return nullptr;
    if (std::memcmp(f.dims.v, cfg_.dims.v, sizeof(f.dims.v)) != 0 || std::memcmp(f.voxel.v, vsz.v, sizeof(vsz.v)) != 0) return nullptr;
    if (vol2node && std::memcmp(f.vol2node, vol2node, sizeof(f.vol2node)) != 0) return nullptr;
    return f.handle.get();
}

void TsdfVolume::copyVoxelsFrom(const TsdfVolume& src) {
    if (src.cfg_.dims[0] != cfg_.dims[0] || src.cfg_.dims[1] != cfg_.dims[1] || src.cfg_.dims[2] != cfg_.dims[2])
        throw dfa::Error(DFA_ERR_INVALID, "TsdfVolume::copyVoxelsFrom: the volumes differ in their dimensions");
    const bool with_map = src.mapTrusted();
    if (hipMemcpy(blob_.ptr<void>(), src.blob_.ptr<void>(), blob_.sizeBytes(), hipMemcpyDeviceToDevice) != hipSuccess ||
        (with_map && hipMemcpy(occ_.ptr<void>(), src.occ_.ptr<void>(), occ_.sizeBytes(), hipMemcpyDeviceToDevice) != hipSuccess))
        throw dfa::Error(DFA_ERR_HIP, "TsdfVolume::copyVoxelsFrom: hipMemcpy");
    occ_known_ = with_map && soleOwner();
}

void TsdfVolume::clearAndIntegrate(const Dists& dists, const Affine3f& camera_pose, const Intr& intr) {
    Affine3f vol2cam = camera_pose.inv() * cfg_.pose;
    float aff[12];
    vol2cam.to12(aff);
    const Vec3f vsz = getVoxelSize();
    // (a map that describes the volume: boxes of zeros that stay zeros are not written again)
    dfa::check((mapTrusted() ? dfa_tsdf_clear_integrate_known_occ : dfa_tsdf_clear_integrate_occ)(
                   dists.ptr(), (int)dists.step(), dists.cols(), dists.rows(), blob_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1],
                   cfg_.dims[2], vsz.v, cfg_.trunc, cfg_.max_weight, aff, intr.fx, intr.fy, intr.cx, intr.cy, occ_.ptr<uint8_t>(), nullptr),
               "TsdfVolume::clearAndIntegrate");
    occ_known_ = soleOwner();  // (the fused sweep leaves volume and map describing each other — while nobody else can write)
    dfa::device_synchronize();
}

void TsdfVolume::raycast(const Affine3f& camera_pose, const Intr& intr, Depth& depth, Normals& normals) {  // :95-110
    Affine3f cam2vol = cfg_.pose.inv() * camera_pose;
    float aff[12], rinv[9];
    cam2vol.to12(aff);
    cam2vol.inverse_rotation(rinv);
    const Vec3f vsz = getVoxelSize();
    dfa::check(dfa_tsdf_raycast_depth(blob_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, cfg_.trunc, aff, rinv,
                                      intr.fx, intr.fy, intr.cx, intr.cy, cfg_.ray_step, cfg_.grad_delta,
                                      depth.ptr(), (int)depth.step(), (float*)normals.ptr(), (int)normals.step(),
                                      depth.cols(), depth.rows(), nullptr),
               "TsdfVolume::raycast(depth)");
}

void TsdfVolume::raycast(const Affine3f& camera_pose, const Intr& intr, Cloud& points, Normals& normals) {  // :112-129
    Affine3f cam2vol = cfg_.pose.inv() * camera_pose;
    float aff[12], rinv[9];
    cam2vol.to12(aff);
    cam2vol.inverse_rotation(rinv);
    const Vec3f vsz = getVoxelSize();
    dfa::check(dfa_tsdf_raycast_points(blob_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, cfg_.trunc, aff,
                                       rinv, intr.fx, intr.fy, intr.cx, intr.cy, cfg_.ray_step,
                                       cfg_.grad_delta, (float*)points.ptr(), (int)points.step(),
                                       (float*)normals.ptr(), (int)normals.step(), points.cols(), points.rows(),
                                       nullptr),
               "TsdfVolume::raycast(points)");
}

void TsdfVolume::raycastRender(const Affine3f& camera_pose, const Intr& intr, int cols, int rows, const Vec3f& light_pose, int mode,
                               Image& image) const {
    if (image.rows() != rows || image.cols() != cols * (mode == DFA_RENDER_BOTH ? 2 : 1))
        throw dfa::Error(DFA_ERR_INVALID, "TsdfVolume::raycastRender: image size does not fit the mode");
    Affine3f cam2vol = cfg_.pose.inv() * camera_pose;
    float aff[12], rinv[9];
    cam2vol.to12(aff);
    cam2vol.inverse_rotation(rinv);
    const Vec3f vsz = getVoxelSize();
    dfa::check(dfa_tsdf_raycast_render(blob_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, cfg_.trunc, aff, rinv,
                                       intr.fx, intr.fy, intr.cx, intr.cy, cfg_.ray_step, cfg_.grad_delta, cols, rows,
                                       light_pose.v, mode, (uint8_t*)image.ptr(), (int)image.step(), nullptr),
               "TsdfVolume::raycastRender");
}

dfa::DeviceArray<Point> TsdfVolume::fetchCloud(dfa::DeviceArray<Point>& cloud_buffer) const {  // :131-147
    enum { DEFAULT_CLOUD_BUFFER_SIZE = 10 * 1000 * 1000 };
    if (cloud_buffer.empty()) cloud_buffer.create(DEFAULT_CLOUD_BUFFER_SIZE);
    float aff[12];
    cfg_.pose.to12(aff);
    const Vec3f vsz       = getVoxelSize();
    const int cap         = (int)std::min<size_t>(cloud_buffer.size(), 0x7fffffff);
    const uint8_t* occ    = occupancy();
    dfa::DeviceArray<int> total(1);
    if (occ)
        dfa::check(dfa_tsdf_extract_cloud_occ(blob_.ptr<uint32_t>(), occ, cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, aff,
                                              (float*)cloud_buffer.ptr(), cap, total.ptr(), nullptr),
                   "TsdfVolume::fetchCloud");
    else
        dfa::check(dfa_tsdf_extract_cloud(blob_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, aff,
                                          (float*)cloud_buffer.ptr(), cap, total.ptr(), nullptr),
                   "TsdfVolume::fetchCloud");
    int n = 0;
    total.DeviceMemory::download(&n, sizeof(n));  // (the reference's extractCloud synchronises the device and reads its counter back)
    return dfa::DeviceArray<Point>(cloud_buffer.ptr(), (size_t)std::min(n, cap));
}

void TsdfVolume::fetchNormals(const dfa::DeviceArray<Point>& cloud, dfa::DeviceArray<Normal>& normals) const {  // :149-160
    normals.create(cloud.size());
    float aff[12], rinv[9];
    cfg_.pose.to12(aff);
    cfg_.pose.inverse_rotation(rinv);
    const Vec3f vsz = getVoxelSize();
    dfa::check(dfa_tsdf_extract_normals(blob_.ptr<uint32_t>(), cfg_.dims[0], cfg_.dims[1], cfg_.dims[2], vsz.v, aff, rinv,
                                        cfg_.grad_delta, (const float*)cloud.ptr(), (int)cloud.size(), (float*)normals.ptr(),
                                        nullptr),
               "TsdfVolume::fetchNormals");
    dfa::device_synchronize();  // (the reference's extractNormals synchronises the device, tsdf_volume.cu:719)
}
