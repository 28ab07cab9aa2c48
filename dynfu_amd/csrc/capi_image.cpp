// capi_image.cpp — C ABI (include/dynfu_amd.h), the image seams: shading, the mesh rasteriser, the visibility of a cloud
// against a model map, the depth filters and resizes, vertex / normal maps and the rigid-ICP sums.  Argument checks and
// launcher calls only (capi_internal.hpp); the kernels are in render.hip, raster.hip, visibility.hip, img.hip and icp.hip.
#include "capi_internal.hpp"

using namespace dfa::capi;
using dfa::DeviceBuffer;
using dfa::stream_scratch;

namespace {
struct IcpScratch : DeviceBuffer<float> {};        // partial sums of dfa_icp_sums
struct VisScratch : DeviceBuffer<int32_t> {};      // per-workgroup counts of dfa_visible_vertices
struct RigidLoopScratch : DeviceBuffer<float> {};  // dfa_rigid_align_cloud: the state of the call, then its partial sums
}  // namespace

extern "C" {

// -------------------------------------------------------------------- render seam

int dfa_render_image_points(const float* points, int points_step, const float* normals, int normals_step, int cols, int rows,
                            const float light_pose[3], uint8_t* image, int image_step, dfa_stream_t stream) {
    REQUIRE(points && normals && image, "null image");
    REQUIRE(cols > 0 && rows > 0, "non-positive image size");
    REQUIRE(points_step >= cols * 16 && normals_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE(image_step >= cols * 4, "row step smaller than a pixel row");
    REQUIRE(light_pose, "null light pose");
    REQUIRE((((uintptr_t)points | (uintptr_t)normals | (uintptr_t)points_step | (uintptr_t)normals_step) & 15) == 0,
            "points / normals rows must be 16-byte aligned");
    REQUIRE((((uintptr_t)image | (uintptr_t)image_step) & 3) == 0, "image rows must be 4-byte aligned");
    HIP_TRY(dfa::launch_render_points(points, points_step, normals, normals_step, cols, rows, light_pose, image, image_step,
                                      S(stream)));
    return DFA_OK;
}

int dfa_render_image_depth(const uint16_t* depth, int depth_step, const float* normals, int normals_step, int cols, int rows,
                           float fx, float fy, float cx, float cy, const float light_pose[3], uint8_t* image, int image_step,
                           dfa_stream_t stream) {
    REQUIRE(depth && normals && image, "null image");
    REQUIRE(cols > 0 && rows > 0, "non-positive image size");
    REQUIRE(depth_step >= cols * 2 && normals_step >= cols * 16, "row step smaller than a row");
    REQUIRE(image_step >= cols * 4, "row step smaller than a pixel row");
    REQUIRE(light_pose, "null light pose");
    REQUIRE((((uintptr_t)depth | (uintptr_t)depth_step) & 1) == 0, "depth rows must be 2-byte aligned");
    REQUIRE((((uintptr_t)normals | (uintptr_t)normals_step) & 15) == 0, "normals rows must be 16-byte aligned");
    REQUIRE((((uintptr_t)image | (uintptr_t)image_step) & 3) == 0, "image rows must be 4-byte aligned");
    HIP_TRY(dfa::launch_render_depth(depth, depth_step, normals, normals_step, cols, rows, fx, fy, cx, cy, light_pose, image,
                                     image_step, S(stream)));
    return DFA_OK;
}

int dfa_render_tangent_colors(const float* normals, int normals_step, int cols, int rows, uint8_t* image, int image_step,
                              dfa_stream_t stream) {
    REQUIRE(normals && image, "null image");
    REQUIRE(cols > 0 && rows > 0, "non-positive image size");
    REQUIRE(normals_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE(image_step >= cols * 4, "row step smaller than a pixel row");
    REQUIRE((((uintptr_t)normals | (uintptr_t)normals_step) & 15) == 0, "normals rows must be 16-byte aligned");
    REQUIRE((((uintptr_t)image | (uintptr_t)image_step) & 3) == 0, "image rows must be 4-byte aligned");
    HIP_TRY(dfa::launch_tangent_colors(normals, normals_step, cols, rows, image, image_step, S(stream)));
    return DFA_OK;
}

int dfa_mesh_rasterize(const float* vertices, const float* normals, int N, const int32_t* indices, int T,
                       const float world2cam[12], float fx, float fy, float cx, float cy, float z_near, int cols, int rows,
                       uint64_t* zbuffer, float* points, int points_step, float* out_normals, int normals_step,
                       dfa_stream_t stream) {
    REQUIRE(zbuffer, "null z-buffer");
    REQUIRE(cols > 0 && rows > 0, "non-positive image size");
    REQUIRE(cols <= 8192 && rows <= 8192, "image larger than 8192 pixels a side");
    REQUIRE(z_near > 0.f, "z_near must be positive");
    REQUIRE(N >= 0 && T >= 0 && T <= 0x7fffffff / 3, "bad mesh size");
    REQUIRE(T == 0 || (vertices && indices && N > 0), "null mesh");
    REQUIRE(!points || points_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE(!out_normals || normals_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE((((uintptr_t)vertices | (uintptr_t)normals) & 15) == 0, "vertices / normals must be 16-byte aligned");
    REQUIRE(((uintptr_t)zbuffer & 7) == 0, "z-buffer must be 8-byte aligned");
    REQUIRE(!points || (((uintptr_t)points | (uintptr_t)points_step) & 15) == 0, "point rows must be 16-byte aligned");
    REQUIRE(!out_normals || (((uintptr_t)out_normals | (uintptr_t)normals_step) & 15) == 0, "normal rows must be 16-byte aligned");
    HIP_TRY(dfa::launch_mesh_rasterize(vertices, normals, N, indices, T, world2cam, fx, fy, cx, cy, z_near, cols, rows, zbuffer,
                                       points, points_step, out_normals, normals_step, S(stream)));
    return DFA_OK;
}

int dfa_visible_vertices(const float* vertices, int stride, int N, const float* model_points, int points_step, int cols, int rows,
                         float fx, float fy, float cx, float cy, float z_tol, uint8_t* flags, int32_t* count,
                         dfa_stream_t stream) {
    REQUIRE(N >= 0, "negative vertex count");
    REQUIRE(stride == 3 || stride == 4, "stride must be 3 or 4 floats");
    REQUIRE(N == 0 || (vertices && flags), "null vertices / flags");
    REQUIRE(model_points, "null model map");
    REQUIRE(cols > 0 && rows > 0, "non-positive image size");
    REQUIRE(points_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE((((uintptr_t)model_points | (uintptr_t)points_step) & 3) == 0, "model map rows must be 4-byte aligned");
    int32_t* partial = nullptr;
    if (count && N > 0) {
        VisScratch& scratch = stream_scratch<VisScratch>(S(stream));
        HIP_TRY(scratch.reserve((size_t)dfa::visible_blocks(N)));
        partial = scratch.data;
    }
    HIP_TRY(dfa::launch_visible_vertices(vertices, stride, N, model_points, points_step, cols, rows, fx, fy, cx, cy, z_tol, flags,
                                         count, partial, S(stream)));
    return DFA_OK;
}

// -------------------------------------------------------------------- depth pre-processing seam

int dfa_depth_bilateral_filter(const uint16_t* src, int src_step, uint16_t* dst, int dst_step, int cols, int rows,
                               int kernel_size, float sigma_spatial, float sigma_depth, dfa_stream_t stream) {
    REQUIRE(src && dst && cols > 0 && rows > 0, "bad images");
    REQUIRE(src != dst, "the bilateral filter cannot run in place");
    REQUIRE(src_step >= cols * 2 && dst_step >= cols * 2, "row step smaller than a row");
    REQUIRE(kernel_size >= 1 && sigma_spatial > 0.f && sigma_depth > 0.f, "bad filter parameters");
    HIP_TRY(dfa::launch_bilateral(src, src_step, dst, dst_step, cols, rows, kernel_size, sigma_spatial, sigma_depth,
                                  S(stream)));
    return DFA_OK;
}

int dfa_depth_truncate(uint16_t* depth, int depth_step, int cols, int rows, float max_dist, dfa_stream_t stream) {
    REQUIRE(depth && cols > 0 && rows > 0 && depth_step >= cols * 2, "bad image");
    REQUIRE(max_dist >= 0.f && max_dist < 65.536f, "max_dist out of the 16-bit millimetre range");
    HIP_TRY(dfa::launch_truncate_depth(depth, depth_step, cols, rows, max_dist, S(stream)));
    return DFA_OK;
}

int dfa_depth_build_pyramid(const uint16_t* src, int src_step, int cols, int rows, uint16_t* dst, int dst_step,
                            float sigma_depth, dfa_stream_t stream) {
    REQUIRE(src && cols > 0 && rows > 0, "bad images");
    if (cols / 2 == 0 || rows / 2 == 0) return DFA_OK;  // empty output
    REQUIRE(dst, "null output");
    REQUIRE(src_step >= cols * 2 && dst_step >= (cols / 2) * 2, "row step smaller than a row");
    HIP_TRY(dfa::launch_depth_pyr(src, src_step, cols, rows, dst, dst_step, sigma_depth, S(stream)));
    return DFA_OK;
}

int dfa_compute_normals_mask_depth(uint16_t* depth, int depth_step, int cols, int rows, float fx, float fy, float cx,
                                   float cy, float* normals, int normals_step, dfa_stream_t stream) {
    REQUIRE(depth && normals && cols > 0 && rows > 0, "bad images");
    REQUIRE(depth_step >= cols * 2 && normals_step >= cols * 16, "row step smaller than a row");
    REQUIRE(fx != 0.f && fy != 0.f, "zero focal length");
    HIP_TRY(dfa::launch_normals_mask_depth(depth, depth_step, cols, rows, fx, fy, cx, cy, normals, normals_step, S(stream)));
    return DFA_OK;
}

int dfa_resize_depth_normals(const uint16_t* depth, int depth_step, const float* normals, int normals_step, int cols,
                             int rows, uint16_t* depth_out, int depth_out_step, float* normals_out, int normals_out_step,
                             dfa_stream_t stream) {
    REQUIRE(depth && normals && cols > 0 && rows > 0, "bad images");
    if (cols / 2 == 0 || rows / 2 == 0) return DFA_OK;  // empty output
    REQUIRE(depth_out && normals_out, "null output");
    REQUIRE(depth_step >= cols * 2 && normals_step >= cols * 16, "row step smaller than a row");
    REQUIRE(depth_out_step >= (cols / 2) * 2 && normals_out_step >= (cols / 2) * 16, "output row step smaller than a row");
    HIP_TRY(dfa::launch_resize_depth_normals(depth, depth_step, normals, normals_step, cols, rows, depth_out, depth_out_step,
                                             normals_out, normals_out_step, S(stream)));
    return DFA_OK;
}

int dfa_resize_points_normals(const float* points, int points_step, const float* normals, int normals_step, int cols,
                              int rows, float* points_out, int points_out_step, float* normals_out, int normals_out_step,
                              dfa_stream_t stream) {
    REQUIRE(points && normals && cols > 0 && rows > 0, "bad images");
    if (cols / 2 == 0 || rows / 2 == 0) return DFA_OK;  // empty output
    REQUIRE(points_out && normals_out, "null output");
    REQUIRE(points_step >= cols * 16 && normals_step >= cols * 16, "row step smaller than a row");
    REQUIRE(points_out_step >= (cols / 2) * 16 && normals_out_step >= (cols / 2) * 16, "output row step smaller than a row");
    HIP_TRY(dfa::launch_resize_points_normals(points, points_step, normals, normals_step, cols, rows, points_out,
                                              points_out_step, normals_out, normals_out_step, S(stream)));
    return DFA_OK;
}

// ------------------------------------------------------------------------------ rigid-ICP seam

int dfa_icp_sums(int depth_variant, const void* curr, int curr_step, const float* ncurr, int ncurr_step, const void* prev,
                 int prev_step, const float* nprev, int nprev_step, int cols, int rows, const float aff[12], float fx,
                 float fy, float cx, float cy, float dist_thres, float angle_thres, float* sums27, unsigned int* matched,
                 dfa_stream_t stream) {
    REQUIRE(curr && ncurr && prev && nprev && sums27 && aff, "null argument");
    REQUIRE(cols > 0 && rows > 0, "bad image size");
    const int px = depth_variant ? 2 : 16;
    REQUIRE(curr_step >= cols * px && prev_step >= cols * px && ncurr_step >= cols * 16 && nprev_step >= cols * 16,
            "row step smaller than a row");
    REQUIRE(fx != 0.f && fy != 0.f && dist_thres >= 0.f, "bad intrinsics / threshold");
    IcpScratch& partial = stream_scratch<IcpScratch>(S(stream));
    HIP_TRY(partial.reserve(dfa::icp_partial_floats(cols, rows)));
    HIP_TRY(dfa::launch_icp_sums(depth_variant != 0, curr, curr_step, ncurr, ncurr_step, prev, prev_step, nprev, nprev_step,
                                 cols, rows, aff, fx, fy, cx, cy, dist_thres, angle_thres, partial.data, sums27,
                                 matched, S(stream)));
    return DFA_OK;
}

int dfa_rigid_sums_cloud(const float* vertices, const float* normals, int stride, int N, const float aff[12],
                         const float* live_vertex_map, int vertex_step, const float* live_normal_map, int normal_step,
                         int cols, int rows, float fx, float fy, float cx, float cy, float dist_thresh, float cos_thresh,
                         float* sums27, unsigned int* matched, dfa_stream_t stream) {
    REQUIRE(N >= 0, "negative vertex count");
    REQUIRE(stride == 3 || stride == 4, "stride must be 3 or 4 floats");
    REQUIRE(N == 0 || vertices, "null vertices");
    REQUIRE(aff && live_vertex_map && live_normal_map && sums27, "null argument");
    REQUIRE(cols > 0 && rows > 0, "bad image size");
    REQUIRE(vertex_step >= cols * 16 && normal_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE((((uintptr_t)live_vertex_map | (uintptr_t)live_normal_map | (uintptr_t)vertex_step | (uintptr_t)normal_step) & 15) == 0,
            "map rows must be 16-byte aligned");
    REQUIRE((((uintptr_t)vertices | (uintptr_t)normals) & 3) == 0, "vertices / normals must be 4-byte aligned");
    REQUIRE(fx != 0.f && fy != 0.f && dist_thresh >= 0.f, "bad intrinsics / threshold");
    IcpScratch& partial = stream_scratch<IcpScratch>(S(stream));
    if (N > 0) HIP_TRY(partial.reserve(dfa::rigid_cloud_partial_floats(N)));
    HIP_TRY(dfa::launch_rigid_sums_cloud(vertices, normals, stride, N, aff, live_vertex_map, vertex_step, live_normal_map,
                                         normal_step, cols, rows, fx, fy, cx, cy, dist_thresh, cos_thresh, partial.data, sums27,
                                         matched, S(stream)));
    return DFA_OK;
}

int dfa_rigid_align_cloud(const float* vertices, const float* normals, int stride, int N, const float aff0[12],
                          const float* live_vertex_map, int vertex_step, const float* live_normal_map, int normal_step,
                          int cols, int rows, float fx, float fy, float cx, float cy, float dist_thresh, float cos_thresh,
                          const int* level_step, const int* level_iters, int levels, float stop_rot, float stop_trans,
                          dfa_rigid_align_report* report, float* trace, dfa_stream_t stream) {
    REQUIRE(N >= 0, "negative vertex count");
    REQUIRE(stride == 3 || stride == 4, "stride must be 3 or 4 floats");
    REQUIRE(N == 0 || vertices, "null vertices");
    REQUIRE(aff0 && live_vertex_map && live_normal_map && report, "null argument");
    REQUIRE(cols > 0 && rows > 0, "bad image size");
    REQUIRE(vertex_step >= cols * 16 && normal_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE((((uintptr_t)live_vertex_map | (uintptr_t)live_normal_map | (uintptr_t)vertex_step | (uintptr_t)normal_step) & 15) == 0,
            "map rows must be 16-byte aligned");
    REQUIRE((((uintptr_t)vertices | (uintptr_t)normals | (uintptr_t)report | (uintptr_t)trace) & 3) == 0,
            "vertices / normals / report / trace must be 4-byte aligned");
    REQUIRE(fx != 0.f && fy != 0.f && dist_thresh >= 0.f, "bad intrinsics / threshold");
    REQUIRE(level_step && level_iters && levels >= 1 && levels <= 4, "the schedule has 1 to 4 levels");
    int total = 0;
    for (int l = 0; l < levels; ++l) {
        REQUIRE(level_step[l] >= 1, "a level's step must be at least 1");
        REQUIRE(level_iters[l] >= 0 && level_iters[l] <= 64, "a level's iterations must be 0 to 64");
        total += level_iters[l];
    }
    REQUIRE(total <= 64, "more than 64 iterations in all");
    REQUIRE(stop_rot >= 0.f && stop_trans >= 0.f, "negative or NaN stop threshold");
    RigidLoopScratch& scratch = stream_scratch<RigidLoopScratch>(S(stream));
    HIP_TRY(scratch.reserve(dfa::rigid_align_scratch_floats(N, level_step, levels)));
    HIP_TRY(dfa::launch_rigid_align_cloud(vertices, normals, stride, N, aff0, live_vertex_map, vertex_step, live_normal_map,
                                          normal_step, cols, rows, fx, fy, cx, cy, dist_thresh, cos_thresh, level_step,
                                          level_iters, levels, stop_rot, stop_trans, report, trace, scratch.data, S(stream)));
    return DFA_OK;
}

// ------------------------------------------------------------------------ vertex / normal maps

int dfa_compute_points_normals(const uint16_t* depth, int depth_step, int cols, int rows, float fx, float fy, float cx,
                               float cy, float* points, int points_step, float* normals, int normals_step,
                               dfa_stream_t stream) {
    REQUIRE(depth && points && normals && cols > 0 && rows > 0, "bad images");
    REQUIRE(depth_step >= cols * 2 && points_step >= cols * 16 && normals_step >= cols * 16, "row step smaller than a row");
    REQUIRE(fx != 0.f && fy != 0.f, "zero focal length");
    HIP_TRY(dfa::launch_points_normals(depth, depth_step, cols, rows, fx, fy, cx, cy, points, points_step, normals,
                                       normals_step, S(stream)));
    return DFA_OK;
}

}  // extern "C"
