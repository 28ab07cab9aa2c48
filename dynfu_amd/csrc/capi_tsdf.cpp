// capi_tsdf.cpp — C ABI (include/dynfu_amd.h), the volume's seams: TSDF clear / integrate / raycast, the warped
// integrations, marching cubes and the point-cloud extraction, with the scratch each keeps per stream.  Argument checks
// and launcher calls only (capi_internal.hpp); the kernels are in tsdf.hip, tsdf_warped.hip, mc.hip and extract.hip.
#include "capi_internal.hpp"

using namespace dfa::capi;
using dfa::DeviceBuffer;
using dfa::stream_scratch;

namespace {

// scratch of dfa_marching_cubes and of the point-cloud extraction (segment offsets + scan partials)
struct McScratch {
    DeviceBuffer<int32_t> seg_off, chunk_sums;
    hipError_t reserve(long nsegs) {
        const hipError_t e = seg_off.reserve((size_t)nsegs + 1);
        return e != hipSuccess ? e : chunk_sums.reserve((size_t)dfa::mc_scan_chunks(nsegs));
    }
};
// scratch of dfa_marching_cubes_indexed: two offset arrays (vertices, indices) over its own segments, one set of partials
struct McIndexedScratch {
    McScratch vert;
    DeviceBuffer<int32_t> idx_off;
    hipError_t reserve(long nsegs) {
        const hipError_t e = vert.reserve(nsegs);
        return e != hipSuccess ? e : idx_off.reserve((size_t)nsegs + 1);
    }
};
}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------- TSDF seam

int dfa_compute_dists(const uint16_t* depth, int depth_step, uint16_t* dists, int dists_step, int cols, int rows,
                      float fx, float fy, float cx, float cy, dfa_stream_t stream) {
    REQUIRE(depth && dists, "null image");
    REQUIRE(cols > 0 && rows > 0, "empty image");
    REQUIRE(depth_step >= cols * 2 && dists_step >= cols * 2, "row step smaller than a row");
    REQUIRE(fx != 0.f && fy != 0.f, "zero focal length");
    HIP_TRY(dfa::launch_compute_dists(depth, depth_step, dists, dists_step, cols, rows, fx, fy, cx, cy, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_clear(uint32_t* volume, int X, int Y, int Z, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    HIP_TRY(dfa::launch_tsdf_clear(volume, X, Y, Z, S(stream)));
    return DFA_OK;
}

size_t dfa_tsdf_occupancy_bytes(int X, int Y, int Z) {
    return X > 0 && Y > 0 && Z > 0 ? dfa::occ_dims(X, Y, Z).bytes() : 0;
}

int dfa_tsdf_clear_occ(uint32_t* volume, int X, int Y, int Z, uint8_t* occupancy, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(occupancy, "null occupancy map");
    HIP_TRY(dfa::launch_tsdf_clear(volume, X, Y, Z, S(stream)));
    HIP_TRY(hipMemsetAsync(occupancy, 0, dfa::occ_dims(X, Y, Z).bytes(), S(stream)));
    return DFA_OK;
}

static int integrate_common(bool fused, const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume,
                            int X, int Y, int Z, const float voxel_size[3], float trunc_dist, int max_weight,
                            const float vol2cam[12], float fx, float fy, float cx, float cy, uint8_t* occupancy,
                            dfa_stream_t stream, bool occupancy_known = false) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(dists && cols > 0 && rows > 0 && dists_step >= cols * 2, "bad dists image");
    REQUIRE(voxel_size && vol2cam, "null parameter block");
    REQUIRE(trunc_dist > 0.f, "trunc_dist must be positive");
    REQUIRE(max_weight >= 0 && max_weight <= 65535, "max_weight must fit the 16-bit weight");
    HIP_TRY(dfa::launch_tsdf_integrate(fused, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, trunc_dist,
                                       max_weight, vol2cam, fx, fy, cx, cy, occupancy, occupancy_known, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_integrate_occ(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                           const float voxel_size[3], float trunc_dist, int max_weight, const float vol2cam[12], float fx,
                           float fy, float cx, float cy, uint8_t* occupancy, dfa_stream_t stream) {
    REQUIRE(occupancy, "null occupancy map");
    return integrate_common(false, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, trunc_dist, max_weight, vol2cam,
                            fx, fy, cx, cy, occupancy, stream);
}

int dfa_tsdf_clear_integrate_occ(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y,
                                 int Z, const float voxel_size[3], float trunc_dist, int max_weight,
                                 const float vol2cam[12], float fx, float fy, float cx, float cy, uint8_t* occupancy,
                                 dfa_stream_t stream) {
    REQUIRE(occupancy, "null occupancy map");
    return integrate_common(true, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, trunc_dist, max_weight, vol2cam,
                            fx, fy, cx, cy, occupancy, stream);
}

int dfa_tsdf_clear_integrate_known_occ(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X,
                                       int Y, int Z, const float voxel_size[3], float trunc_dist, int max_weight,
                                       const float vol2cam[12], float fx, float fy, float cx, float cy, uint8_t* occupancy,
                                       dfa_stream_t stream) {
    REQUIRE(occupancy, "null occupancy map");
    return integrate_common(true, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, trunc_dist, max_weight, vol2cam,
                            fx, fy, cx, cy, occupancy, stream, true);
}

int dfa_tsdf_integrate(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                       const float voxel_size[3], float trunc_dist, int max_weight, const float vol2cam[12], float fx,
                       float fy, float cx, float cy, dfa_stream_t stream) {
    return integrate_common(false, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, trunc_dist, max_weight,
                            vol2cam, fx, fy, cx, cy, nullptr, stream);
}

int dfa_tsdf_clear_integrate(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y,
                             int Z, const float voxel_size[3], float trunc_dist, int max_weight,
                             const float vol2cam[12], float fx, float fy, float cx, float cy, dfa_stream_t stream) {
    return integrate_common(true, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, trunc_dist, max_weight,
                            vol2cam, fx, fy, cx, cy, nullptr, stream);
}

int dfa_tsdf_vertex_normals(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3],
                            float gradient_delta_factor, const float* points, int n, float* normals,
                            dfa_stream_t stream) {
    REQUIRE(volume && voxel_size, "null volume / voxel_size");
    REQUIRE(X > 1 && Y > 1 && Z > 1, "the volume needs two voxels per axis");
    REQUIRE(n >= 0 && (n == 0 || (points && normals)), "null points / normals");
    REQUIRE(voxel_size[0] > 0.f && voxel_size[1] > 0.f && voxel_size[2] > 0.f && gradient_delta_factor > 0.f,
            "voxel size and gradient delta must be positive");
    REQUIRE((((uintptr_t)points | (uintptr_t)normals) & 15) == 0, "points / normals must be 16-byte aligned");
    HIP_TRY(dfa::launch_vertex_normals(volume, X, Y, Z, voxel_size, gradient_delta_factor, points, n, normals, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_raycast_points(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                            const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                            float step_factor, float delta_factor, float* points, int points_step, float* normals,
                            int normals_step, int cols, int rows, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(X >= 2 && Y >= 2 && Z >= 2, "volume needs at least 2 voxels per axis");
    REQUIRE(points && normals && cols > 0 && rows > 0, "bad output images");
    REQUIRE(points_step >= cols * 16 && normals_step >= cols * 16, "row step smaller than a float4 row");
    REQUIRE(voxel_size && cam2vol && Rinv, "null parameter block");
    REQUIRE(trunc_dist > 0.f && step_factor > 0.f, "non-positive ray step");
    HIP_TRY(dfa::launch_raycast_points(volume, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy,
                                       step_factor, delta_factor, points, points_step, normals, normals_step, cols,
                                       rows, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_raycast_depth(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                           const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                           float step_factor, float delta_factor, uint16_t* depth, int depth_step, float* normals,
                           int normals_step, int cols, int rows, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(X >= 2 && Y >= 2 && Z >= 2, "volume needs at least 2 voxels per axis");
    REQUIRE(depth && normals && cols > 0 && rows > 0, "bad output images");
    REQUIRE(depth_step >= cols * 2 && normals_step >= cols * 16, "row step smaller than a row");
    REQUIRE(voxel_size && cam2vol && Rinv, "null parameter block");
    REQUIRE(trunc_dist > 0.f && step_factor > 0.f, "non-positive ray step");
    HIP_TRY(dfa::launch_raycast_depth(volume, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy,
                                      step_factor, delta_factor, depth, depth_step, normals, normals_step, cols, rows,
                                      S(stream)));
    return DFA_OK;
}

int dfa_tsdf_raycast_tally(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                           const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                           float step_factor, float delta_factor, int cols, int rows, uint64_t* counts,
                           uint32_t* touched_bits, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(X >= 2 && Y >= 2 && Z >= 2, "volume needs at least 2 voxels per axis");
    REQUIRE(counts && cols > 0 && rows > 0, "bad counters / image size");
    REQUIRE(voxel_size && cam2vol && Rinv, "null parameter block");
    REQUIRE(trunc_dist > 0.f && step_factor > 0.f, "non-positive ray step");
    HIP_TRY(hipMemsetAsync(counts, 0, 4 * sizeof(uint64_t), S(stream)));
    HIP_TRY(dfa::launch_raycast_tally(volume, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy, step_factor,
                                      delta_factor, cols, rows, (unsigned long long*)counts, touched_bits, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_raycast_render(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                            const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                            float step_factor, float delta_factor, int cols, int rows, const float light_pose[3], int mode,
                            uint8_t* image, int image_step, dfa_stream_t stream) {
    REQUIRE(image, "null image");
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(X >= 2 && Y >= 2 && Z >= 2, "volume needs at least 2 voxels per axis");
    REQUIRE(cols > 0 && rows > 0, "non-positive image size");
    REQUIRE(mode == DFA_RENDER_PHONG || mode == DFA_RENDER_NORMALS || mode == DFA_RENDER_BOTH, "unknown render mode");
    REQUIRE(cols <= 0x1fffffff / (mode == DFA_RENDER_BOTH ? 2 : 1) && image_step >= cols * 4 * (mode == DFA_RENDER_BOTH ? 2 : 1),
            "row step smaller than a pixel row");
    REQUIRE((((uintptr_t)image | (uintptr_t)image_step) & 3) == 0, "image rows must be 4-byte aligned");
    REQUIRE(voxel_size && cam2vol && Rinv && light_pose, "null parameter block");
    REQUIRE(trunc_dist > 0.f && step_factor > 0.f, "non-positive ray step");
    HIP_TRY(dfa::launch_raycast_render(volume, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy, step_factor,
                                       delta_factor, cols, rows, light_pose, mode, image, image_step, S(stream)));
    return DFA_OK;
}

// ------------------------------------------------------------------------ marching-cubes seam

static int marching_cubes_common(const uint32_t* volume, int X, int Y, int Z, const float cell_size[3],
                                 const int32_t* tri_table, const int32_t* num_verts_table, float* out_points,
                                 int max_vertices, int32_t* total_vertices, const uint8_t* occupancy, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(cell_size && tri_table && num_verts_table, "null parameter block / case tables");
    REQUIRE(max_vertices >= 0 && (max_vertices == 0 || out_points), "bad output buffer");
    REQUIRE((long)X * Y * Z / 64 < (1L << 31), "volume too large");
    const bool vec4  = (X % 4 == 0) && (((uintptr_t)volume & 15) == 0);
    const long nsegs = dfa::mc_segments(X, Y, Z, vec4);
    McScratch& scratch = stream_scratch<McScratch>(S(stream));
    HIP_TRY(scratch.reserve(nsegs));
    HIP_TRY(dfa::launch_marching_cubes(volume, X, Y, Z, cell_size, tri_table, num_verts_table, out_points,
                                       max_vertices, total_vertices, scratch.seg_off.data, scratch.chunk_sums.data,
                                       occupancy, S(stream)));
    return DFA_OK;
}

int dfa_marching_cubes(const uint32_t* volume, int X, int Y, int Z, const float cell_size[3],
                       const int32_t* tri_table, const int32_t* num_verts_table, float* out_points, int max_vertices,
                       int32_t* total_vertices, dfa_stream_t stream) {
    return marching_cubes_common(volume, X, Y, Z, cell_size, tri_table, num_verts_table, out_points, max_vertices,
                                 total_vertices, nullptr, stream);
}

int dfa_marching_cubes_occ(const uint32_t* volume, const uint8_t* occupancy, int X, int Y, int Z, const float cell_size[3],
                           const int32_t* tri_table, const int32_t* num_verts_table, float* out_points, int max_vertices,
                           int32_t* total_vertices, dfa_stream_t stream) {
    REQUIRE(occupancy, "null occupancy map");
    return marching_cubes_common(volume, X, Y, Z, cell_size, tri_table, num_verts_table, out_points, max_vertices,
                                 total_vertices, occupancy, stream);
}

// min_weight 0: the plain call (no floor); fn: the entry point a refusal names
static int marching_cubes_indexed_common(const char* fn, const uint32_t* volume, const uint8_t* occupancy, int X, int Y, int Z,
                                         const float cell_size[3], const int32_t* tri_table, const int32_t* num_verts_table,
                                         int min_weight, float* out_vertices, int max_vertices, int32_t* out_indices,
                                         int max_indices, int32_t* totals, dfa_stream_t stream) {
    REQUIRE_AS(fn, volume && X >= 2 && Y >= 2 && Z >= 2, "bad volume");
    REQUIRE_AS(fn, cell_size && tri_table && num_verts_table, "null parameter block / case tables");
    REQUIRE_AS(fn, max_vertices >= 0 && (max_vertices == 0 || out_vertices), "bad vertex buffer");
    REQUIRE_AS(fn, max_indices >= 0 && (max_indices == 0 || out_indices), "bad index buffer");
    REQUIRE_AS(fn, ((uintptr_t)out_vertices & 15) == 0, "out_vertices must be 16-byte aligned");
    REQUIRE_AS(fn, totals, "null totals");
    REQUIRE_AS(fn, (long)X * Y * Z / 64 < (1L << 31), "volume too large");
    const long nsegs = dfa::mci_segments(X, Y, Z);
    McIndexedScratch& scratch = stream_scratch<McIndexedScratch>(S(stream));
    HIP_TRY(scratch.reserve(nsegs));
    if (min_weight == 0) {
        HIP_TRY(dfa::launch_marching_cubes_indexed(volume, X, Y, Z, cell_size, tri_table, num_verts_table, out_vertices,
                                                   max_vertices, out_indices, max_indices, totals, scratch.vert.seg_off.data,
                                                   scratch.idx_off.data, scratch.vert.chunk_sums.data, occupancy, S(stream)));
    } else {
        HIP_TRY(dfa::launch_marching_cubes_indexed_min_weight(volume, X, Y, Z, cell_size, tri_table, num_verts_table, min_weight,
                                                              out_vertices, max_vertices, out_indices, max_indices, totals,
                                                              scratch.vert.seg_off.data, scratch.idx_off.data,
                                                              scratch.vert.chunk_sums.data, occupancy, S(stream)));
    }
    return DFA_OK;
}

int dfa_marching_cubes_indexed(const uint32_t* volume, const uint8_t* occupancy, int X, int Y, int Z, const float cell_size[3],
                               const int32_t* tri_table, const int32_t* num_verts_table, float* out_vertices,
                               int max_vertices, int32_t* out_indices, int max_indices, int32_t* totals,
                               dfa_stream_t stream) {
    return marching_cubes_indexed_common(__func__, volume, occupancy, X, Y, Z, cell_size, tri_table, num_verts_table, 0, out_vertices,
                                         max_vertices, out_indices, max_indices, totals, stream);
}

int dfa_marching_cubes_indexed_min_weight(const uint32_t* volume, const uint8_t* occupancy, int X, int Y, int Z,
                                          const float cell_size[3], const int32_t* tri_table, const int32_t* num_verts_table,
                                          int min_weight, float* out_vertices, int max_vertices, int32_t* out_indices,
                                          int max_indices, int32_t* totals, dfa_stream_t stream) {
    REQUIRE(min_weight >= 1 && min_weight <= 65535, "min_weight outside 1..65535 (the weight is 16 bits; 0 would admit unobserved voxels)");
    return marching_cubes_indexed_common(__func__, volume, occupancy, X, Y, Z, cell_size, tri_table, num_verts_table, min_weight,
                                         out_vertices, max_vertices, out_indices, max_indices, totals, stream);
}

// -------------------------------------------------------------- TSDF seam: point-cloud extraction

static int extract_cloud_common(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3],
                                const float vol2world[12], float* out_points, int max_points, int32_t* total_points,
                                const uint8_t* occupancy, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(voxel_size && vol2world, "null voxel_size / vol2world");
    REQUIRE(max_points >= 0 && (max_points == 0 || out_points), "bad output buffer");
    REQUIRE(((uintptr_t)out_points & 15) == 0, "out_points must be 16-byte aligned");
    REQUIRE((long)X * Y * Z / 64 < (1L << 31), "volume too large");
    const bool vec4  = (X % 4 == 0) && (((uintptr_t)volume & 15) == 0);
    McScratch& scratch = stream_scratch<McScratch>(S(stream));  // (the row segments and the scan are marching cubes')
    HIP_TRY(scratch.reserve(dfa::mc_segments(X, Y, Z, vec4)));
    HIP_TRY(dfa::launch_extract_cloud(volume, X, Y, Z, voxel_size, vol2world, out_points, max_points, total_points,
                                      scratch.seg_off.data, scratch.chunk_sums.data, occupancy, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_extract_cloud(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3], const float vol2world[12],
                           float* out_points, int max_points, int32_t* total_points, dfa_stream_t stream) {
    return extract_cloud_common(volume, X, Y, Z, voxel_size, vol2world, out_points, max_points, total_points, nullptr, stream);
}

int dfa_tsdf_extract_cloud_occ(const uint32_t* volume, const uint8_t* occupancy, int X, int Y, int Z,
                               const float voxel_size[3], const float vol2world[12], float* out_points, int max_points,
                               int32_t* total_points, dfa_stream_t stream) {
    REQUIRE(occupancy, "null occupancy map");
    return extract_cloud_common(volume, X, Y, Z, voxel_size, vol2world, out_points, max_points, total_points, occupancy,
                                stream);
}

int dfa_tsdf_extract_normals(const uint32_t* volume, int X, int Y, int Z, const float voxel_size[3], const float vol2world[12],
                             const float Rinv[9], float gradient_delta_factor, const float* points, int n, float* normals,
                             dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(voxel_size && vol2world && Rinv, "null voxel_size / vol2world / Rinv");
    REQUIRE(n >= 0 && (n == 0 || (points && normals)), "null points / normals");
    REQUIRE(voxel_size[0] > 0.f && voxel_size[1] > 0.f && voxel_size[2] > 0.f && gradient_delta_factor > 0.f,
            "voxel size and gradient delta must be positive");
    REQUIRE((((uintptr_t)points | (uintptr_t)normals) & 15) == 0, "points / normals must be 16-byte aligned");
    HIP_TRY(dfa::launch_extract_normals(volume, X, Y, Z, voxel_size, vol2world, Rinv, gradient_delta_factor, points, n,
                                        normals, S(stream)));
    return DFA_OK;
}

int dfa_color_sample(const uint32_t* colors, int X, int Y, int Z, const float voxel_size[3], const float* vertices, int stride,
                     int N, const float to_volume[12], uint8_t* out, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(colors, X, Y, Z), "bad colour volume");
    REQUIRE(voxel_size && voxel_size[0] > 0.f && voxel_size[1] > 0.f && voxel_size[2] > 0.f, "voxel size must be positive");
    REQUIRE(stride == 3 || stride == 4, "stride must be 3 or 4 floats");
    REQUIRE(N >= 0 && (N == 0 || (vertices && out)), "null vertices / out");
    REQUIRE(((uintptr_t)out & 3) == 0, "out must be 4-byte aligned");
    HIP_TRY(dfa::launch_color_sample(colors, X, Y, Z, voxel_size, vertices, stride, N, to_volume, out, S(stream)));
    return DFA_OK;
}

int dfa_mc_default_tables(int32_t* tri_table, int32_t* num_verts_table) {
    REQUIRE(tri_table && num_verts_table, "null table");
    dfa::mc_default_tables(tri_table, num_verts_table);
    return DFA_OK;
}

// -------------------------------------------------------------- TSDF seam: integration through the warp field

int dfa_tsdf_integrate_warped(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                              uint8_t* occupancy, const float voxel_size[3], float trunc_dist, int max_weight,
                              const float vol2cam[12], float fx, float fy, float cx, float cy, const float* node_pos,
                              const float* node_dq, const float* node_w, int D, int k, int unsupported_mode,
                              dfa_stream_t stream) {
    if (int rc = warped_args_ok(__func__, true, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, vol2cam, trunc_dist,
                                max_weight, node_pos, node_dq, node_w, D, k, unsupported_mode))
        return rc;
    const bool rigid = unsupported_mode == DFA_WARPED_RIGID;
    if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
    WarpedScratch* ws;
    const dfa::KnnGridView* grid;
    if (int rc = warped_scratch(X, Y, Z, node_pos, D, stream, &ws, &grid)) return rc;
    HIP_TRY(dfa::launch_tsdf_integrate_warped(dists, dists_step, cols, rows, volume, X, Y, Z, occupancy, voxel_size, trunc_dist,
                                              max_weight, vol2cam, fx, fy, cx, cy, node_pos, node_dq, node_w, D, k, rigid, grid,
                                              ws->bricks.data, ws->wmax.data, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_integrate_warped6(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                               uint8_t* occupancy, const float voxel_size[3], float trunc_dist, int max_weight,
                               const float vol2node[12], const float node2cam[12], float fx, float fy, float cx, float cy,
                               const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                               int unsupported_mode, dfa_stream_t stream) {
    if (int rc = warped_args_ok(__func__, false, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, nullptr, trunc_dist,
                                max_weight, node_pos, node_dq, node_w, D, k, unsupported_mode))
        return rc;
    const bool rigid = unsupported_mode == DFA_WARPED_RIGID;
    float node2vol[12], stretch, tmax;
    REQUIRE(dfa::warped6_frame(vol2node, node2vol, &stretch, &tmax), "vol2node must be rigid");
    if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
    WarpedScratch* ws;
    const dfa::KnnGridView* grid;
    if (int rc = warped_scratch(X, Y, Z, node_pos, D, stream, &ws, &grid)) return rc;
    HIP_TRY(dfa::launch_tsdf_integrate_warped6(dists, dists_step, cols, rows, volume, X, Y, Z, occupancy, voxel_size, trunc_dist,
                                               max_weight, vol2node, node2cam, node2vol, stretch, tmax, fx, fy, cx, cy, node_pos,
                                               node_dq, node_w, D, k, rigid, grid, ws->bricks.data, ws->wmax.data, S(stream)));
    return DFA_OK;
}

}  // extern "C"
