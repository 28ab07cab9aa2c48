// kernels.hpp — host-callable launchers of the gfx950 kernels (internal; the public surface
// is include/dynfu_amd.h).
#pragma once
#include <map>
#include <mutex>
#include <utility>
#include <hip/hip_runtime.h>
#include <stdint.h>

struct dfa_rigid_align_report;  // include/dynfu_amd.h

namespace dfa {

// tsdf.hip
hipError_t launch_compute_dists(const uint16_t* depth, int depth_step, uint16_t* dists, int dists_step, int cols,
                                int rows, float fx, float fy, float cx, float cy, hipStream_t s);
hipError_t launch_tsdf_clear(uint32_t* vol, int X, int Y, int Z, hipStream_t s);
// Occupancy map of a volume (optional; include/dynfu_amd.h: dfa_tsdf_occupancy_bytes): one byte per box of 32 x 2 x 8 voxels
// — the patch of columns a wave of the sweep owns times one classified run —: bit 0 if a sweep may have left a voxel with a
// non-zero weight in it, bit 1 if one may have left a NEGATIVE distance there (a run classified FULL: FRONT runs write +1).
// Byte ((z / 8) oy + y / 2) ox + x / 32.
struct OccDims {
    int ox, oy, oz;
    __host__ __device__ size_t bytes() const { return (size_t)ox * oy * oz; }
};
__host__ __device__ inline OccDims occ_dims(int X, int Y, int Z) { return OccDims{(X + 31) / 32, (Y + 1) / 2, (Z + 7) / 8}; }
// occ (may be null): fused_clear writes every byte of it (the sweep writes every voxel), the accumulating sweep only sets bytes
hipError_t launch_tsdf_integrate(bool fused_clear, const uint16_t* dists, int dists_step, int cols, int rows,
                                 uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                 int max_weight, const float vol2cam[12], float fx, float fy, float cx, float cy,
                                 uint8_t* occ, bool occ_known /* fused: the map describes the volume on entry */, hipStream_t s);
hipError_t launch_vertex_normals(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float delta_factor,
                                 const float* points, int n, float* normals, hipStream_t s);
hipError_t launch_raycast_points(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3],
                                 float trunc_dist, const float cam2vol[12], const float Rinv[9], float fx, float fy,
                                 float cx, float cy, float step_factor, float delta_factor, float* points,
                                 int points_step, float* normals, int normals_step, int cols, int rows,
                                 hipStream_t s);
hipError_t launch_raycast_tally(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                                float step_factor, float delta_factor, int cols, int rows, unsigned long long* counts,
                                uint32_t* touched, hipStream_t s);
hipError_t launch_raycast_depth(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                                float step_factor, float delta_factor, uint16_t* depth, int depth_step,
                                float* normals, int normals_step, int cols, int rows, hipStream_t s);

// knn_grid.hip
// Uniform grid over the deformation nodes (device-resident, geometry computed on the device).
constexpr int KNN_GRID_MAX_DIM   = 32;
constexpr int KNN_GRID_MAX_CELLS = KNN_GRID_MAX_DIM * KNN_GRID_MAX_DIM * KNN_GRID_MAX_DIM;
struct KnnGridDesc {
    float bmin[3];
    float cs, inv_cs;
    int dim[3];
};
struct KnnGridView {
    KnnGridDesc* desc;
    int32_t* cell_count;  // KNN_GRID_MAX_CELLS   (counts, then fill cursors)
    int32_t* cell_start;  // KNN_GRID_MAX_CELLS + 1
    int32_t* node_cell;   // D
    float4* sorted;       // D   (x, y, z, node index bits), grouped by cell
};
// The same structure at up to 256^3 cells for large point sets (dfa_correspond's canonical cloud)
constexpr int PGRID_MAX_DIM     = 256;   // (128 up to half a million points: see pgrid_finalize_kernel)
constexpr int PGRID_MAX_CELLS   = PGRID_MAX_DIM * PGRID_MAX_DIM * PGRID_MAX_DIM;
constexpr int PGRID_CHUNK       = 8192;  // cells per scan workgroup -> up to 2048 chunks
constexpr int PGRID_BBOX_BLOCKS = 512;
struct PointGridView {
    KnnGridView g;           // cell_count: PGRID_MAX_CELLS, cell_start: PGRID_MAX_CELLS + 1
    int32_t* chunk_sums;     // PGRID_MAX_CELLS / PGRID_CHUNK
    float* bbox_partials;    // PGRID_BBOX_BLOCKS x 6
};
hipError_t point_grid_build(const PointGridView& pg, const float* pts, int n, hipStream_t s);
hipError_t knn_grid_build(const KnnGridView& g, const float* node_pos, int D, hipStream_t s);

// knn.hip
// grid == nullptr: exhaustive scan
hipError_t launch_knn(const float* node_pos, const float* node_w, int D, const float* query, int n_query, int k,
                      int32_t* idx, float* weights, const KnnGridView* grid, hipStream_t s);

// correspond.hip
hipError_t launch_correspond_projective(const float* verts, const float* normals, int n, const float* vmap, int vmap_step,
                                        const float* nmap, int nmap_step, int cols, int rows, float fx, float fy, float cx,
                                        float cy, float dist_thres, float min_cosine, float* out_v, float* out_n,
                                        int32_t* out_pixel, hipStream_t s);
hipError_t launch_correspond(const float* canon_v, const float* canon_n, int n_canon, const float* live_v,
                             int n_live, float* out_v, float* out_n, int32_t* out_idx, const KnnGridView* grid,
                             hipStream_t s);

// warp.hip
hipError_t launch_warp_to_live(const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                               const float* verts, const float* normals, int N, float* out_verts, float* out_normals,
                               const KnnGridView* grid, hipStream_t s);
hipError_t launch_dqb_support(const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                              const float* pts, int n, float* out_dq, uint8_t* out_flag, const KnnGridView* grid,
                              hipStream_t s);
hipError_t launch_warp_graph(const float* node_pos, const float* node_dq, const float* node_w, int k, const int32_t* idx,
                             const float* verts, const float* normals, int N, float* out_verts, float* out_normals,
                             hipStream_t s);

// tsdf_warped.hip — a depth frame integrated through the warp field, the four sweeps: searching (here) and served from a k-NN
// field (below, behind KnnFieldView).  dfa_tsdf_integrate_warped: bricks: knn_field_bricks(X, Y, Z) bytes (warped_bricks.hpp)
// and wmax: one float, both device scratch of the call; grid: the node grid (knn_grid_build) or null = scan all nodes
hipError_t launch_tsdf_integrate_warped(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, int X, int Y,
                                        int Z, uint8_t* occ, const float voxel_size[3], float trunc_dist, int max_weight,
                                        const float vol2cam[12], float fx, float fy, float cx, float cy, const float* node_pos,
                                        const float* node_dq, const float* node_w, int D, int k, bool rigid,
                                        const KnnGridView* grid, uint8_t* bricks, float* wmax, hipStream_t s);
// ... through the north-star warp field (dfa_tsdf_integrate_warped6).  warped6_frame (host): vol2node checked for rigidity
// (false: refused) and inverted — node2vol, the pre-pass's relative widening `stretch` and the largest |translation| `tmax`,
// which the launcher takes beside the two transforms (each may be null: identity)
bool warped6_frame(const float* vol2node, float node2vol[12], float* stretch, float* tmax);
hipError_t launch_tsdf_integrate_warped6(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, int X, int Y,
                                         int Z, uint8_t* occ, const float voxel_size[3], float trunc_dist, int max_weight,
                                         const float* vol2node, const float* node2cam, const float node2vol[12], float stretch,
                                         float tmax, float fx, float fy, float cx, float cy, const float* node_pos,
                                         const float* node_dq, const float* node_w, int D, int k, bool rigid,
                                         const KnnGridView* grid, uint8_t* bricks, float* wmax, hipStream_t s);

// knn_field.hip — the k-NN field of a volume (dfa_knn_field_*: stored set, search, merge, lookup): per stored brick (the 64 x 4 x 1 voxels of the warped sweeps)
// one record of k slots x 256 int32 ids, slot-major — ids[(record k + slot) 256 + voxel of the brick] —, a table brick ->
// record (-1: not stored) and the list record -> brick.  A brick is stored when a node's OWN radius reaches its box.
struct KnnFieldView {
    int X, Y, Z, k;
    float vs[3];
    int has_frame;  // vol2node given: the search position is c = R_n v + t_n
    float vol2node[12], node2vol[12], stretch, tmax;  // (warped6_frame's)
    int32_t* table;   // knn_field_bricks(X, Y, Z)
    int32_t* coords;  // per record: its brick's index in the table
    int32_t* ids;     // records x k x 256
};
// Step 1 of an extension by the nodes [first, D): the bricks they reach that the table does not hold yet, counted.  marks:
// one byte per brick; offsets: bricks + 1 ints (on return the exclusive scan of the new bricks' flags); chunk_sums:
// mc_scan_chunks(bricks) ints; total: one device int, the number of new bricks.  Writes scratch only.
hipError_t launch_knn_field_count(const KnnFieldView& f, const float* node_pos, const float* node_w, int first, int D,
                                  uint8_t* marks, int32_t* offsets, int32_t* chunk_sums, int32_t* total, hipStream_t s);
// Step 2: the new bricks become records [records, records + fresh) with a search over all D nodes (grid: the node grid or
// null = scan), and every voxel of the records [0, records) merges the nodes [D_old, D) into its list.
hipError_t launch_knn_field_extend(const KnnFieldView& f, const float* node_pos, int D_old, int D, size_t records, size_t fresh,
                                   const int32_t* offsets, const KnnGridView* grid, hipStream_t s);
hipError_t launch_knn_field_lookup(const KnnFieldView& f, const int32_t* voxels, int n, int32_t* out_idx, hipStream_t s);
// tsdf_warped.hip — the two warped sweeps with the neighbours read from the field (records: the number of stored bricks)
hipError_t launch_tsdf_integrate_warped_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol,
                                              uint8_t* occ, float trunc_dist, int max_weight, const float vol2cam[12], float fx,
                                              float fy, float cx, float cy, const float* node_pos, const float* node_dq,
                                              const float* node_w, bool rigid, const KnnFieldView& f, size_t records,
                                              hipStream_t s);
hipError_t launch_tsdf_integrate_warped6_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol,
                                               uint8_t* occ, float trunc_dist, int max_weight, const float* node2cam, float fx,
                                               float fy, float cx, float cy, const float* node_pos, const float* node_dq,
                                               const float* node_w, bool rigid, const KnnFieldView& f, size_t records,
                                               hipStream_t s);

// tsdf_warped_color.hip — dfa_tsdf_integrate_warped6_color: the two north-star sweeps above (searching: grid, bricks, wmax
// as launch_tsdf_integrate_warped6; or from the field) with the colour rule of warped_color_device.hpp behind the distance.
// vol null: colours only — no TSDF word and no byte of occ is read or written.
struct ColorArgs {
    const uint8_t* image;  // b, g, r, x pixels, the dists image's cols x rows; rows 4-byte aligned
    int image_step;
    uint32_t* colors;      // X Y Z words, the volume's order
    int max_color_weight;  // 1..255
};
// tsdf_warped.hip — the support pre-pass of the searching north-star sweeps: bricks cleared, then marked by the nodes
hipError_t launch_warped6_mark_bricks(const float* node_pos, const float* node_w, int D, bool has_vol2node, const float node2vol[12],
                                      float stretch, float tmax, int X, int Y, int Z, const float voxel_size[3], uint8_t* bricks,
                                      float* wmax, hipStream_t s);
hipError_t launch_tsdf_integrate_warped6_color(const uint16_t* dists, int dists_step, int cols, int rows, const ColorArgs& color,
                                               uint32_t* vol, int X, int Y, int Z, uint8_t* occ, const float voxel_size[3],
                                               float trunc_dist, int max_weight, const float* vol2node, const float* node2cam,
                                               const float node2vol[12], float stretch, float tmax, float fx, float fy, float cx,
                                               float cy, const float* node_pos, const float* node_dq, const float* node_w, int D,
                                               int k, bool rigid, const KnnGridView* grid, uint8_t* bricks, float* wmax,
                                               hipStream_t s);
hipError_t launch_tsdf_integrate_warped6_color_field(const uint16_t* dists, int dists_step, int cols, int rows, const ColorArgs& color,
                                                     uint32_t* vol, uint8_t* occ, float trunc_dist, int max_weight,
                                                     const float* node2cam, float fx, float fy, float cx, float cy,
                                                     const float* node_pos, const float* node_dq, const float* node_w, bool rigid,
                                                     const KnnFieldView& f, size_t records, hipStream_t s);
// color.hip — dfa_color_sample: per vertex, the colour volume's words blended over the 8 corners of its cell
hipError_t launch_color_sample(const uint32_t* colors, int X, int Y, int Z, const float voxel_size[3], const float* vertices,
                               int stride, int N, const float* to_volume, uint8_t* out, hipStream_t s);

// points.hip
hipError_t launch_repack_points(const float* src, int sstride, float* dst, int dstride, int n, float pad, hipStream_t s);
hipError_t launch_transform_points(const float* in, int n, const float aff[12], bool with_translation, float* out, hipStream_t s);
int compact_chunks(int n);  // entries of chunk_scratch
hipError_t launch_compact_points(const float* pts, const uint8_t* flags, int n, float* out_pts, int32_t* out_idx,
                                 int32_t* count, int32_t* chunk_scratch, hipStream_t s);

// mc.hip
long mc_segments(int X, int Y, int Z, bool vec4);  // entries of seg_off (+1)
long mc_scan_chunks(long nsegs);                   // entries of chunk_sums
hipError_t launch_marching_cubes(const uint32_t* vol, int X, int Y, int Z, const float cell_size[3],
                                 const int32_t* tri_table, const int32_t* num_verts_table, float* out_points,
                                 int max_vertices, int32_t* total_vertices, int32_t* seg_off, int32_t* chunk_sums,
                                 const uint8_t* occ /* occupancy map of the volume or null */, hipStream_t s);
// indexed mesh (dfa_marching_cubes_indexed): voff / ioff hold mci_segments(X, Y, Z) + 1 entries each (segments of 256
// voxels, whatever the alignment), chunk_sums mc_scan_chunks of that; totals: device, 2 ints
long mci_segments(int X, int Y, int Z);
hipError_t launch_marching_cubes_indexed(const uint32_t* vol, int X, int Y, int Z, const float cell_size[3],
                                         const int32_t* tri_table, const int32_t* num_verts_table, float* out_vertices,
                                         int max_vertices, int32_t* out_indices, int max_indices, int32_t* totals,
                                         int32_t* voff, int32_t* ioff, int32_t* chunk_sums, const uint8_t* occ,
                                         hipStream_t s);
// ... with a weight floor (dfa_marching_cubes_indexed_min_weight): a voxel counts as observed from min_weight (1..65535) on
hipError_t launch_marching_cubes_indexed_min_weight(const uint32_t* vol, int X, int Y, int Z, const float cell_size[3],
                                                    const int32_t* tri_table, const int32_t* num_verts_table,
                                                    int min_weight, float* out_vertices, int max_vertices,
                                                    int32_t* out_indices, int max_indices, int32_t* totals, int32_t* voff,
                                                    int32_t* ioff, int32_t* chunk_sums, const uint8_t* occ, hipStream_t s);
void mc_default_tables(int32_t tri_table[256 * 16], int32_t num_verts_table[256]);
// exclusive scan of n segment counts in place (counts: n + 1 entries; counts[n] and *total (device, optional) receive the
// sum; chunk_sums: mc_scan_chunks(n) entries) — marching cubes' step 2, shared with the point-cloud extraction
void launch_segment_scan(int32_t* counts, long n, int32_t* chunk_sums, int32_t* total, hipStream_t s);

// extract.hip — TsdfVolume::fetchCloud (kfusion extract_kernel); the row segments are marching cubes' (mc_segments)
hipError_t launch_extract_cloud(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], const float vol2world[12],
                                float* out_points, int max_points, int32_t* total_points, int32_t* seg_off, int32_t* chunk_sums,
                                const uint8_t* occ /* occupancy map of the volume or null */, hipStream_t s);
// tsdf.hip (beside the raycaster's interpolate) — TsdfVolume::fetchNormals (kfusion extract_normals_kernel)
hipError_t launch_extract_normals(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], const float vol2world[12],
                                  const float Rinv[9], float delta_factor, const float* points, int n, float* normals,
                                  hipStream_t s);

// render.hip — the Phong / normal-colour views (kfusion imgproc.cu:363-514) and the raycast fused with them
hipError_t launch_render_points(const float* points, int points_step, const float* normals, int normals_step, int cols,
                                int rows, const float light[3], uint8_t* image, int image_step, hipStream_t s);
hipError_t launch_render_depth(const uint16_t* depth, int depth_step, const float* normals, int normals_step, int cols,
                               int rows, float fx, float fy, float cx, float cy, const float light[3], uint8_t* image,
                               int image_step, hipStream_t s);
hipError_t launch_tangent_colors(const float* normals, int normals_step, int cols, int rows, uint8_t* image, int image_step,
                                 hipStream_t s);
hipError_t launch_raycast_render(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                 const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                                 float step_factor, float delta_factor, int cols, int rows, const float light[3], int mode,
                                 uint8_t* image, int image_step, hipStream_t s);

// raster.hip — the mesh rasteriser (z-buffer fill, draw, resolve)
hipError_t launch_mesh_rasterize(const float* vertices, const float* normals, int N, const int32_t* indices, int T,
                                 const float world2cam[12], float fx, float fy, float cx, float cy, float z_near, int cols,
                                 int rows, uint64_t* zbuffer, float* points, int points_step, float* out_normals,
                                 int normals_step, hipStream_t s);

// visibility.hip — a cloud's vertices against a model point map (dfa_visible_vertices).  partial: visible_blocks(n) ints of
// device scratch, needed when count is given
int visible_blocks(int n);
hipError_t launch_visible_vertices(const float* vertices, int stride, int n, const float* model_points, int points_step, int cols,
                                   int rows, float fx, float fy, float cx, float cy, float z_tol, uint8_t* flags, int32_t* count,
                                   int32_t* partial, hipStream_t s);

// img.hip
hipError_t launch_bilateral(const uint16_t* src, int src_step, uint16_t* dst, int dst_step, int cols, int rows, int ksz,
                            float sigma_spatial, float sigma_depth, hipStream_t s);
hipError_t launch_truncate_depth(uint16_t* depth, int step, int cols, int rows, float max_dist, hipStream_t s);
hipError_t launch_depth_pyr(const uint16_t* src, int src_step, int cols, int rows, uint16_t* dst, int dst_step,
                            float sigma_depth, hipStream_t s);
hipError_t launch_normals_mask_depth(uint16_t* depth, int depth_step, int cols, int rows, float fx, float fy, float cx,
                                     float cy, float* normals, int normals_step, hipStream_t s);
hipError_t launch_points_normals(const uint16_t* depth, int depth_step, int cols, int rows, float fx, float fy, float cx,
                                 float cy, float* points, int points_step, float* normals, int normals_step,
                                 hipStream_t st);
hipError_t launch_resize_depth_normals(const uint16_t* dsrc, int dsrc_step, const float* nsrc, int nsrc_step, int cols,
                                       int rows, uint16_t* ddst, int ddst_step, float* ndst, int ndst_step, hipStream_t s);
hipError_t launch_resize_points_normals(const float* vsrc, int vsrc_step, const float* nsrc, int nsrc_step, int cols,
                                        int rows, float* vdst, int vdst_step, float* ndst, int ndst_step, hipStream_t s);

// icp.hip
size_t icp_partial_floats(int cols, int rows);
hipError_t launch_icp_sums(bool depth_variant, const void* curr, int curr_step, const float* ncurr, int ncurr_step,
                           const void* prev, int prev_step, const float* nprev, int nprev_step, int cols, int rows,
                           const float aff[12], float fx, float fy, float cx, float cy, float dist_thres, float angle_thres,
                           float* partial, float* sums27, unsigned int* matched, hipStream_t s);
// the same sums over a cloud against the live maps (the north-star data term's association); n = 0: zeros, no kernel
size_t rigid_cloud_partial_floats(int n);
hipError_t launch_rigid_sums_cloud(const float* vertices, const float* normals, int stride, int n, const float aff[12],
                                   const float* vmap, int vstep, const float* nmap, int nstep, int cols, int rows, float fx,
                                   float fy, float cx, float cy, float dist_thresh, float cos_thresh, float* partial,
                                   float* sums27, unsigned int* matched, hipStream_t s);
// the whole rigid Gauss-Newton on the device (dfa_rigid_align_cloud; rigid_step.hpp states the step and the rules): two
// launches per iteration, all enqueued on s, nothing waits for the host.  scratch: rigid_align_scratch_floats(...) floats
// — the state of the call (RIGID_STATE_FLOATS), then the partial sums of the largest level.  The schedule is checked by
// the caller: 1 <= levels <= 4, steps >= 1, iters >= 0, at most 64 iterations in all
constexpr size_t RIGID_STATE_FLOATS = 128;
size_t rigid_align_scratch_floats(int n, const int* level_step, int levels);
hipError_t launch_rigid_align_cloud(const float* vertices, const float* normals, int stride, int n, const float aff0[12],
                                    const float* vmap, int vstep, const float* nmap, int nstep, int cols, int rows, float fx,
                                    float fy, float cx, float cy, float dist_thresh, float cos_thresh, const int* level_step,
                                    const int* level_iters, int levels, float stop_rot, float stop_trans,
                                    dfa_rigid_align_report* report, float* trace, float* scratch, hipStream_t s);


// Several kernels publish partial results with write-through stores and then arrive at a ticket / raise a flag word, ordering
// the two by `s_waitcnt vmcnt(0)` (solve_linearise.hip: linearise tail; solve_pcg_team.hip; solve6_linearise.hip: linearise tail).  That is an ordering
// on gfx9 parts only, where stores count in vmcnt; gfx10 and later track them in vscnt.  This library is built for gfx950.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "dynfu_amd orders published stores with s_waitcnt vmcnt(0): gfx90a / gfx942 / gfx950 only"
#endif

// hipFuncAttributeMaxDynamicSharedMemorySize is an attribute of a kernel ON A DEVICE: the opt-in to more than 48 KiB of
// dynamic LDS is made once per (device, kernel), under a lock (the C ABI serves several devices and host threads)
inline hipError_t allow_dynamic_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> done;
    int dev      = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    int& have = done[std::make_pair(dev, kernel)];
    if (have >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

}  // namespace dfa
