// capi_field.cpp — C ABI (include/dynfu_amd.h), the k-NN field of a volume: dfa_knn_field_*, the two warped integrations
// served from a field and the coloured north-star integration (searching or from a field: its one entry point takes either).
// Argument checks, the field's memory and launcher calls only (capi_internal.hpp); the field's kernels are in knn_field.hip,
// the sweeps in tsdf_warped.hip and tsdf_warped_color.hip, the size arithmetic in warped_bricks.hpp.
#include <algorithm>
#include <cstring>

#include "capi_internal.hpp"
#include "warped_bricks.hpp"

using namespace dfa::capi;
using dfa::DeviceBuffer;

// the opaque object: geometry and frame fixed at creation, the node count and the stored bricks as of the last build / append
struct dfa_knn_field {
    dfa::KnnFieldView v{};  // (the device pointers are refreshed from the buffers below before every launch)
    size_t max_bytes = 0, bricks = 0, records = 0;
    int D = 0;
    DeviceBuffer<int32_t> table, coords, ids;
    // scratch of a build / append: brick marks, the scan of the new bricks, its partials and its total
    DeviceBuffer<uint8_t> marks;
    DeviceBuffer<int32_t> offsets, chunk_sums, total;

    const dfa::KnnFieldView& view() {
        v.table = table.data, v.coords = coords.data, v.ids = ids.data;
        return v;
    }
    void release() {
        table.release(), coords.release(), ids.release(), marks.release(), offsets.release(), chunk_sums.release(), total.release();
    }
};

namespace {

// what the cached integrations require of a field, beyond the checks of the uncached calls
int field_matches(const char* fn, const dfa_knn_field* f, int X, int Y, int Z, const float voxel_size[3], int k, int D,
                  const float* vol2node, bool reference_mode) {
#define MATCH(cond, msg) REQUIRE_AS(fn, cond, msg)
    MATCH(f, "null field");
    MATCH(f->v.X == X && f->v.Y == Y && f->v.Z == Z && std::memcmp(f->v.vs, voxel_size, sizeof(float) * 3) == 0,
          "the field belongs to another volume geometry");
    MATCH(f->v.k == k, "the field was created for another k");
    MATCH(f->D == D, "the field holds another number of nodes (dfa_knn_field_append brings it up to date)");
    MATCH(!reference_mode || !f->v.has_frame, "the field has a vol2node: it serves dfa_tsdf_integrate_warped6_field only");
    MATCH(reference_mode || ((vol2node != nullptr) == (f->v.has_frame != 0) &&
                             (!vol2node || std::memcmp(f->v.vol2node, vol2node, sizeof(float) * 12) == 0)),
          "vol2node differs from the field's");
#undef MATCH
    return DFA_OK;
}

// nodes [D_old, D) join the field (D_old == f->D; a build comes here with an emptied field)
int field_extend(dfa_knn_field* f, const float* node_pos, const float* node_w, int D, dfa_stream_t stream, const char* fn) {
    const int D_old = f->D;
    if (D == D_old) return DFA_OK;
    hipStream_t st = S(stream);
    // the table exists from the first node on, every brick -1
    if (!f->table.data) {
        HIP_TRY(f->table.reserve(f->bricks));
        HIP_TRY(hipMemsetAsync(f->table.data, 0xff, sizeof(int32_t) * f->bricks, st));
    }
    HIP_TRY(f->marks.reserve(f->bricks));
    HIP_TRY(f->offsets.reserve(f->bricks + 1));
    HIP_TRY(f->chunk_sums.reserve((size_t)dfa::mc_scan_chunks((long)f->bricks)));
    HIP_TRY(f->total.reserve(1));
    HIP_TRY(dfa::launch_knn_field_count(f->view(), node_pos, node_w, D_old, D, f->marks.data, f->offsets.data, f->chunk_sums.data,
                                        f->total.data, st));
    int32_t fresh = 0;  // the one wait: how many bricks join
    HIP_TRY(hipMemcpyAsync(&fresh, f->total.data, sizeof(fresh), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t records = f->records + (size_t)fresh;
    if (!dfa::knn_field_fits(records, f->v.k, f->max_bytes))
        return fail(DFA_ERR_CAPACITY, "%s: %zu stored bricks of %zu bytes each exceed max_bytes = %zu", fn, records,
                    dfa::knn_field_record_bytes(f->v.k), f->max_bytes);
    // a warp field grows by a few nodes per frame: a quarter of headroom, as the node grid's
    const size_t per = dfa::knn_field_record_bytes(f->v.k) / sizeof(int32_t);
    size_t room      = records / 4;
    if (f->max_bytes) room = std::min(room, f->max_bytes / dfa::knn_field_record_bytes(f->v.k) - records);
    HIP_TRY(f->coords.grow_keep(records, f->records, room, st));
    HIP_TRY(f->ids.grow_keep(records * per, f->records * per, room * per, st));
    const dfa::KnnGridView* grid;
    if (int rc = warped_node_grid(node_pos, D, st, &grid)) return rc;
    HIP_TRY(dfa::launch_knn_field_extend(f->view(), node_pos, D_old, D, f->records, (size_t)fresh, f->offsets.data, grid, st));
    f->records = records, f->D = D;
    return DFA_OK;
}

}  // namespace

extern "C" {

int dfa_knn_field_create(int X, int Y, int Z, const float voxel_size[3], int k, const float vol2node[12], size_t max_bytes,
                         dfa_knn_field** out) {
    REQUIRE(out, "null out");
    *out = nullptr;
    REQUIRE(X > 0 && Y > 0 && Z > 0, "bad volume dimensions");
    REQUIRE(voxel_size, "null voxel_size");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    REQUIRE(dfa::knn_field_bricks(X, Y, Z) <= dfa::KNN_FIELD_MAX_RECORDS, "volume too large");
    float node2vol[12], stretch, tmax;
    REQUIRE(dfa::warped6_frame(vol2node, node2vol, &stretch, &tmax), "vol2node must be rigid");
    dfa_knn_field* f = new dfa_knn_field;
    f->v.X = X, f->v.Y = Y, f->v.Z = Z, f->v.k = k;
    std::memcpy(f->v.vs, voxel_size, sizeof(float) * 3);
    f->v.has_frame = vol2node ? 1 : 0;
    if (vol2node) std::memcpy(f->v.vol2node, vol2node, sizeof(float) * 12);
    std::memcpy(f->v.node2vol, node2vol, sizeof(node2vol));
    f->v.stretch = stretch, f->v.tmax = tmax;
    f->max_bytes = max_bytes;
    f->bricks    = dfa::knn_field_bricks(X, Y, Z);
    *out         = f;
    return DFA_OK;
}

void dfa_knn_field_destroy(dfa_knn_field* field) {
    if (!field) return;
    field->release();
    delete field;
}

int dfa_knn_field_build(dfa_knn_field* field, const float* node_pos, const float* node_w, int D, dfa_stream_t stream) {
    REQUIRE(field, "null field");
    REQUIRE(D >= 0, "negative node count");
    REQUIRE(D == 0 || (node_pos && node_w), "nodes without positions or radii");
    // empty first (the rows stay allocated: nothing points at them)
    if (field->table.data && field->records > 0)
        HIP_TRY(hipMemsetAsync(field->table.data, 0xff, sizeof(int32_t) * field->bricks, S(stream)));
    field->records = 0, field->D = 0;
    return field_extend(field, node_pos, node_w, D, stream, __func__);
}

int dfa_knn_field_append(dfa_knn_field* field, const float* node_pos, const float* node_w, int D_new, dfa_stream_t stream) {
    REQUIRE(field, "null field");
    REQUIRE(D_new >= field->D, "D_new is smaller than the field's node count: nodes are only ever appended");
    REQUIRE(D_new == 0 || (node_pos && node_w), "nodes without positions or radii");
    return field_extend(field, node_pos, node_w, D_new, stream, __func__);
}

int dfa_knn_field_info(const dfa_knn_field* field, dfa_knn_field_desc* info) {
    REQUIRE(field && info, "null field / info");
    info->D = field->D, info->k = field->v.k;
    info->stored_bricks = (int64_t)field->records, info->total_bricks = (int64_t)field->bricks;
    info->bytes = (uint64_t)(field->records * dfa::knn_field_record_bytes(field->v.k));
    return DFA_OK;
}

int dfa_knn_field_lookup(const dfa_knn_field* field, const int32_t* voxels, int n, int32_t* out_idx, dfa_stream_t stream) {
    REQUIRE(field, "null field");
    REQUIRE(n >= 0 && (n == 0 || (voxels && out_idx)), "null voxels / out_idx");
    HIP_TRY(dfa::launch_knn_field_lookup(const_cast<dfa_knn_field*>(field)->view(), voxels, n, out_idx, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_integrate_warped_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                                    uint8_t* occupancy, const float voxel_size[3], float trunc_dist, int max_weight,
                                    const float vol2cam[12], float fx, float fy, float cx, float cy, const float* node_pos,
                                    const float* node_dq, const float* node_w, int D, int k, int unsupported_mode,
                                    const dfa_knn_field* field, dfa_stream_t stream) {
    if (int rc = warped_args_ok(__func__, true, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, vol2cam, trunc_dist,
                                max_weight, node_pos, node_dq, node_w, D, k, unsupported_mode))
        return rc;
    const bool rigid = unsupported_mode == DFA_WARPED_RIGID;
    if (int rc = field_matches(__func__, field, X, Y, Z, voxel_size, k, D, nullptr, true)) return rc;
    if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
    dfa_knn_field* f = const_cast<dfa_knn_field*>(field);
    HIP_TRY(dfa::launch_tsdf_integrate_warped_field(dists, dists_step, cols, rows, volume, occupancy, trunc_dist, max_weight, vol2cam,
                                                    fx, fy, cx, cy, node_pos, node_dq, node_w, rigid, f->view(), f->records,
                                                    S(stream)));
    return DFA_OK;
}

int dfa_tsdf_integrate_warped6_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                                     uint8_t* occupancy, const float voxel_size[3], float trunc_dist, int max_weight,
                                     const float vol2node[12], const float node2cam[12], float fx, float fy, float cx, float cy,
                                     const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                                     int unsupported_mode, const dfa_knn_field* field, dfa_stream_t stream) {
    if (int rc = warped_args_ok(__func__, false, dists, dists_step, cols, rows, volume, X, Y, Z, voxel_size, nullptr, trunc_dist,
                                max_weight, node_pos, node_dq, node_w, D, k, unsupported_mode))
        return rc;
    const bool rigid = unsupported_mode == DFA_WARPED_RIGID;
    if (int rc = field_matches(__func__, field, X, Y, Z, voxel_size, k, D, vol2node, false)) return rc;
    if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
    dfa_knn_field* f = const_cast<dfa_knn_field*>(field);
    HIP_TRY(dfa::launch_tsdf_integrate_warped6_field(dists, dists_step, cols, rows, volume, occupancy, trunc_dist, max_weight, node2cam,
                                                     fx, fy, cx, cy, node_pos, node_dq, node_w, rigid, f->view(), f->records,
                                                     S(stream)));
    return DFA_OK;
}

int dfa_tsdf_integrate_warped6_color(const uint16_t* dists, int dists_step, int cols, int rows, const uint8_t* image, int image_step,
                                     uint32_t* volume, uint32_t* colors, int X, int Y, int Z, uint8_t* occupancy,
                                     const float voxel_size[3], float trunc_dist, int max_weight, int max_color_weight,
                                     const float vol2node[12], const float node2cam[12], float fx, float fy, float cx, float cy,
                                     const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                                     int unsupported_mode, const dfa_knn_field* field, dfa_stream_t stream) {
    REQUIRE(colors, "null colour volume");
    REQUIRE(image, "null colour image");
    REQUIRE(max_color_weight >= 1 && max_color_weight <= 255, "max_color_weight outside 1..255 (the colour weight is 8 bits)");
    // (volume may be null — colours only —: the colour volume stands in where the checks ask for the volume's geometry)
    if (int rc = warped_args_ok(__func__, false, dists, dists_step, cols, rows, colors, X, Y, Z, voxel_size, nullptr, trunc_dist,
                                max_weight, node_pos, node_dq, node_w, D, k, unsupported_mode))
        return rc;
    REQUIRE(cols <= 0x1fffffff && image_step >= cols * 4, "image row step smaller than a pixel row");
    REQUIRE((((uintptr_t)image | (uintptr_t)image_step) & 3) == 0, "image rows must be 4-byte aligned");
    const bool rigid = unsupported_mode == DFA_WARPED_RIGID;
    const dfa::ColorArgs color{image, image_step, colors, max_color_weight};
    if (field) {
        if (int rc = field_matches(__func__, field, X, Y, Z, voxel_size, k, D, vol2node, false)) return rc;
        if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
        dfa_knn_field* f = const_cast<dfa_knn_field*>(field);
        HIP_TRY(dfa::launch_tsdf_integrate_warped6_color_field(dists, dists_step, cols, rows, color, volume, occupancy, trunc_dist,
                                                               max_weight, node2cam, fx, fy, cx, cy, node_pos, node_dq, node_w, rigid,
                                                               f->view(), f->records, S(stream)));
        return DFA_OK;
    }
    float node2vol[12], stretch, tmax;
    REQUIRE(dfa::warped6_frame(vol2node, node2vol, &stretch, &tmax), "vol2node must be rigid");
    if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
    WarpedScratch* ws;
    const dfa::KnnGridView* grid;
    if (int rc = warped_scratch(X, Y, Z, node_pos, D, stream, &ws, &grid)) return rc;
    HIP_TRY(dfa::launch_tsdf_integrate_warped6_color(dists, dists_step, cols, rows, color, volume, X, Y, Z, occupancy, voxel_size,
                                                     trunc_dist, max_weight, vol2node, node2cam, node2vol, stretch, tmax, fx, fy, cx,
                                                     cy, node_pos, node_dq, node_w, D, k, rigid, grid, ws->bricks.data, ws->wmax.data,
                                                     S(stream)));
    return DFA_OK;
}

}  // extern "C"
