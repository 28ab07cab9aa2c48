// capi_warp.cpp — C ABI (include/dynfu_amd.h), the warp-field seam and the point utilities: k-NN, warping, blending,
// repack / transform / compact, the two correspondence searches, with the scratch each keeps per stream.  Argument
// checks and launcher calls only (capi_internal.hpp); the kernels are in knn_grid.hip, knn.hip, warp.hip, correspond.hip and points.hip.
#include "capi_internal.hpp"

using namespace dfa::capi;
using dfa::DeviceBuffer;
using dfa::stream_scratch;

namespace {

// scratch of the 128^3 point grid of dfa_correspond
struct PointGridScratch {
    GridScratch g;
    DeviceBuffer<int32_t> chunk_sums;
    DeviceBuffer<float> bbox_partials;
    dfa::PointGridView v{};
    hipError_t reserve(int n) {  // clouds of consecutive frames differ by a few per cent (see GridScratch)
        const size_t cells = dfa::PGRID_MAX_CELLS;
        hipError_t e;
        if ((e = g.reserve(cells, (size_t)n, (size_t)n / 4 + 1024)) || (e = chunk_sums.reserve(cells / dfa::PGRID_CHUNK)) ||
            (e = bbox_partials.reserve(6 * dfa::PGRID_BBOX_BLOCKS)))
            v = dfa::PointGridView{};
        else v = dfa::PointGridView{g.v, chunk_sums.data, bbox_partials.data};
        return e;
    }
};

struct CompactScratch : DeviceBuffer<int32_t> {};  // chunk counts of dfa_compact_points

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------- warp-field seam

int dfa_knn(const float* node_pos, const float* node_w, int D, const float* query, int n_query, int k, int32_t* idx,
            float* weights, dfa_stream_t stream) {
    REQUIRE(node_pos && D > 0, "no nodes");
    REQUIRE(n_query >= 0 && (n_query == 0 || (query && idx)), "bad query / output");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    REQUIRE(!weights || node_w, "weights requested without node_w");
    const dfa::KnnGridView* grid;
    if (int rc = scratch_grid(node_pos, D, n_query, S(stream), &grid)) return rc;
    HIP_TRY(dfa::launch_knn(node_pos, node_w, D, query, n_query, k, idx, weights, grid, S(stream)));
    return DFA_OK;
}

int dfa_warp_to_live(const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                     const float* vertices, const float* normals, int N, float* out_vertices, float* out_normals,
                     dfa_stream_t stream) {
    REQUIRE(node_pos && node_dq && node_w && D > 0, "no nodes");
    REQUIRE(N >= 0 && (N == 0 || (vertices && out_vertices)), "bad vertices / output");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    const dfa::KnnGridView* grid;
    if (int rc = scratch_grid(node_pos, D, N, S(stream), &grid)) return rc;
    HIP_TRY(dfa::launch_warp_to_live(node_pos, node_dq, node_w, D, k, vertices, normals, N, out_vertices,
                                     out_normals, grid, S(stream)));
    return DFA_OK;
}

int dfa_warp_to_live_graph(const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                           const int32_t* idx, const float* vertices, const float* normals, int N, float* out_vertices,
                           float* out_normals, dfa_stream_t stream) {
    REQUIRE(node_pos && node_dq && node_w && D > 0, "no nodes");
    REQUIRE(N >= 0 && (N == 0 || (vertices && out_vertices && idx)), "bad vertices / graph / output");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    if (N > 0)
        HIP_TRY(dfa::launch_warp_graph(node_pos, node_dq, node_w, k, idx, vertices, normals, N, out_vertices, out_normals,
                                       S(stream)));
    return DFA_OK;
}

int dfa_calc_dqb(const float* node_pos, const float* node_dq, const float* node_w, int D, int k, const float* points,
                 int n, float* out_dq, dfa_stream_t stream) {
    REQUIRE(node_pos && node_dq && node_w && D > 0, "no nodes");
    REQUIRE(n >= 0 && (n == 0 || (points && out_dq)), "bad points / output");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    const dfa::KnnGridView* grid;
    if (int rc = scratch_grid(node_pos, D, n, S(stream), &grid)) return rc;
    HIP_TRY(dfa::launch_dqb_support(node_pos, node_dq, node_w, D, k, points, n, out_dq, nullptr, grid, S(stream)));
    return DFA_OK;
}

int dfa_unsupported_vertices(const float* node_pos, const float* node_w, int D, int k, const float* vertices, int N,
                             uint8_t* flags, dfa_stream_t stream) {
    REQUIRE(N >= 0 && (N == 0 || (vertices && flags)), "bad vertices / output");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    if (D == 0) {  // no node supports anything (min stays HUGE_VALF, warp_field.cpp:40,53)
        if (N > 0) HIP_TRY(hipMemsetAsync(flags, 1, (size_t)N, S(stream)));
        return DFA_OK;
    }
    REQUIRE(node_pos && node_w && D > 0, "bad nodes");
    const dfa::KnnGridView* grid;
    if (int rc = scratch_grid(node_pos, D, N, S(stream), &grid)) return rc;
    HIP_TRY(dfa::launch_dqb_support(node_pos, nullptr, node_w, D, k, vertices, N, nullptr, flags, grid, S(stream)));
    return DFA_OK;
}

int dfa_repack_points(const float* src, int src_stride, float* dst, int dst_stride, int n, float pad,
                      dfa_stream_t stream) {
    REQUIRE(n >= 0 && (n == 0 || (src && dst)), "bad points");
    REQUIRE(src_stride >= 3 && dst_stride >= 3, "strides are floats per point, >= 3");
    REQUIRE(src_stride != 4 || ((uintptr_t)src & 15) == 0, "float4 source must be 16-byte aligned");
    REQUIRE(dst_stride != 4 || ((uintptr_t)dst & 15) == 0, "float4 destination must be 16-byte aligned");
    HIP_TRY(dfa::launch_repack_points(src, src_stride, dst, dst_stride, n, pad, S(stream)));
    return DFA_OK;
}

int dfa_transform_points(const float* points, int n, const float aff[12], int with_translation, float* out,
                         dfa_stream_t stream) {
    REQUIRE(n >= 0 && (n == 0 || (points && out)), "bad points");
    REQUIRE(aff, "null transform");
    HIP_TRY(dfa::launch_transform_points(points, n, aff, with_translation != 0, out, S(stream)));
    return DFA_OK;
}

int dfa_compact_points(const float* points, const uint8_t* flags, int N, float* out_points, int32_t* out_index,
                       int32_t* count, dfa_stream_t stream) {
    REQUIRE(count, "count is required");
    REQUIRE(N >= 0 && (N == 0 || flags), "bad flags");
    REQUIRE(!out_points || points || N == 0, "out_points requested without points");
    CompactScratch& chunks = stream_scratch<CompactScratch>(S(stream));
    const size_t n         = (size_t)dfa::compact_chunks(N > 0 ? N : 1);
    HIP_TRY(chunks.reserve(n, n / 4 + 16));
    HIP_TRY(dfa::launch_compact_points(points, flags, N, out_points, out_index, count, chunks.data, S(stream)));
    return DFA_OK;
}

int dfa_correspond(const float* canon_vertices, const float* canon_normals, int n_canon, const float* live_vertices,
                   int n_live, float* out_vertices, float* out_normals, int32_t* out_index, dfa_stream_t stream) {
    REQUIRE(canon_vertices && n_canon > 0, "no canonical vertices");
    REQUIRE(n_live >= 0 && (n_live == 0 || live_vertices), "bad live vertices");
    REQUIRE(!out_normals || canon_normals, "normals requested without canonical normals");
    const dfa::KnnGridView* grid;
    if (n_canon >= 16384 && want_grid(n_canon, n_live)) {  // large cloud: 128^3 point grid
        PointGridScratch& pg = stream_scratch<PointGridScratch>(S(stream));
        HIP_TRY(pg.reserve(n_canon));
        HIP_TRY(dfa::point_grid_build(pg.v, canon_vertices, n_canon, S(stream)));
        grid = &pg.v.g;
    } else if (int rc = scratch_grid(canon_vertices, n_canon, n_live, S(stream), &grid))
        return rc;
    HIP_TRY(dfa::launch_correspond(canon_vertices, canon_normals, n_canon, live_vertices, n_live, out_vertices,
                                   out_normals, out_index, grid, S(stream)));
    return DFA_OK;
}

int dfa_correspond_projective(const float* vertices, const float* normals, int n, const float* vmap, int vmap_step,
                              const float* nmap, int nmap_step, int cols, int rows, float fx, float fy, float cx, float cy,
                              float dist_thresh, float min_cosine, float* out_vertices, float* out_normals,
                              int32_t* out_pixel, dfa_stream_t stream) {
    REQUIRE(n >= 0 && (n == 0 || vertices), "bad vertices");
    REQUIRE(vmap && cols > 0 && rows > 0 && vmap_step >= 16 * cols, "bad vertex map");
    REQUIRE(!nmap || nmap_step >= 16 * cols, "bad normal map pitch");
    REQUIRE(!out_normals || nmap, "normals requested without a normal map");
    REQUIRE(fx > 0.f && fy > 0.f && dist_thresh >= 0.f, "bad intrinsics / threshold");
    REQUIRE(((uintptr_t)vmap & 15) == 0 && (vmap_step & 15) == 0 && ((uintptr_t)nmap & 15) == 0 && (!nmap || (nmap_step & 15) == 0),
            "maps must be 16-byte aligned float4 images");
    HIP_TRY(dfa::launch_correspond_projective(vertices, normals, n, vmap, vmap_step, nmap, nmap_step, cols, rows, fx, fy, cx,
                                              cy, dist_thresh, min_cosine, out_vertices, out_normals, out_pixel,
                                              S(stream)));
    return DFA_OK;
}

}  // extern "C"
