// capi_internal.hpp — what the units of the C ABI layer (capi*.cpp) share: the error state and its macros, the argument
// checks and the node-grid scratch that more than one of them uses.  Host-only; the buffer itself is defined in capi.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/dynfu_amd.h"
#include "kernels.hpp"
#include "device_memory.hpp"
#include "warped_bricks.hpp"

#pragma GCC visibility push(hidden)  // internal to the library: nothing here joins its exported symbols
namespace dfa {
namespace capi {

// ONE per thread for all the units (capi.cpp): what dfa_last_error returns.  __thread, not thread_local: behind an extern
// thread_local the compiler calls an initialisation function that may exist elsewhere, through a weak reference that a
// hidden symbol of a shared library cannot leave unresolved (the call lands on the library's load address)
extern __thread char g_err[512];

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

inline int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorNoDevice ? DFA_ERR_NO_GPU : DFA_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// (a check shared by several public functions reports under the name of the one that was called: `fn`, its __func__)
#define REQUIRE_AS(fn, cond, msg) \
    if (!(cond)) return fail(DFA_ERR_INVALID, "%s: %s", fn, msg)
#define REQUIRE(cond, msg) REQUIRE_AS(__func__, cond, msg)
// (`text` is what a failure reports: a call that moved into a helper keeps the words it failed under before)
#define HIP_TRY_AS(expr, text)                         \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return hip_fail(e_, text); \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(expr, #expr)

inline hipStream_t S(dfa_stream_t s) { return (hipStream_t)s; }

inline bool volume_args_ok(const void* vol, int X, int Y, int Z) { return vol && X > 0 && Y > 0 && Z > 0; }

// The argument checks the four warped integrations open with (dfa_tsdf_integrate_warped, _warped6 and their _field forms), in
// one order and one wording, under the called function's name.  reference_mode: vol2cam belongs to the parameter block and k
// goes up to DFA_MAX_KNN; otherwise (north-star) vol2cam is not looked at and k goes up to 8.
inline int warped_args_ok(const char* fn, bool reference_mode, const uint16_t* dists, int dists_step, int cols, int rows,
                          const uint32_t* volume, int X, int Y, int Z, const float* voxel_size, const float* vol2cam,
                          float trunc_dist, int max_weight, const float* node_pos, const float* node_dq, const float* node_w, int D,
                          int k, int unsupported_mode) {
    REQUIRE_AS(fn, volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE_AS(fn, dists && cols > 0 && rows > 0 && dists_step >= cols * 2, "bad dists image");
    REQUIRE_AS(fn, voxel_size && (vol2cam || !reference_mode), "null parameter block");
    REQUIRE_AS(fn, trunc_dist > 0.f, "trunc_dist must be positive");
    REQUIRE_AS(fn, max_weight >= 0 && max_weight <= 65535, "max_weight must fit the 16-bit weight");
    REQUIRE_AS(fn, D >= 0, "negative node count");
    REQUIRE_AS(fn, D == 0 || (node_pos && node_dq && node_w), "nodes without positions, transforms or radii");
    REQUIRE_AS(fn, k >= 1 && k <= (reference_mode ? DFA_MAX_KNN : 8), reference_mode ? "k out of range 1..16" : "k out of range 1..8");
    REQUIRE_AS(fn, unsupported_mode == DFA_WARPED_SKIP || unsupported_mode == DFA_WARPED_RIGID, "unknown unsupported_mode");
    return DFA_OK;
}

// device scratch of one uniform grid (knn_grid.hip): the node grid of the k-NN searches and, with more cells, the grid part
// of dfa_correspond's point grid.  (Declared in a named namespace: stream_scratch<GridScratch> is ONE table per process,
// whichever unit asks for it; a type of an anonymous namespace would be another type, and another grid, in every unit.)
struct GridScratch {
    DeviceBuffer<dfa::KnnGridDesc> desc;
    DeviceBuffer<int32_t> cell_count, cell_start, node_cell;
    DeviceBuffer<float4> sorted;
    dfa::KnnGridView v{};  // the buffers as the kernels take them
    void release() {
        desc.release(), cell_count.release(), cell_start.release(), node_cell.release(), sorted.release();
        v = dfa::KnnGridView{};
    }
    hipError_t reserve(size_t cells, size_t points, size_t headroom) {
        hipError_t e;
        if ((e = desc.reserve(1)) || (e = cell_count.reserve(cells)) || (e = cell_start.reserve(cells + 1)) ||
            (e = node_cell.reserve(points, headroom)) || (e = sorted.reserve(points, headroom)))
            release();  // (nothing half-allocated stays behind a failure)
        else v = dfa::KnnGridView{desc.data, cell_count.data, cell_start.data, node_cell.data, sorted.data};
        return e;
    }
    // a warp field grows by a few nodes per frame: a quarter of headroom, so that growing (hipFree waits for the
    // device, and a fresh hipMalloc costs milliseconds) happens a handful of times in a sequence, not every frame
    hipError_t reserve(int D) { return reserve(dfa::KNN_GRID_MAX_CELLS, (size_t)D, (size_t)D / 4 + 64); }
};

// exhaustive scan below this many distance evaluations (grid build = 4 small launches)
// the uniform-grid k-NN (three small launches to build, ~40 us) against the exhaustive scan: worth it for many queries, and for
// ANY number of queries over a large node set — a dozen new nodes against 8.5 k existing ones is one workgroup scanning them
// all, 0.86 ms in the adaptor's 512^3 sequence
inline bool want_grid(int D, long n_query) { return D >= 64 && ((long)D * n_query >= (1L << 22) || D >= 1024); }

// the grid of a search over D points where it pays (built in the stream's scratch), null where the exhaustive scan does
inline int scratch_grid(const float* pos, int D, long n_query, hipStream_t st, const dfa::KnnGridView** grid) {
    *grid = nullptr;
    if (!want_grid(D, n_query)) return DFA_OK;
    GridScratch& gs = stream_scratch<GridScratch>(st);
    HIP_TRY(gs.reserve(D));
    HIP_TRY(dfa::knn_grid_build(gs.v, pos, D, st));
    *grid = &gs.v;
    return DFA_OK;
}

// the search of the warped integrations and of the k-NN field (every voxel of a brick searches): the node grid for 64 nodes
// and more — wherever it is exact and cheaper than a scan of all the nodes —, built in the stream's scratch; null: the scan
inline int warped_node_grid(const float* node_pos, int D, hipStream_t st, const dfa::KnnGridView** grid) {
    *grid = nullptr;
    if (D >= 64) {
        GridScratch& gs = stream_scratch<GridScratch>(st);
        HIP_TRY(gs.reserve(D));
        HIP_TRY(dfa::knn_grid_build(gs.v, node_pos, D, st));
        *grid = &gs.v;
    }
    return DFA_OK;
}

// scratch of dfa_tsdf_integrate_warped and dfa_tsdf_integrate_warped6: the brick flags of the support pre-pass and the largest node radius
struct WarpedScratch {
    DeviceBuffer<uint8_t> bricks;
    DeviceBuffer<float> wmax;
};

// behind the argument checks of both warped integrations: the stream's WarpedScratch at the volume's size and, for 64 nodes
// and more, the node grid.  Every voxel of a marked brick searches: the grid wherever it is exact and cheaper than a scan of
// all the nodes (null: the scan)
inline int warped_scratch(int X, int Y, int Z, const float* node_pos, int D, dfa_stream_t stream, WarpedScratch** scratch,
                   const dfa::KnnGridView** grid) {
    WarpedScratch& ws = stream_scratch<WarpedScratch>(S(stream));
    // (the words this reservation failed under while the count had a name of its own)
    HIP_TRY_AS(ws.bricks.reserve(dfa::knn_field_bricks(X, Y, Z)), "ws.bricks.reserve(dfa::warped_brick_count(X, Y, Z))");
    HIP_TRY(ws.wmax.reserve(1));
    *scratch = &ws;
    return warped_node_grid(node_pos, D, S(stream), grid);
}

// behind the field list of a plan: the arena's first failure as the C ABI reports it
inline int plan_status(const dfa::PlanArena& mem) { return mem.ok() ? DFA_OK : hip_fail(mem.error, mem.what); }
inline int plan_grid(GridScratch& grid, int max_D) {
    const hipError_t e = grid.reserve(max_D);
    return e == hipSuccess ? DFA_OK : hip_fail(e, "hipMalloc (node grid)");
}

// the sum of a plan's per-row count array (D device ints, D > 0), read back with a blocking copy
inline hipError_t row_count_sum(const int32_t* counts, int D, long long* sum) {
    std::vector<int32_t> cnt((size_t)D);
    const hipError_t e = hipMemcpy(cnt.data(), counts, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (int32_t c : cnt) *sum += c;
    return e;
}

}  // namespace capi
}  // namespace dfa
#pragma GCC visibility pop
