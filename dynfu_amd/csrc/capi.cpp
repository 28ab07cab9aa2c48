// capi.cpp — the C ABI declared in include/dynfu_amd.h: argument checking, error strings, the scratch each entry point
// keeps per stream, the two solver plans (their field lists, graphs and timing brackets) and the per-frame launch
// sequences.  What owns memory is in device_memory.hpp, the north-star launch budget in launch_budget.hpp; no arithmetic
// lives here, and the kernels are in the .hip files.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <new>
#include <vector>

#include "../../include/dynfu_amd.h"
#include "kernels.hpp"
#include "dev_switch.hpp"
#include "device_memory.hpp"
#include "launch_budget.hpp"
#include "solve.hpp"
#include "solve6.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(e == hipErrorNoDevice ? DFA_ERR_NO_GPU : DFA_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

#define REQUIRE(cond, msg) \
    if (!(cond)) return fail(DFA_ERR_INVALID, "%s: %s", __func__, msg)
#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t e_ = (expr);                        \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

inline hipStream_t S(dfa_stream_t s) { return (hipStream_t)s; }

bool volume_args_ok(const void* vol, int X, int Y, int Z) { return vol && X > 0 && Y > 0 && Z > 0; }

using dfa::DeviceBuffer;
using dfa::stream_scratch;

// device scratch of one uniform grid (warp.hip): the node grid of the k-NN searches and, with more cells, the grid part
// of dfa_correspond's point grid
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
struct IcpScratch : DeviceBuffer<float> {};        // partial sums of dfa_icp_sums
// scratch of dfa_tsdf_integrate_warped and dfa_tsdf_integrate_warped6: the brick flags of the support pre-pass and the largest node radius
struct WarpedScratch {
    DeviceBuffer<uint8_t> bricks;
    DeviceBuffer<float> wmax;
};
struct CompactScratch : DeviceBuffer<int32_t> {};  // chunk counts of dfa_compact_points

// exhaustive scan below this many distance evaluations (grid build = 4 small launches)
// the uniform-grid k-NN (three small launches to build, ~40 us) against the exhaustive scan: worth it for many queries, and for
// ANY number of queries over a large node set — a dozen new nodes against 8.5 k existing ones is one workgroup scanning them
// all, 0.86 ms in the adaptor's 512^3 sequence
bool want_grid(int D, long n_query) { return D >= 64 && ((long)D * n_query >= (1L << 22) || D >= 1024); }

// the grid of a search over D points where it pays (built in the stream's scratch), null where the exhaustive scan does
int scratch_grid(const float* pos, int D, long n_query, hipStream_t st, const dfa::KnnGridView** grid) {
    *grid = nullptr;
    if (!want_grid(D, n_query)) return DFA_OK;
    GridScratch& gs = stream_scratch<GridScratch>(st);
    HIP_TRY(gs.reserve(D));
    HIP_TRY(dfa::knn_grid_build(gs.v, pos, D, st));
    *grid = &gs.v;
    return DFA_OK;
}

}  // namespace

struct dfa_solver {
    int max_D, max_N, k;
    size_t max_R;
    int ell_cap;
    dfa::SolveView v;          // pointers into `mem`
    dfa::SolveState* state;    // device
    double* cost_partials;     // device
    unsigned int* ticket;      // device: arrival counter of the linearise kernel (self re-arming)
    dfa::PlanArena mem;         // every hipMalloc and pinned block of this plan
    GridScratch grid;           // node grid of the current problem
    bool has_problem;
    bool timing;
    dfa::EventPool ev;               // timing events, in begin / end pairs: they accumulate from enable_timing(1) on
    std::vector<int> ev_pcg, ev_asm; // indices of the begin events of each bracketed launch
    int timed_solves = 0;
    dfa::MbGraphCache mb_graphs;  // HIP graphs of the many-workgroup PCG's launch chunks
    dfa::TeamPcg team;            // host side of the team PCG (plans of 2 049 nodes up to solve_team_pcg_fits: 19 584;
                                  // rows longer than J x 20 entries make the first launch give up and the plan fall back)
    bool deterministic = false;  // order-stable variant (dfa_solver_set_deterministic), applied by the next set_problem
    bool just_reset = false;  // the unknowns and the state block were zeroed by set_problem and not touched since
    bool graph_rows = false;  // the last set_problem built graphs and rows with the fused launch (solve_build_graph_rows)
    long long* iters_total = nullptr;  // device: PCG iterations of all solves since enable_timing(1)
    dfa_overlap_fn overlap_fn = nullptr;  // called behind the first assembly launch of every solve
    void* overlap_user        = nullptr;
    int* host_flag = nullptr;        // pinned int[4]: stop flag of the many-workgroup PCG, the plan's converged flag, (skip), iterations;
                                     // read back between launch chunks
};

struct dfa_solver6 {
    int max_D, max_N, k;
    dfa::Solve6View v;
    dfa::Solve6State* state;
    float* raw_w;       // N x k un-normalised weights of the k-NN pass
    int32_t* raw_reg;   // D x (k + 1)
    const float* node_dq;  // borrowed: transforms at set_problem time
    dfa::PlanArena mem;
    GridScratch grid;
    bool has_problem;
    // the PCG of one Gauss-Newton iteration (linear_iter + 2 dependent launches) captured as a HIP graph:
    // re-captured when the problem size or the iteration parameters change
    std::map<int, hipGraphExec_t> pcg_graphs;  // by the number of step launches
    int last_launches = 0;  // step launches enqueued by the last solve
    dfa::LaunchBudget budget;                  // dfa_solve6_params.adaptive_launch (launch_budget.hpp)
    int* mirror = nullptr;                     // pinned int[S6_RING][S6_HIST]: the device's counts, solve n in slot n % S6_RING
    hipEvent_t done_ev[dfa::S6_RING] = {};     // end of solve n, n % S6_RING
    bool graph_disabled = false;
    hipStream_t capture_stream = nullptr;  // capture is not allowed on the legacy default stream
    bool timing = false;  // hipEvent brackets around linearise / assemble / PCG of every Gauss-Newton iteration
    dfa::EventPool ev;  // 4 per Gauss-Newton iteration
    int pcg_key_D = -1;  // node count the captured PCG graphs were recorded for
};

namespace {
// a begin / end pair of timing events: the begin event's index, recorded on st (-1: no events, the bracket is not taken)
int bracket_open(dfa_solver* s, hipStream_t st) {
    const int idx = s->timing ? s->ev.take(2) : -1;
    if (idx >= 0) (void)hipEventRecord(s->ev.events[idx], st);
    return idx;
}

// behind the field list of a plan: the arena's first failure as the C ABI reports it
int plan_status(const dfa::PlanArena& mem) { return mem.ok() ? DFA_OK : hip_fail(mem.error, mem.what); }
int plan_grid(GridScratch& grid, int max_D) {
    const hipError_t e = grid.reserve(max_D);
    return e == hipSuccess ? DFA_OK : hip_fail(e, "hipMalloc (node grid)");
}
}  // namespace

extern "C" {

const char* dfa_last_error(void) { return g_err; }

const char* dfa_version(void) { return "dynfu_amd 0.1 (gfx950, HIP)"; }

int dfa_abi_version(void) { return DFA_ABI_VERSION; }

size_t dfa_abi_struct_size(int id) {
    switch (id) {
        case DFA_STRUCT_SOLVE_PARAMS: return sizeof(dfa_solve_params);
        case DFA_STRUCT_SOLVE_STATS: return sizeof(dfa_solve_stats);
        case DFA_STRUCT_SOLVE_TIMING: return sizeof(dfa_solve_timing);
        case DFA_STRUCT_SOLVE6_PARAMS: return sizeof(dfa_solve6_params);
        case DFA_STRUCT_SOLVE6_STATS: return sizeof(dfa_solve6_stats);
        case DFA_STRUCT_SOLVE6_TIMING: return sizeof(dfa_solve6_timing);
        default: return 0;
    }
}

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

int dfa_marching_cubes_indexed(const uint32_t* volume, const uint8_t* occupancy, int X, int Y, int Z, const float cell_size[3],
                               const int32_t* tri_table, const int32_t* num_verts_table, float* out_vertices,
                               int max_vertices, int32_t* out_indices, int max_indices, int32_t* totals,
                               dfa_stream_t stream) {
    REQUIRE(volume && X >= 2 && Y >= 2 && Z >= 2, "bad volume");
    REQUIRE(cell_size && tri_table && num_verts_table, "null parameter block / case tables");
    REQUIRE(max_vertices >= 0 && (max_vertices == 0 || out_vertices), "bad vertex buffer");
    REQUIRE(max_indices >= 0 && (max_indices == 0 || out_indices), "bad index buffer");
    REQUIRE(((uintptr_t)out_vertices & 15) == 0, "out_vertices must be 16-byte aligned");
    REQUIRE(totals, "null totals");
    REQUIRE((long)X * Y * Z / 64 < (1L << 31), "volume too large");
    const long nsegs = dfa::mci_segments(X, Y, Z);
    McIndexedScratch& scratch = stream_scratch<McIndexedScratch>(S(stream));
    HIP_TRY(scratch.reserve(nsegs));
    HIP_TRY(dfa::launch_marching_cubes_indexed(volume, X, Y, Z, cell_size, tri_table, num_verts_table, out_vertices,
                                               max_vertices, out_indices, max_indices, totals, scratch.vert.seg_off.data,
                                               scratch.idx_off.data, scratch.vert.chunk_sums.data, occupancy, S(stream)));
    return DFA_OK;
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

int dfa_mc_default_tables(int32_t* tri_table, int32_t* num_verts_table) {
    REQUIRE(tri_table && num_verts_table, "null table");
    dfa::mc_default_tables(tri_table, num_verts_table);
    return DFA_OK;
}

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

int dfa_tsdf_integrate_warped(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                              uint8_t* occupancy, const float voxel_size[3], float trunc_dist, int max_weight,
                              const float vol2cam[12], float fx, float fy, float cx, float cy, const float* node_pos,
                              const float* node_dq, const float* node_w, int D, int k, int unsupported_mode,
                              dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(dists && cols > 0 && rows > 0 && dists_step >= cols * 2, "bad dists image");
    REQUIRE(voxel_size && vol2cam, "null parameter block");
    REQUIRE(trunc_dist > 0.f, "trunc_dist must be positive");
    REQUIRE(max_weight >= 0 && max_weight <= 65535, "max_weight must fit the 16-bit weight");
    REQUIRE(D >= 0, "negative node count");
    REQUIRE(D == 0 || (node_pos && node_dq && node_w), "nodes without positions, transforms or radii");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    REQUIRE(unsupported_mode == DFA_WARPED_SKIP || unsupported_mode == DFA_WARPED_RIGID, "unknown unsupported_mode");
    const bool rigid = unsupported_mode == DFA_WARPED_RIGID;
    if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
    WarpedScratch& ws = stream_scratch<WarpedScratch>(S(stream));
    HIP_TRY(ws.bricks.reserve(dfa::warped_brick_count(X, Y, Z)));
    HIP_TRY(ws.wmax.reserve(1));
    // every voxel of a marked brick searches: the grid wherever it is exact and cheaper than a scan of all the nodes
    const dfa::KnnGridView* grid = nullptr;
    if (D >= 64) {
        GridScratch& gs = stream_scratch<GridScratch>(S(stream));
        HIP_TRY(gs.reserve(D));
        HIP_TRY(dfa::knn_grid_build(gs.v, node_pos, D, S(stream)));
        grid = &gs.v;
    }
    HIP_TRY(dfa::launch_tsdf_integrate_warped(dists, dists_step, cols, rows, volume, X, Y, Z, occupancy, voxel_size, trunc_dist,
                                              max_weight, vol2cam, fx, fy, cx, cy, node_pos, node_dq, node_w, D, k, rigid, grid,
                                              ws.bricks.data, ws.wmax.data, S(stream)));
    return DFA_OK;
}

int dfa_tsdf_integrate_warped6(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* volume, int X, int Y, int Z,
                               uint8_t* occupancy, const float voxel_size[3], float trunc_dist, int max_weight,
                               const float vol2node[12], const float node2cam[12], float fx, float fy, float cx, float cy,
                               const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                               int unsupported_mode, dfa_stream_t stream) {
    REQUIRE(volume_args_ok(volume, X, Y, Z), "bad volume");
    REQUIRE(dists && cols > 0 && rows > 0 && dists_step >= cols * 2, "bad dists image");
    REQUIRE(voxel_size, "null parameter block");
    REQUIRE(trunc_dist > 0.f, "trunc_dist must be positive");
    REQUIRE(max_weight >= 0 && max_weight <= 65535, "max_weight must fit the 16-bit weight");
    REQUIRE(D >= 0, "negative node count");
    REQUIRE(D == 0 || (node_pos && node_dq && node_w), "nodes without positions, transforms or radii");
    REQUIRE(k >= 1 && k <= 8, "k out of range 1..8");
    REQUIRE(unsupported_mode == DFA_WARPED_SKIP || unsupported_mode == DFA_WARPED_RIGID, "unknown unsupported_mode");
    float node2vol[12], stretch, tmax;
    REQUIRE(dfa::warped6_frame(vol2node, node2vol, &stretch, &tmax), "vol2node must be rigid");
    const bool rigid = unsupported_mode == DFA_WARPED_RIGID;
    if (D == 0 && !rigid) return DFA_OK;  // no node supports anything: every voxel is left alone
    WarpedScratch& ws = stream_scratch<WarpedScratch>(S(stream));
    HIP_TRY(ws.bricks.reserve(dfa::warped_brick_count(X, Y, Z)));
    HIP_TRY(ws.wmax.reserve(1));
    const dfa::KnnGridView* grid = nullptr;  // (as dfa_tsdf_integrate_warped)
    if (D >= 64) {
        GridScratch& gs = stream_scratch<GridScratch>(S(stream));
        HIP_TRY(gs.reserve(D));
        HIP_TRY(dfa::knn_grid_build(gs.v, node_pos, D, S(stream)));
        grid = &gs.v;
    }
    HIP_TRY(dfa::launch_tsdf_integrate_warped6(dists, dists_step, cols, rows, volume, X, Y, Z, occupancy, voxel_size, trunc_dist,
                                               max_weight, vol2node, node2cam, node2vol, stretch, tmax, fx, fy, cx, cy, node_pos,
                                               node_dq, node_w, D, k, rigid, grid, ws.bricks.data, ws.wmax.data, S(stream)));
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

// ------------------------------------------------------------------------------- solver seam

int dfa_solver_create(int max_D, int max_N, int k, dfa_solver** out) {
    REQUIRE(out, "null out");
    *out = nullptr;
    REQUIRE(max_D > 0 && max_N >= 0, "bad sizes");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    REQUIRE(max_D <= dfa::solve_pcg_max_nodes(), "more nodes than a plan supports (32768)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DFA_ERR_NO_GPU, "no HIP device");
    dfa_solver* s = new (std::nothrow) dfa_solver();
    REQUIRE(s, "out of host memory");
    s->max_D = max_D, s->max_N = max_N, s->k = k;
    s->max_R       = (size_t)max_N + (size_t)max_D * k;
    s->ell_cap     = 256;
    s->has_problem = false;
    s->timing      = false;
    {
        // (the one environment variable of the product library, read once per plan: the order-stable assembly for a caller
        // that cannot reach dfa_solver_set_deterministic — include/dynfu_amd.h)
        const char* e    = getenv("DFA_ASSEMBLE_DETERMINISTIC");
        s->deterministic = e && atoi(e) != 0;
    }
    std::memset(&s->v, 0, sizeof(s->v));
    const size_t R = s->max_R, D = (size_t)max_D;
    dfa::PlanArena& mem = s->mem;
#define A(field, count) mem.alloc(&s->v.field, (count))
    A(ridx, R * k);
    A(rw, R * k);
    A(rtau, R);
    A(rb, R * 3);
    A(re, R * (size_t)dfa::solve_rec_words(k));
    A(reg_idx, D * k);
    A(blk_hist, D * (dfa::SOLVE_TG_BLOCKS + 1));
    A(node_ptr, D + 1);
    A(node_list, R * k);
    A(ell, D * s->ell_cap);
    A(ell_cnt, D);
    A(diag, D);
    A(g, D * 3);
    A(g_base, D * 3);
    A(t_base, D * 3);
    A(pk_perm, D);
    A(pk_perm2, D);
    A(pk_vals, D * s->ell_cap);
    A(pk_cols, D * s->ell_cap);
    A(mb_x, D);
    A(mb_r, D);
    A(mb_p, D);
    A(mb_s, D);
    A(mb_w, D);
    A(mb_u[0], D);
    A(mb_u[1], D);
    A(mb_m[0], D);
    A(mb_m[1], D);
    A(mb_t[0], D);
    A(mb_t[1], D);
    A(mb_gpart[0], (size_t)dfa::solve_mb_blocks(max_D));
    A(mb_gpart[1], (size_t)dfa::solve_mb_blocks(max_D));
    A(mb_dpart[0], (size_t)dfa::solve_mb_blocks(max_D));
    A(mb_dpart[1], (size_t)dfa::solve_mb_blocks(max_D));
    A(t, D * 3);
    A(huber, D);
    A(node_dq_out, D * 8);
#undef A
    int rc = plan_status(mem);
    if (rc == DFA_OK) rc = plan_grid(s->grid, max_D);
    // (plans of up to 2 048 nodes solve in the register-resident kernels: no team buffers for them outside development builds)
    if (rc == DFA_OK && dfa::solve_team_pcg_fits(max_D) && (max_D > 2048 || dfa::kDevAB)) {
        // team PCG: control block and flag words (zeroed once: barrier rounds grow; the words are cleared again only where
        // the rounds would wrap), exchange buffer, the pinned abort count
        s->v.team_stride = (max_D + 3) & ~3;
        const size_t areas = (size_t)3 * dfa::solve_team_pcg_rounds();  // an area per barrier round and coordinate (50 MB at 8 k nodes)
        mem.alloc(&s->v.team_ctl, 1, true);
        mem.alloc(&s->v.team_mt, areas * s->v.team_stride, true);
        mem.alloc(&s->v.team_words, dfa::solve_team_pcg_words(), true);
        s->team.host_abort = mem.pinned<int>(1);
        if ((rc = plan_status(mem)) == DFA_OK && !s->team.host_abort) rc = fail(DFA_ERR_HIP, "hipHostMalloc (team PCG abort count)");
        if (rc == DFA_OK) {
            s->team.ctl = s->v.team_ctl;
            // (development builds: DFA_MB_TEAM_EPOCH = the first barrier round, e.g. just below 2^32 for the wrap's test)
            if (const char* e0 = dfa::dev_env("DFA_MB_TEAM_EPOCH")) s->team.epoch = (unsigned)std::strtoul(e0, nullptr, 0);
        }
    }
    if (rc == DFA_OK) {
        mem.alloc(&s->state, 1);
        mem.alloc(&s->iters_total, 1, true);
        s->host_flag = mem.pinned<int>(4);  // (none: the solve does without the read-backs)
        // (per linearise workgroup, at most 1024 of them: its share of the energy; behind those its largest matrix addend)
        mem.alloc(&s->cost_partials, std::max<size_t>((R + 255) / 256 + 1, 1024) + 1024);
        mem.alloc(&s->ticket, 64, true);
        rc = plan_status(mem);
    }
    if (rc != DFA_OK) {
        dfa_solver_destroy(s);
        return rc;
    }
    *out = s;
    return DFA_OK;
}

void dfa_solver_destroy(dfa_solver* s) {
    if (!s) return;
    s->grid.release();
    s->mb_graphs.release();
    delete s;  // (the arena frees the plan's memory, the pool its events)
}

int dfa_solver_set_problem(dfa_solver* s, const float* node_pos, const float* node_dq, const float* node_w, int D,
                           const float* canon_vertices, const float* canon_normals, const float* live_vertices,
                           const float* live_normals, int N, dfa_stream_t stream) {
    (void)canon_normals;
    (void)live_normals;  // declared by energy.t:28-31, never read by an Energy term
    REQUIRE(s, "null plan");
    REQUIRE(node_pos && node_dq && node_w && D > 0, "no nodes");
    REQUIRE(N >= 0 && (N == 0 || (canon_vertices && live_vertices)), "bad vertex arrays");
    if (D > s->max_D || N > s->max_N)
        return fail(DFA_ERR_CAPACITY, "dfa_solver_set_problem: D=%d N=%d exceed the plan (max_D=%d max_N=%d)", D, N,
                    s->max_D, s->max_N);
    dfa::SolveView& v = s->v;
    v.N = N, v.D = D, v.k = s->k, v.Dpad = (D + 3) & ~3, v.ell_cap = s->ell_cap;
    v.deterministic = s->deterministic ? 1 : 0;
    v.node_pos = node_pos, v.node_dq = node_dq, v.node_w = node_w;
    v.canon = canon_vertices, v.live = live_vertices;
    hipStream_t st = S(stream);
    // initializeDataGraph (opt_solver.cpp:56-72): rows [0, N) = k-NN of the canonical vertices + RBF weights
    const dfa::KnnGridView* grid = nullptr;
    // (development builds: DFA_GRAPH_GRID=1 puts the nodes of ANY problem in the grid — the tests of the fused graph build
    // reach its branches with a few dozen nodes)
    if (want_grid(D, (long)N + D) || dfa::dev_env_int("DFA_GRAPH_GRID", 0) != 0) {
        HIP_TRY(dfa::knn_grid_build(s->grid.v, node_pos, D, st));
        grid = &s->grid.v;
    }
    s->graph_rows = grid && dfa::solve_graph_rows_fits(v);
    if (s->graph_rows) {
        // both searches, the rows and the reset as one launch, then the transposition: the same bits as the sequence below
        HIP_TRY(dfa::solve_build_graph_rows(v, *grid, s->state, s->ticket, 64, st));
    } else {
        if (N > 0) HIP_TRY(dfa::launch_knn(node_pos, node_w, D, canon_vertices, N, s->k, v.ridx, v.rw, grid, st));
        // initializeRegGraph (:74-105): k-NN of every node among the nodes (itself included at distance 0)
        HIP_TRY(dfa::launch_knn(node_pos, node_w, D, node_pos, D, s->k, v.reg_idx, nullptr, grid, st));
        // rows + transposition; resetGPUMemory (:149-202): unknowns start at zero (same launch as the row set-up)
        HIP_TRY(dfa::solve_build_graph(v, s->state, s->ticket, 64, st));
    }
    s->has_problem = true;
    s->just_reset  = true;
    return DFA_OK;
}

int dfa_solver_set_deterministic(dfa_solver* s, int on) {
    REQUIRE(s, "null plan");
    s->deterministic = on != 0;
    return DFA_OK;
}

int dfa_solver_solve(dfa_solver* s, const dfa_solve_params* p, dfa_stream_t stream) {
    REQUIRE(s && p, "null plan / params");
    REQUIRE(s->has_problem, "set_problem has not been called");
    REQUIRE(p->num_iter >= 0 && p->nonlinear_iter >= 0 && p->linear_iter >= 0, "negative iteration count");
    REQUIRE(p->tukey_offset > 0.f && p->psi_data > 0.f, "tukey_offset / psi_data must be positive");
    REQUIRE(p->lambda >= 0.f && std::isfinite(p->lambda), "lambda must be non-negative and finite");
    const dfa::SolveView& v = s->v;
    hipStream_t st          = S(stream);
    if (!s->just_reset) HIP_TRY(dfa::solve_reset(v, s->state, s->ticket, 64, st));  // (set_problem has just done it)
    s->just_reset = false;
    // w_reg = sqrt(lambda / (D * KNN))  (opt_solver.cpp:30); rows carry tau = w_reg^2
    const double w_reg    = std::sqrt((double)p->lambda / ((double)v.D * (double)v.k));
    const float w_reg_f   = (float)w_reg;
    const float w_reg_sq  = w_reg_f * w_reg_f;
    if (s->timing) s->timed_solves += 1;
    if (s->host_flag) s->host_flag[0] = s->host_flag[1] = 0;
    s->mb_graphs.call = 0;
    int not_launched = 0;  // iterations after the host has seen the converged flag (many-workgroup path only)
    int gn_launched = 0;  // Gauss-Newton iterations whose assembly has been enqueued
    bool huber_done = false;
    const bool big_budget = (long)p->num_iter * p->nonlinear_iter > 8;
    const bool pcg_async  = dfa::solve_pcg_is_async(v, &s->team, p->linear_iter);  // (else the PCG itself reads the flags back)
    const bool no_regradient = dfa::dev_env("DFA_NO_REGRADIENT") != nullptr;  // (development builds: the tests compare both ways)
    // Behind the launch that left this iteration's system (the assembly, or the regradient that stands in for one) in the
    // bracket ev_asm: this iteration's PCG starts here — the caller's chip-wide work may run in its shadow
    auto run_pcg = [&](int ev_asm) -> int {
        if (ev_asm >= 0) {  // close that bracket and book it
            (void)hipEventRecord(s->ev.events[ev_asm + 1], st);
            s->ev_asm.push_back(ev_asm);
        }
        if (s->overlap_fn) s->overlap_fn(s->overlap_user, stream, gn_launched);
        ++gn_launched;
        const int ev = bracket_open(s, st);  // closed behind the solving kernel, before the fallback launch
        HIP_TRY(dfa::solve_pcg(v, s->state, p->linear_iter, p->pcg_tol, s->host_flag, &s->mb_graphs, &s->team,
                               ev >= 0 ? s->ev.events[ev + 1] : nullptr, st));
        if (ev >= 0) s->ev_pcg.push_back(ev);
        return DFA_OK;
    };
    for (int outer = 0; outer < p->num_iter; ++outer) {
        // preNonlinearSolve (opt_solver.cpp:135-140): the Huber weights are only observable after
        // the solve, so they are evaluated for the last outer iteration alone
        // (folded into that iteration's first linearisation; a launch of its own only if that one is never enqueued)
        // converged == 2 (gradient at the floor under stale weights) ended the inner iterations of the outer iteration
        // before only: this one re-weights, and its first linearisation clears the flag on the device
        if (s->host_flag && s->host_flag[1] == 2) s->host_flag[1] = 0;
        int gn_in_outer = 0;  // iterations of this outer iteration enqueued (the device's flag is current behind them)
        for (int gn = 0; gn < p->nonlinear_iter; ++gn) {
            // Iteration budgets like the reference's (24 x 16, dyn_fusion.cpp:183-189) are ~380 iterations of which a
            // handful do anything: behind a converged one the kernels return at entry, but 4 launches x 5 us x 380 is
            // still 8 ms of stream time.  Small budgets (<= 8 iterations: bench.py's 5) stay free of any host
            // synchronisation; larger ones read the `converged` flag back every 4th iteration (plans whose PCG does not
            // synchronise by itself: the register-resident kernels and the team form).
            if (big_budget && gn_in_outer >= 4 && gn_in_outer % 4 == 0 && s->host_flag && !s->host_flag[1] && pcg_async) {
                HIP_TRY(hipMemcpyAsync(&s->host_flag[1], &s->state->converged, sizeof(int), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            if (s->host_flag && s->host_flag[1]) {  // t can no longer change (in this outer iteration, when the flag is
                ++not_launched;                     // 2): every further iteration is a no-op
                continue;
            }
            ++gn_in_outer;
            // An inner iteration (frozen robust weights: linear least squares) restarts the PCG on the true residual of
            // the SAME matrix, g = g_base - A (t - t_base): one sparse product instead of a linearisation and an assembly
            // (the reference's budget is 16 inner iterations per re-weighting).  With a cost-decrease tolerance the cost
            // of every iteration is wanted: the long way.  Without the regulariser (lambda = 0: the reference's OptTests,
            // fewer vertices than nodes) the matrix is singular, and the cancellation in g_base - A (t - t_base) leaves
            // round-off in its null space, which CG then amplifies (a re-linearised gradient is J^T of something and has
            // none; measured: two of the eight OptTest scenes leave their 1e-3 tolerance): the long way as well.
            // DFA_NO_REGRADIENT=1: the long way always (A/B).
            if (gn > 0 && p->gn_tol == 0.f && p->lambda > 0.f && !no_regradient) {
                const int ev = bracket_open(s, st);  // booked with the assemblies: it stands in for one
                HIP_TRY(dfa::solve_regradient(v, s->state, st));
                if (int rc = run_pcg(ev)) return rc;
                continue;
            }
            const bool with_huber = gn == 0 && outer == p->num_iter - 1;
            HIP_TRY(dfa::solve_linearise(v, s->state, s->cost_partials, s->ticket, gn == 0, gn == 0 ? 0 : 1,
                                         p->gn_tol, p->tukey_offset, p->psi_data, w_reg_sq, with_huber ? p->psi_reg : 0.f, nullptr, st));
            huber_done |= with_huber;
            const int ev = bracket_open(s, st);
            HIP_TRY(dfa::solve_assemble(v, s->state, gn == 0 && p->nonlinear_iter > 1, w_reg_sq, st));
            if (int rc = run_pcg(ev)) return rc;
        }
    }
    if (s->overlap_fn && gn_launched == 0) s->overlap_fn(s->overlap_user, stream, -1);  // no iteration ran: the caller's work still goes out
    if (not_launched) HIP_TRY(dfa::solve_count_noop(s->state, not_launched, st));
    // final cost at the solved t; weights re-evaluated only if no iteration ever did
    const bool no_weights = p->num_iter == 0 || p->nonlinear_iter == 0;
    if (!huber_done) HIP_TRY(dfa::solve_huber(v, p->psi_reg, st));  // no outer iteration, or the host stopped launching before the last
    HIP_TRY(dfa::solve_linearise(v, s->state, s->cost_partials, s->ticket, no_weights ? 1 : 0, 2, 0.f,
                                 p->tukey_offset, p->psi_data, w_reg_sq, 0.f, s->timing ? s->iters_total : nullptr, st));
    // (postSingleSolve -> copyResultToCPUFromFloat3, opt_solver.cpp:133,270-285: composed once, by that same launch)
    return DFA_OK;
}

int dfa_solver_set_overlap_callback(dfa_solver* s, dfa_overlap_fn fn, void* user) {
    REQUIRE(s, "null plan");
    s->overlap_fn = fn, s->overlap_user = user;
    return DFA_OK;
}

const float* dfa_solver_translations(const dfa_solver* s) { return s ? s->v.t : nullptr; }
const float* dfa_solver_node_dq(const dfa_solver* s) { return s ? s->v.node_dq_out : nullptr; }
const float* dfa_solver_tukey_weights(const dfa_solver* s) { return s ? s->v.rtau : nullptr; }
const float* dfa_solver_huber_weights(const dfa_solver* s) { return s ? s->v.huber : nullptr; }
const int32_t* dfa_solver_data_graph(const dfa_solver* s) { return s ? s->v.ridx : nullptr; }
const int32_t* dfa_solver_reg_graph(const dfa_solver* s) { return s ? s->v.reg_idx : nullptr; }
const float* dfa_solver_matrix_entries(const dfa_solver* s) { return s ? (const float*)s->v.ell : nullptr; }
const int32_t* dfa_solver_matrix_row_lengths(const dfa_solver* s) { return s ? s->v.ell_cnt : nullptr; }
const float* dfa_solver_gradient(const dfa_solver* s) { return s ? s->v.g : nullptr; }

int dfa_solver_warp_to_live(dfa_solver* s, const float* normals, float* out_vertices, float* out_normals,
                            dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(out_vertices || s->v.N == 0, "null output");
    HIP_TRY(dfa::launch_warp_graph(s->v.node_pos, s->v.node_dq_out, s->v.node_w, s->k, s->v.ridx, s->v.canon, normals,
                                   s->v.N, out_vertices, out_normals, S(stream)));
    return DFA_OK;
}

int dfa_solver_get_stats(dfa_solver* s, dfa_solve_stats* host_out, dfa_stream_t stream) {
    REQUIRE(s && host_out, "null plan / out");
    dfa::SolveState h;
    HIP_TRY(hipMemcpyAsync(&h, s->state, sizeof(h), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    host_out->initial_cost = h.initial_cost;
    host_out->final_cost   = h.final_cost;
    host_out->gn_iters     = h.gn_iters;
    host_out->pcg_iters    = h.pcg_iters;
    host_out->max_row_nnz  = h.max_row_nnz;
    host_out->gn_noop      = h.gn_noop;
    if (dfa::dev_env("DFA_PCG_PROFILE_PRINT"))
        fprintf(stderr, "pcg phase cycles: spmv %lld  red_pAp %lld  update %lld  red_rz %lld  p_update+barrier %lld  loop %lld  (iters %d)\n",
                h.prof[0], h.prof[1], h.prof[2], h.prof[3], h.prof[4], h.prof[5], h.pcg_iters);
    if (dfa::dev_env("DFA_PCG_PROFILE_PRINT"))
        fprintf(stderr, "assemble block 7 cycles: init %lld  list+hash %lld  reduce+barrier %lld  compact %lld   (raw prof[6] %lld prof[7] %lld)\n",
                h.prof[6] / 1000000, h.prof[6] % 1000000, h.prof[7] / 1000000, h.prof[7] % 1000000, h.prof[6], h.prof[7]);
    if (h.overflow)
        return fail(DFA_ERR_CAPACITY, "normal-matrix row wider than the plan's ELL capacity (%d > %d)", h.max_row_nnz,
                    s->ell_cap);
    return DFA_OK;
}

int dfa_solver_enable_timing(dfa_solver* s, int enable) {
    REQUIRE(s, "null plan");
    s->timing = enable != 0;
    if (enable == 1) {  // a new measurement: forget the brackets collected so far (2 = resume, keeps them)
        s->ev.rewind(), s->timed_solves = 0;
        s->ev_pcg.clear(), s->ev_asm.clear();
        if (s->iters_total) HIP_TRY(hipMemset(s->iters_total, 0, sizeof(long long)));
    }
    return DFA_OK;
}

int dfa_solver_team_pcg_info(dfa_solver* s, int* launches, int* aborts, int* disabled) {
    REQUIRE(s, "null plan");
    if (launches) *launches = (int)std::min<long>(s->team.launches, 0x7fffffffL);
    if (aborts) *aborts = s->team.host_abort ? *(volatile int*)s->team.host_abort : 0;
    if (disabled) *disabled = (!s->team.ctl || s->team.disabled) ? 1 : 0;
    return DFA_OK;
}

int dfa_solver_get_timing(dfa_solver* s, dfa_solve_timing* out, dfa_stream_t stream) {
    REQUIRE(s && out, "null plan / out");
    HIP_TRY(hipStreamSynchronize(S(stream)));
    std::memset(out, 0, sizeof(*out));
    for (const std::vector<int>* brackets : {&s->ev_pcg, &s->ev_asm})
        for (int idx : *brackets) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ev.events[idx], s->ev.events[idx + 1]));
            (brackets == &s->ev_pcg ? out->pcg_ms : out->assemble_ms) += ms;
        }
    out->pcg_launches      = (int)s->ev_pcg.size();
    out->assemble_launches = (int)s->ev_asm.size();
    out->solves            = s->timed_solves;
    if (s->iters_total) HIP_TRY(hipMemcpy(&out->pcg_iters, s->iters_total, sizeof(long long), hipMemcpyDeviceToHost));
    if (s->has_problem && s->v.D > 0) {
        std::vector<int32_t> cnt((size_t)s->v.D);
        HIP_TRY(hipMemcpy(cnt.data(), s->v.ell_cnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost));
        long long nnz = 0;
        for (int32_t c : cnt) nnz += c;
        out->matrix_nnz = nnz;
    }
    return DFA_OK;
}

// -------------------------------------------------------------------- north-star solver seam

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

int dfa_solver6_create(int max_D, int max_N, int k, dfa_solver6** out) {
    REQUIRE(out, "null out");
    *out = nullptr;
    REQUIRE(max_D > 0 && max_N >= 0, "bad sizes");
    REQUIRE(k >= 1 && k <= 8, "k out of range 1..8");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DFA_ERR_NO_GPU, "no HIP device");
    dfa_solver6* s = new (std::nothrow) dfa_solver6();
    REQUIRE(s, "out of host memory");
    s->max_D = max_D, s->max_N = max_N, s->k = k, s->has_problem = false, s->node_dq = nullptr;
    std::memset(&s->v, 0, sizeof(s->v));
    s->v.cap = DFA_SOLVE6_ROW_BLOCKS;  // = S6_MAXSLOT of solve6_internal.hpp
    const size_t N = (size_t)max_N, D = (size_t)max_D, cap = (size_t)s->v.cap;
    dfa::PlanArena& mem = s->mem;
#define A(field, count) mem.alloc(&s->v.field, (count))
    A(idx, N * k);
    A(wn, N * k);
    A(idx_nat, N * k);
    A(near, N);
    A(vptr, D + 1);
    A(vlist, N);
    A(vperm, N);
    A(canon_own, N * 3);
    A(canon_n_own, N * 3);
    A(reg_idx, D * k);
    A(blk_hist, D * (dfa::SOLVE_TG_BLOCKS + 1));
    A(node_ptr, D + 1);
    A(node_list, N * k + 1);  // (+ 1: the assembly reads one entry even of an empty list)
    A(rnode_ptr, D + 1);
    A(rnode_list, D * k + 1);  // (+ 1: the assembly reads one entry even of an empty list)
    A(dq, D * 8);
    A(dq_prev, D * 8);
    A(ghat, D * 3);
    A(rec, N * (12 + (k <= 4 ? 4 : 8)));
    A(cost_part, (N + 255) / 256 + (D * k + 255) / 256 + 1);
    A(valid_part, (N + 255) / 256 + (D * k + 255) / 256 + 1);
    A(mnode, D * 48);
    A(rho, N);
    A(rres, D * k * 3);
    A(rvec, D * k * 18);
    A(rhub, D * k);
    A(bcols, D * cap);
    A(bcnt, D);
    A(bfu, D);
    A(rslot, D * cap);
    A(utab, D * 256);
    A(eslot, N * k * k);
    A(pair_list, N * k * k);
    A(pair_ptr, D * (cap + 1));
    A(bvals, D * cap * 36);
    A(minv, D * 36);
    A(g, D * 6);
    A(x, D * 6);
    A(r, D * 6);
    A(p, D * 6);
    A(s, D * 6);
    A(w, D * 6);
    A(u[0], D * 6);
    A(u[1], D * 6);
    A(t[0], D * 6);
    A(t[1], D * 6);
    A(m[0], D * 6);
    A(m[1], D * 6);
    A(g_part[0], (size_t)dfa::s6_matvec_blocks(max_D));
    A(g_part[1], (size_t)dfa::s6_matvec_blocks(max_D));
    A(d_part[0], (size_t)dfa::s6_matvec_blocks(max_D));
    A(d_part[1], (size_t)dfa::s6_matvec_blocks(max_D));
#undef A
    mem.alloc(&s->raw_w, N * k);
    mem.alloc(&s->raw_reg, D * (k + 1));
    mem.alloc(&s->state, 1);
    int rc = plan_status(mem);
    if (rc == DFA_OK) {  // the launch budget's mirror and completion events (none: every PCG gets its full budget)
        bool ok = true;
        for (int i = 0; ok && i < dfa::S6_RING; ++i)
            ok = hipEventCreateWithFlags(&s->done_ev[i], hipEventDisableTiming) == hipSuccess;
        if (ok) s->mirror = mem.pinned<int>(dfa::S6_RING * dfa::S6_HIST);
        else (void)hipGetLastError();
        rc = plan_grid(s->grid, max_D);
    }
    if (rc != DFA_OK) {
        dfa_solver6_destroy(s);
        return rc;
    }
    *out = s;
    return DFA_OK;
}

void dfa_solver6_destroy(dfa_solver6* s) {
    if (!s) return;
    for (auto& g : s->pcg_graphs) (void)hipGraphExecDestroy(g.second);
    for (hipEvent_t e : s->done_ev)
        if (e) (void)hipEventDestroy(e);
    if (s->capture_stream) (void)hipStreamDestroy(s->capture_stream);
    s->grid.release();
    delete s;  // (the arena frees the plan's memory, the pool its events)
}

int dfa_solver6_set_problem(dfa_solver6* s, const float* node_pos, const float* node_dq, const float* node_w, int D,
                            const float* canon_vertices, const float* canon_normals, int N, dfa_stream_t stream) {
    REQUIRE(s, "null plan");
    REQUIRE(node_pos && node_dq && node_w && D > 0, "no nodes");
    REQUIRE(N >= 0 && (N == 0 || canon_vertices), "bad vertex arrays");
    if (D > s->max_D || N > s->max_N) return fail(DFA_ERR_CAPACITY, "problem larger than the plan");
    dfa::Solve6View& v = s->v;
    v.N = N, v.D = D, v.k = s->k;
    // (the solver reads its own, sorted copies of the vertices: s6_build_graph)
    v.node_pos = node_pos, v.node_w = node_w, v.canon = v.canon_own, v.canon_n = canon_normals ? v.canon_n_own : nullptr;
    s->node_dq = node_dq;
    const dfa::KnnGridView* grid = nullptr;
    if (want_grid(D, N)) {
        HIP_TRY(dfa::knn_grid_build(s->grid.v, node_pos, D, S(stream)));
        grid = &s->grid.v;
    }
    HIP_TRY(dfa::launch_knn(node_pos, node_w, D, canon_vertices, N, s->k, v.idx_nat, s->raw_w, grid, S(stream)));
    const int kreg = s->k + 1;
    HIP_TRY(dfa::launch_knn(node_pos, node_w, D, node_pos, D, kreg, s->raw_reg, nullptr, grid, S(stream)));
    HIP_TRY(dfa::s6_build_graph(v, s->state, canon_vertices, canon_normals, s->raw_w, s->raw_reg, kreg, S(stream)));
    s->has_problem = true;
    return DFA_OK;
}

int dfa_solver6_set_node_transforms(dfa_solver6* s, const float* node_dq) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(node_dq, "null transforms");
    s->node_dq = node_dq;
    return DFA_OK;
}

int dfa_solver6_solve(dfa_solver6* s, const float* live_vertex_map, int vertex_step, const float* live_normal_map,
                      int normal_step, int cols, int rows, float fx, float fy, float cx, float cy,
                      const dfa_solve6_params* prm, dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(prm, "null params");
    REQUIRE(live_vertex_map && live_normal_map && cols > 0 && rows > 0, "bad live maps");
    REQUIRE(vertex_step >= cols * 16 && normal_step >= cols * 16, "row step smaller than a row");
    REQUIRE(prm->num_iter >= 0 && prm->gn_iter >= 0 && prm->linear_iter >= 0, "negative iteration count");
    REQUIRE(prm->tukey_offset > 0.f && prm->psi_data > 0.f && prm->psi_reg > 0.f, "non-positive robust parameter");
    REQUIRE(prm->damping >= 0.f && prm->lambda >= 0.f, "negative damping / lambda");
    REQUIRE(prm->pcg_tol_first <= 0.f || prm->pcg_tol_adapt > 0.f || (prm->pcg_tol_decay > 0.f && prm->pcg_tol_decay <= 1.f),
            "forcing decay outside (0, 1]");
    REQUIRE(prm->pcg_tol_adapt >= 0.f, "negative adaptive forcing factor");
    REQUIRE(prm->gn_tol >= 0.f && prm->gn_tol < 1.f, "gn_tol outside [0, 1)");
    dfa::Solve6Params p{prm->num_iter, prm->gn_iter, prm->linear_iter, prm->tukey_offset, prm->psi_data, prm->lambda,
                        prm->psi_reg, prm->dist_thresh, prm->cos_thresh, prm->damping, prm->pcg_tol, prm->pcg_tol_first,
                        prm->pcg_tol_decay, prm->pcg_tol_adapt, prm->gn_tol};
    const bool early = p.gn_tol > 0.f;
    dfa::Solve6Image img{live_vertex_map, live_normal_map, vertex_step, normal_step, cols, rows, fx, fy, cx, cy};
    hipStream_t st = S(stream);
    s->ev.rewind();
    HIP_TRY(dfa::s6_begin(s->v, s->state, s->node_dq, early ? p.num_iter * p.gn_iter : 0, st));
    s->last_launches = 0;
    // ---- launch budget (launch_budget.hpp): the solves up to n - 2 enter the history, in order, each behind its completion event
    dfa::LaunchBudget& budget = s->budget;
    const auto b = budget.start(prm->adaptive_launch && s->mirror,
                                dfa::BudgetKey{s->v.D, s->v.N, p.num_iter, p.gn_iter, p.linear_iter, p.pcg_tol, p.pcg_tol_first,
                                               p.pcg_tol_decay, p.pcg_tol_adapt, p.gn_tol});
    for (unsigned long long f = b.fold_from; f < b.fold_to; ++f) {
        const int fs = (int)(f % dfa::S6_RING);
        HIP_TRY(hipEventSynchronize(s->done_ev[fs]));  // two solves back: complete long ago unless the caller is far ahead
        budget.fold(s->mirror + fs * dfa::S6_HIST);
    }
    if (b.reset) budget.forget(b.n);
    int* mirror_slot = s->mirror ? s->mirror + b.slot * dfa::S6_HIST : nullptr;
    if (mirror_slot) {
        // the slot's previous owner, solve n - S6_RING, must have finished writing it (it has, unless the caller runs more
        // than S6_RING - 1 solves ahead of the device)
        if (b.slot_reused) HIP_TRY(hipEventSynchronize(s->done_ev[b.slot]));
        std::memset(mirror_slot, 0, dfa::S6_HIST * sizeof(int));
        budget.slot_gn[b.slot] = p.num_iter * p.gn_iter;
    }
    // the graphs replay launches over the plan's own buffers: only the node count is part of what they captured
    if (s->pcg_key_D != s->v.D) {
        for (auto& g : s->pcg_graphs) (void)hipGraphExecDestroy(g.second);
        s->pcg_graphs.clear();
        s->pcg_key_D = s->v.D;
    }
    for (int outer = 0; outer < p.num_iter; ++outer)
        for (int gn = 0; gn < p.gn_iter; ++gn) {
            auto mark = [&]() { if (s->timing) (void)s->ev.record(st); };  // 4 per Gauss-Newton iteration: | linearise | assemble | pcg |
            const int gi = outer * p.gn_iter + gn;
            mark();
            // gn_tol > 0: the launch's last workgroup applies the stopping rule on the device — launches behind the end of an
            // outer iteration return at entry (nothing comes back to the host: the launches of the whole solve are enqueued
            // regardless)
            HIP_TRY(dfa::s6_linearise(s->v, s->state, img, p, gn == 0, gi, gn, 0, st));
            mark();
            HIP_TRY(dfa::s6_assemble(s->v, s->state, p, gn, st));
            mark();
            int launches = budget.launches(gi, p.linear_iter);  // the caller's cap, or what this iteration has needed
            // the PCG launches of one Gauss-Newton iteration are replayed as a HIP graph (one per launch count); if capture
            // is not possible here (it never is on some stream configurations) the launches are issued one by one
            bool replayed = false;
            if (!s->graph_disabled) {
                auto it = s->pcg_graphs.find(launches);
                if (it == s->pcg_graphs.end()) {
                    hipGraph_t g = nullptr;
                    hipGraphExec_t ge = nullptr;
                    bool ok = s->capture_stream || hipStreamCreateWithFlags(&s->capture_stream, hipStreamNonBlocking) == hipSuccess;
                    ok = ok && hipStreamBeginCapture(s->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
                    if (ok) {
                        const hipError_t le = dfa::s6_pcg_n(s->v, s->state, launches, s->capture_stream);
                        const hipError_t ce = hipStreamEndCapture(s->capture_stream, &g);
                        ok = le == hipSuccess && ce == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
                        if (g) (void)hipGraphDestroy(g);
                    }
                    if (ok) {
                        it = s->pcg_graphs.emplace(launches, ge).first;
                    } else {
                        (void)hipGetLastError();  // clear the sticky error of the failed attempt
                        s->graph_disabled = true;
                    }
                }
                if (it != s->pcg_graphs.end()) {
                    HIP_TRY(hipGraphLaunch(it->second, st));
                    replayed = true;
                }
            }
            if (!replayed) HIP_TRY(dfa::s6_pcg_n(s->v, s->state, launches, st));
            s->last_launches += launches + 1;
            mark();
            HIP_TRY(dfa::s6_update(s->v, s->state, launches, p.linear_iter, gi < dfa::S6_HIST ? mirror_slot : nullptr, gi, 1, st));
        }
    if (early && p.num_iter * p.gn_iter > 0) {
        // the last step of the solve, if its outer iteration ran to the cap: one closing linearisation decides whether it stays
        const int gi = p.num_iter * p.gn_iter;
        HIP_TRY(dfa::s6_linearise(s->v, s->state, img, p, 0, gi, p.gn_iter, 1, st));
        HIP_TRY(dfa::s6_update(s->v, s->state, 0, p.linear_iter, nullptr, gi, 0, st));
    }
    if (mirror_slot) HIP_TRY(hipEventRecord(s->done_ev[b.slot], st));
    return DFA_OK;
}

int dfa_solver6_enable_timing(dfa_solver6* s, int enable) {
    REQUIRE(s, "null plan");
    s->timing = enable != 0;
    return DFA_OK;
}

int dfa_solver6_get_timing(dfa_solver6* s, dfa_solve6_timing* out, dfa_stream_t stream) {
    REQUIRE(s && out, "null plan / out");
    HIP_TRY(hipStreamSynchronize(S(stream)));
    std::memset(out, 0, sizeof(*out));
    const std::vector<hipEvent_t>& ev = s->ev.events;
    for (size_t i = 0; i + 3 < s->ev.used; i += 4) {
        float a = 0.f, b = 0.f, c = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, ev[i], ev[i + 1]));
        HIP_TRY(hipEventElapsedTime(&b, ev[i + 1], ev[i + 2]));
        HIP_TRY(hipEventElapsedTime(&c, ev[i + 2], ev[i + 3]));
        out->linearise_ms += a, out->assemble_ms += b, out->pcg_ms += c;
        out->gn_iterations += 1;
    }
    if (s->has_problem && s->v.D > 0) {
        std::vector<int32_t> cnt((size_t)s->v.D);
        HIP_TRY(hipMemcpy(cnt.data(), s->v.bcnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost));
        for (int32_t c : cnt) out->matrix_blocks += c;
    }
    return DFA_OK;
}

const float* dfa_solver6_node_dq(const dfa_solver6* s) { return s ? s->v.dq : nullptr; }
static_assert(DFA_SOLVE6_ROW_BLOCKS == dfa::S6_ROW_BLOCKS, "row capacity of the C ABI and of the plan (S6_MAXSLOT of solve6_internal.hpp)");
const float* dfa_solver6_matrix_blocks(const dfa_solver6* s) { return s ? s->v.bvals : nullptr; }
const int32_t* dfa_solver6_matrix_columns(const dfa_solver6* s) { return s ? s->v.bcols : nullptr; }
const int32_t* dfa_solver6_matrix_row_blocks(const dfa_solver6* s) { return s ? s->v.bcnt : nullptr; }
const float* dfa_solver6_gradient(const dfa_solver6* s) { return s ? s->v.g : nullptr; }
const float* dfa_solver6_step(const dfa_solver6* s) { return s ? s->v.x : nullptr; }
const int32_t* dfa_solver6_data_graph(const dfa_solver6* s) { return s ? s->v.idx_nat : nullptr; }
const int32_t* dfa_solver6_reg_graph(const dfa_solver6* s) { return s ? s->v.reg_idx : nullptr; }

int dfa_solver6_warp(dfa_solver6* s, float* out_vertices, float* out_normals, dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(out_vertices, "null output");
    HIP_TRY(dfa::s6_warp(s->v, s->v.dq, out_vertices, out_normals, S(stream)));
    return DFA_OK;
}

int dfa_solver6_warp_with(dfa_solver6* s, const float* node_dq, float* out_vertices, float* out_normals, dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(node_dq && out_vertices, "null transforms / output");
    HIP_TRY(dfa::s6_warp(s->v, node_dq, out_vertices, out_normals, S(stream)));
    return DFA_OK;
}

int dfa_solver6_get_stats(dfa_solver6* s, dfa_solve6_stats* out, dfa_stream_t stream) {
    REQUIRE(s && out, "null argument");
    dfa::Solve6State h;
    HIP_TRY(hipMemcpyAsync(&h, s->state, sizeof(h), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    out->initial_cost = h.initial_cost, out->final_cost = h.final_cost;
    out->gn_iters = h.gn_iters, out->pcg_iters = h.pcg_iters;
    out->gn_solves = h.gn_solves, out->gn_rejected = h.gn_rejected, out->gn_converged = h.gn_converged, out->hist_n = h.hist_n;
    out->valid_first = (long long)h.valid_first, out->valid_last = (long long)h.valid_last;
    out->max_row_blocks = h.max_row_blocks, out->overflow = h.overflow;
    out->pcg_short = h.pcg_short, out->pcg_launches = s->last_launches;
    static_assert(DFA_SOLVE6_HIST == dfa::S6_HIST, "history length of the C ABI and of the state block");
    for (int i = 0; i < DFA_SOLVE6_HIST; ++i) {
        const bool in = i < h.hist_n;
        out->valid_hist[i] = in ? (long long)h.valid_hist[i] : 0ll;
        out->stop_hist[i] = in ? h.stop_hist[i] : 0;
        out->cost_hist[i] = in ? h.cost_hist[i] : 0.0;
        out->pcg_rel_hist[i] = in ? h.pcg_rel_hist[i] : 0.f;
        out->pcg_tol_hist[i] = in ? h.pcg_tol_hist[i] : 0.f;
        out->pcg_it_hist[i] = in ? h.pcg_it_hist[i] : 0;
    }
    return h.overflow ? fail(DFA_ERR_CAPACITY, "a block row of the normal matrix exceeded the plan's capacity") : DFA_OK;
}

}  // extern "C"

#ifdef DFA_DEV_AB  // development flavour only: the plan's graph-build outputs, for the tests that compare the two launch sequences
// out[0..10] = ridx, rw, rb, re, reg_idx, node_ptr, node_list, t, state block, tickets, (size_t) bytes of the state block;
// returns 1 if the last set_problem took the fused graph build
extern "C" __attribute__((visibility("default"))) int dfa_dev_solver_graph_ptrs(dfa_solver* s, void** out) {
    const dfa::SolveView& v = s->v;
    void* p[] = {v.ridx, v.rw, v.rb, v.re, v.reg_idx, v.node_ptr, v.node_list, v.t, s->state, s->ticket, (void*)sizeof(dfa::SolveState)};
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i) out[i] = p[i];
    return s->graph_rows ? 1 : 0;
}
#endif

#ifdef DFA_S6_DEBUG  // development builds only: device pointers of the north-star plan (tools/ns_plan_check.py)
extern "C" __attribute__((visibility("default"))) int dfa_dev_solver6_ptrs(dfa_solver6* s, void** out) {
    const dfa::Solve6View& v = s->v;
    void* p[] = {v.utab, v.pair_ptr, v.pair_list, v.bcnt, v.bfu, (void*)v.node_ptr, (void*)v.node_list, v.bcols, v.bvals, v.g,
                 (void*)v.idx, v.rec, nullptr, v.mnode, v.rslot};
    out[18] = v.minv;
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i) out[i] = p[i];
    out[15] = (void*)(size_t)v.cap, out[16] = (void*)(size_t)v.D, out[17] = (void*)(size_t)v.N;
    return 0;
}
#endif
