// solve_graph.hip — the per-problem set-up of the reference-mode solve (formulation and MI355X mapping: solve.hpp): the
// residual rows (graph_rows_kernel: both k-NN searches and the rows in one launch; prepare_rows_kernel behind searches
// launched on their own), the reset of the unknowns / state block / tickets, and the node -> rows transposition the
// assembly gathers through.  Row graph and record head: solve_rows.hpp.
//
// Launches of one problem (dfa_solver_set_problem), nodes in the grid, k in {4, 8, 16}:
//   grid_build_one_kernel (knn_grid.hip) -> graph_rows_kernel<K> (both k-NN searches, rows, reset) -> tg_count_kernel ->
//   tg_colscan_kernel -> tg_fill_kernel [-> sort_node_lists_kernel, order-stable variant]
// otherwise (no grid, another k, no vertices; DFA_GRAPH_ROWS=0 in development builds):
//   [grid build ->] knn_kernel / knn_wave_kernel (vertices) -> knn_wave_kernel / knn_kernel (nodes) ->
//   prepare_rows_kernel<K> -> tg_count_kernel -> tg_colscan_kernel -> tg_fill_kernel [-> sort_node_lists_kernel]
// Both leave the same bits (tests/test_gpu_graph_rows.py).
#include <hip/hip_runtime.h>

#include "dev_switch.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"
#include "solve.hpp"
#include "solve_internal.hpp"
#include "solve_rows.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------
// transpose graph node -> (row, slot).  A counting sort of the R*k slot entries by node id with
// workgroup-private histograms in LDS: TG_BLOCKS workgroups each own a contiguous chunk of the
// entries, count into LDS (no global atomics: 1 M device-scope atomics on 2 k counters were
// the whole cost of the first version), publish their histogram, a thread per node turns the
// [block][node] table into per-block bases + node totals, and the fill pass (which scans the totals
// itself) replays the chunk with an LDS cursor per node.  Deterministic up to the order inside one chunk.

constexpr int TG_BLOCKS = SOLVE_TG_BLOCKS;

__global__ __launch_bounds__(1024) void tg_count_kernel(const int32_t* __restrict__ ridx, size_t total, int D,
                                                        int32_t* __restrict__ blk_hist /* [TG_BLOCKS][D] */) {
    extern __shared__ int32_t hist[];
    for (int i = threadIdx.x; i < D; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const size_t chunk = (total + TG_BLOCKS - 1) / TG_BLOCKS;
    const size_t beg = chunk * blockIdx.x, end = min(beg + chunk, total);
    for (size_t e = beg + threadIdx.x; e < end; e += blockDim.x) {
        const int n = ridx[e];
        if (n >= 0) atomicAdd(&hist[n], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += blockDim.x) blk_hist[(size_t)blockIdx.x * D + i] = hist[i];
}

// per node (one thread each): exclusive prefix over the TG_BLOCKS workgroup counts -> per-block bases RELATIVE to the
// node's segment, and the node's total in row TG_BLOCKS of the table.  (Round 1 did this and the scan of the totals in
// one 1024-thread workgroup: two passes of 64 dependent loads per thread, 19 us at C2; now 64 independent loads.)
__global__ __launch_bounds__(256) void tg_colscan_kernel(int32_t* __restrict__ blk_hist /* [TG_BLOCKS + 1][D] */, int D) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    constexpr int G = 32;  // counts in flight per thread (all TG_BLOCKS at once would be 256 registers)
    static_assert(TG_BLOCKS % G == 0, "workgroups of the counting sort in groups");
    int run = 0;
    for (int b0 = 0; b0 < TG_BLOCKS; b0 += G) {
        int h[G];
#pragma unroll
        for (int b = 0; b < G; ++b) h[b] = blk_hist[(size_t)(b0 + b) * D + i];
#pragma unroll
        for (int b = 0; b < G; ++b) {
            blk_hist[(size_t)(b0 + b) * D + i] = run;
            run += h[b];
        }
    }
    blk_hist[(size_t)TG_BLOCKS * D + i] = run;
}

// Every fill workgroup scans the D node totals itself (LDS, a few microseconds) instead of waiting for a scan launch;
// workgroup 0 publishes node_ptr.
__global__ __launch_bounds__(1024) void tg_fill_kernel(const int32_t* __restrict__ ridx, size_t total, int D,
                                                       const int32_t* __restrict__ blk_base /* [TG_BLOCKS + 1][D] */,
                                                       int32_t* __restrict__ node_ptr, uint32_t* __restrict__ node_list) {
    extern __shared__ int32_t cursor[];
    __shared__ int32_t wave_tot[16];
    __shared__ int32_t carry_sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_sh = 0;
    __syncthreads();
    for (int base = 0; base < D; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < D ? blk_base[(size_t)TG_BLOCKS * D + i] : 0;
        const int incl = wave_inclusive_scan(v);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int off = carry_sh + incl - v;
        for (int w = 0; w < wave; ++w) off += wave_tot[w];
        if (i < D) {
            cursor[i] = off + blk_base[(size_t)blockIdx.x * D + i];
            if (blockIdx.x == 0) node_ptr[i] = off;
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_sh = off + v;
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) node_ptr[D] = carry_sh;
    const size_t chunk = (total + TG_BLOCKS - 1) / TG_BLOCKS;
    const size_t beg = chunk * blockIdx.x, end = min(beg + chunk, total);
    for (size_t e = beg + threadIdx.x; e < end; e += blockDim.x) {
        const int n = ridx[e];
        if (n >= 0) node_list[atomicAdd(&cursor[n], 1)] = (uint32_t)e;
    }
}

// start of a solve: unknowns, state block and arrival tickets zeroed by ONE launch
__global__ __launch_bounds__(256) void reset_kernel(float* __restrict__ t, int n3, SolveState* __restrict__ st,
                                                    unsigned int* __restrict__ ticket, int nticket) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) t[i] = 0.f;
    if (blockIdx.x == 0) {
        unsigned int* w = (unsigned int*)st;
        for (int j = threadIdx.x; j < (int)(sizeof(SolveState) / 4); j += blockDim.x) w[j] = 0u;
        for (int j = threadIdx.x; j < nticket; j += blockDim.x) ticket[j] = 0u;
    }
}

// slots of the regularisation row of node n and its neighbour m: {m: -1, n: +1}; all empty for an absent neighbour and for
// the self edge (opt_solver.cpp:74-105, energy.t:75-78)
template <int K>
__device__ __forceinline__ void reg_row_slots(int m, int n, int (&ids)[K], float (&ws)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) ids[j] = -1, ws[j] = 0.f;
    if (m >= 0 && m != n) ids[0] = m, ws[0] = -1.f, ids[1] = n, ws[1] = +1.f;  // k >= 2 whenever a non-self neighbour exists
}

// row r's K node ids and weights by 16-byte stores (k == K, K a multiple of 4)
template <int K>
__device__ __forceinline__ void store_row_graph(const SolveView& s, size_t r, const int (&ids)[K], const float (&ws)[K]) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        reinterpret_cast<int4*>(s.ridx + r * K)[q]  = make_int4(ids[4 * q], ids[4 * q + 1], ids[4 * q + 2], ids[4 * q + 3]);
        reinterpret_cast<float4*>(s.rw + r * K)[q] = make_float4(ws[4 * q], ws[4 * q + 1], ws[4 * q + 2], ws[4 * q + 3]);
    }
}

// The per-problem row set-up as ONE launch, a thread per row: regularisation rows (opt_solver.cpp:74-105), right-hand
// sides of the data rows (energy.t:55), packed record heads and the zeroing of the
// unknowns / state block / tickets (reset_kernel) — four launches of 5-16 us each at C2 in round 1.
template <int K>
__global__ __launch_bounds__(256) void prepare_rows_kernel(SolveView s, SolveState* __restrict__ st,
                                                           unsigned int* __restrict__ ticket, int nticket) {
    const size_t R = (size_t)s.N + (size_t)s.D * s.k;
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < (size_t)3 * s.D) s.t[r] = 0.f;
    if (blockIdx.x == 0) {
        unsigned int* w = (unsigned int*)st;
        for (int j = threadIdx.x; j < (int)(sizeof(SolveState) / 4); j += blockDim.x) w[j] = 0u;
        for (int j = threadIdx.x; j < nticket; j += blockDim.x) ticket[j] = 0u;
    }
    if (r >= R) return;
    const int k = s.k;
    int ids[K];
    float ws[K];
    const bool wide = k == K && K % 4 == 0;  // (uniform) the common case: every row's ids / weights / record head by 16-byte accesses
    if (r < (size_t)s.N) {  // data row: k-NN + RBF weights already in ridx / rw; b = live - canonical (energy.t:55)
#pragma unroll
        for (int c = 0; c < 3; ++c) s.rb[3 * r + c] = s.live[3 * r + c] - s.canon[3 * r + c];
        if (wide) load_row_graph<K>(s, r, ids, ws);
        else {
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < k) ids[j] = s.ridx[r * k + j], ws[j] = s.rw[r * k + j];
        }
    } else {  // regularisation row N + n k + i <- {reg_idx[n][i]: -1, n: +1} (opt_solver.cpp:74-105, energy.t:75-78)
        const int e = (int)(r - (size_t)s.N), n = e / k, m = s.reg_idx[e];
        reg_row_slots<K>(m, n, ids, ws);
        if (wide) store_row_graph<K>(s, r, ids, ws);
        else {
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (j < k) s.ridx[r * k + j] = ids[j], s.rw[r * k + j] = ws[j];
        }
        s.rb[3 * r + 0] = s.rb[3 * r + 1] = s.rb[3 * r + 2] = 0.f;
    }
    store_record_head<K>(s, r, ids, ws, wide);
}

// Both graphs and the row set-up as ONE launch (plans whose nodes are in the grid, k == K, K a multiple of 4): what
// knn_kernel<K, true> (vertex -> nodes), knn_wave_kernel<K> (node -> nodes) and prepare_rows_kernel<K> do one after the
// other, with the rows written by the searches that find them — prepare_rows_kernel re-read ridx / rw / reg_idx / canon
// a few microseconds after they were written, only to pack them again.  The two searches do not depend on each other: the
// node search's waves (one per node) run beside the vertex search, a chain of dependent loads at 4 waves per SIMD.
//   workgroups [0, ceil(N / 256))       data role: a lane per canonical vertex — knn_grid_query, RBF weights, ridx / rw,
//                                       rb = live - canonical (the query itself), the record head
//   the next ceil(D / 4) workgroups     regularisation role: a wave per node — knn_wave_search, reg_idx, and lanes j < k
//                                       write row N + n k + j; their first 3 D threads zero the unknowns, the first
//                                       workgroup the state block and the tickets (reset_kernel)
// Same searches, same expressions, same operands: every output holds the bits the three launches leave.
// ONE_LOOP: the data role's lanes walk the nine rows around their cell in one loop each (knn_walk.hpp; the ranges wait in
// LDS, 18 KiB per workgroup); false — development builds, DFA_KNN_ONE_LOOP=0 — keeps the nine wave-wide loops.
template <int K, bool ONE_LOOP>
__global__ __launch_bounds__(256) void graph_rows_kernel(SolveView s, KnnGridView grid, SolveState* __restrict__ st,
                                                         unsigned int* __restrict__ ticket, int nticket, int data_blocks) {
    static_assert(K % 4 == 0, "rows by 16-byte stores");
    static_assert(KNN_WALK_STRIDE == 256, "one column of slots per thread");
    __shared__ KnnWalkSlots<ONE_LOOP> slots;
    if ((int)blockIdx.x < data_blocks) {
        const int v = blockIdx.x * blockDim.x + threadIdx.x;
        if (v >= s.N) return;
        const f3 q = mk3(s.canon[3 * (size_t)v], s.canon[3 * (size_t)v + 1], s.canon[3 * (size_t)v + 2]);
        KnnList<K> best;
        knn_grid_query<K, false, ONE_LOOP>(*grid.desc, grid.cell_start, grid.sorted, q, best, false, s.D, slots.of_lane());
        int ids[K];
        float ws[K];
        knn_ids_weights<K>(best, K, s.node_pos, s.node_w, true, q, ids, ws);
        const size_t r = (size_t)v;
        store_row_graph<K>(s, r, ids, ws);
        s.rb[3 * r + 0] = s.live[3 * r + 0] - q.x, s.rb[3 * r + 1] = s.live[3 * r + 1] - q.y, s.rb[3 * r + 2] = s.live[3 * r + 2] - q.z;
        store_record_head<K>(s, r, ids, ws, true);
        return;
    }
    const int b = (int)blockIdx.x - data_blocks;
    const int i = b * (int)blockDim.x + (int)threadIdx.x;
    if (i < 3 * s.D) s.t[i] = 0.f;
    if (b == 0) {
        unsigned int* w = (unsigned int*)st;
        for (int j = threadIdx.x; j < (int)(sizeof(SolveState) / 4); j += blockDim.x) w[j] = 0u;
        for (int j = threadIdx.x; j < nticket; j += blockDim.x) ticket[j] = 0u;
    }
    const int n = b * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= s.D) return;
    const f3 q = mk3(s.node_pos[3 * (size_t)n], s.node_pos[3 * (size_t)n + 1], s.node_pos[3 * (size_t)n + 2]);
    int near[K];
    knn_wave_search<K>(*grid.desc, grid.cell_start, grid.sorted, q, lane, near);
    if (lane >= K) return;
    int m = -1;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j == lane) m = near[j];
    const size_t e = (size_t)n * K + lane, r = (size_t)s.N + e;
    s.reg_idx[e] = m;
    int ids[K];
    float ws[K];
    reg_row_slots<K>(m, n, ids, ws);
    store_row_graph<K>(s, r, ids, ws);
    s.rb[3 * r + 0] = s.rb[3 * r + 1] = s.rb[3 * r + 2] = 0.f;
    store_record_head<K>(s, r, ids, ws, true);
}

// Order-stable variant (SolveView::deterministic; what else it changes: solve_assemble.hip): a node's row list sorted, since
// the transposition fills it in the order its LDS cursor atomics land and that order feeds float sums of the assembly.
constexpr int DET_SORT_MAX = 4096;

__global__ __launch_bounds__(256) void sort_node_lists_kernel(const int32_t* __restrict__ node_ptr, uint32_t* __restrict__ node_list) {
    __shared__ uint32_t buf[DET_SORT_MAX];
    const int a = blockIdx.x, tid = threadIdx.x;
    const int beg = node_ptr[a], len = node_ptr[a + 1] - beg;
    if (len < 2 || len > DET_SORT_MAX) return;  // (longer lists keep the order of the transposition)
    int n2 = 1;
    while (n2 < len) n2 <<= 1;
    for (int i = tid; i < n2; i += 256) buf[i] = i < len ? node_list[beg + i] : 0xffffffffu;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2 / 2; i += 256) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t x = buf[lo], y = buf[hi];
                if ((x > y) == up) buf[lo] = y, buf[hi] = x;
            }
            __syncthreads();
        }
    for (int i = tid; i < len; i += 256) node_list[beg + i] = buf[i];
}

// ------------------------------------------------------------------------------------------
// launchers

// node -> (row, slot) lists of any R x k index array (shared with solve6_graph.hip)
hipError_t solve_transpose_graph(const int32_t* ridx, size_t total, int D, int32_t* blk_hist, int32_t* node_ptr,
                                 uint32_t* node_list, hipStream_t st) {
    const size_t lds = sizeof(int32_t) * (size_t)D;
    tg_count_kernel<<<TG_BLOCKS, 1024, lds, st>>>(ridx, total, D, blk_hist);
    tg_colscan_kernel<<<(D + 255) / 256, 256, 0, st>>>(blk_hist, D);
    tg_fill_kernel<<<TG_BLOCKS, 1024, lds, st>>>(ridx, total, D, blk_hist, node_ptr, node_list);
    return hipGetLastError();
}

// the node -> rows transposition of the rows in place, sorted lists in the order-stable variant
static hipError_t transpose_rows(const SolveView& s, hipStream_t st) {
    const size_t total = ((size_t)s.N + (size_t)s.D * s.k) * s.k;
    const hipError_t e = solve_transpose_graph(s.ridx, total, s.D, s.blk_hist, s.node_ptr, s.node_list, st);
    if (e != hipSuccess) return e;
    if (s.deterministic) sort_node_lists_kernel<<<s.D, 256, 0, st>>>(s.node_ptr, s.node_list);
    return hipGetLastError();
}

hipError_t solve_build_graph(const SolveView& s, SolveState* state, unsigned int* ticket, int nticket, hipStream_t st) {
    const int D = s.D, N = s.N, k = s.k;
    const size_t R = (size_t)N + (size_t)D * k;
    const size_t threads = R > (size_t)3 * D ? R : (size_t)3 * D;
    KDISPATCH(prepare_rows_kernel, k, <<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(s, state, ticket, nticket));
    return transpose_rows(s, st);
}

bool solve_graph_rows_fits(const SolveView& s) {
    const int k = s.k;
    // (the template's K is k itself, and the rows go out as 16-byte stores; DFA_GRAPH_ROWS=0 — development builds — keeps
    // the searches and prepare_rows_kernel as launches of their own, for the comparison)
    return s.N > 0 && (k == 4 || k == 8 || k == 16) &&
           ((reinterpret_cast<uintptr_t>(s.ridx) | reinterpret_cast<uintptr_t>(s.rw) | reinterpret_cast<uintptr_t>(s.re)) & 15u) == 0 &&
           dev_env_int("DFA_GRAPH_ROWS", 1) != 0;
}

hipError_t solve_build_graph_rows(const SolveView& s, const KnnGridView& grid, SolveState* state, unsigned int* ticket,
                                  int nticket, hipStream_t st) {
    const int data_blocks = (s.N + 255) / 256, reg_blocks = (s.D + 3) / 4;
#define GRAPH_ROWS_LAUNCH(K, ONE_LOOP) \
    graph_rows_kernel<K, ONE_LOOP><<<data_blocks + reg_blocks, 256, 0, st>>>(s, grid, state, ticket, nticket, data_blocks)
#ifdef DFA_DEV_AB
    if (!knn_one_loop()) {
        if (s.k <= 4) GRAPH_ROWS_LAUNCH(4, false);
        else if (s.k <= 8) GRAPH_ROWS_LAUNCH(8, false);
        else GRAPH_ROWS_LAUNCH(16, false);
        return transpose_rows(s, st);
    }
#endif
    if (s.k <= 4) GRAPH_ROWS_LAUNCH(4, true);
    else if (s.k <= 8) GRAPH_ROWS_LAUNCH(8, true);
    else GRAPH_ROWS_LAUNCH(16, true);
#undef GRAPH_ROWS_LAUNCH
    return transpose_rows(s, st);
}

hipError_t solve_reset(const SolveView& s, SolveState* state, unsigned int* ticket, int nticket, hipStream_t st) {
    reset_kernel<<<(3 * s.D + 255) / 256, 256, 0, st>>>(s.t, 3 * s.D, state, ticket, nticket);
    return hipGetLastError();
}

}  // namespace dfa
