// solve6_graph.hip — once per frame of the north-star solve (formulation and launch list: solve6.hpp): the solver's
// vertex order (by nearest node, by index inside a node), the normalised weights, the regularisation graph and the three
// node -> rows transpositions; s6_build_graph ends in the pattern's two launches (solve6_pattern.hip).  Also here, because
// it goes through that vertex order: s6_gather_mask, a caller's vertex mask brought into it.
#include <hip/hip_runtime.h>

#include "solve.hpp"  // solve_transpose_graph
#include "solve6.hpp"
#include "solve6_internal.hpp"

namespace dfa {

namespace {

// ------------------------------------------------------------------------------------ graphs
// nearest node of every vertex (the key of the vertex sort).  A vertex WITHOUT a nearest node (NaN coordinates: the k-NN
// returns -1 for it) is filed under the last node: the sort is a permutation of ALL N vertices — a key the transposition
// skipped would leave positions [vptr[D], N) of the solver's arrays unwritten — and such a vertex keeps its row of -1
// ids and zero weights, i.e. it is passed through unchanged by every kernel, as it was before the sort existed.
__global__ __launch_bounds__(256) void s6_near_kernel(const int32_t* __restrict__ idx_nat, int N, int k, int D,
                                                      int32_t* __restrict__ near) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const int n = idx_nat[(size_t)v * k];
    near[v]     = n >= 0 && n < D ? n : D - 1;
}

// One workgroup per node: its vertices (grouped by the transposition in whatever order the atomics landed) sorted by
// index — a reproducible order — and gathered into the solver's arrays at their sorted positions, the radial basis
// weights normalised on the way (weight of node.cpp:29-36 divided by the row sum).
template <int K>
__global__ __launch_bounds__(256) void s6_permute_kernel(Solve6View s, const float* __restrict__ canon_user,
                                                         const float* __restrict__ canon_n_user,
                                                         const float* __restrict__ raw_w) {
    __shared__ uint32_t sortbuf[S6_SORT_MAX];
    const int a = blockIdx.x, tid = threadIdx.x, k = s.k;
    const int beg = s.vptr[a], len = s.vptr[a + 1] - beg;
    const bool sorted = len <= S6_SORT_MAX;
    if (sorted && len > 1) {
        int n2 = 1;
        while (n2 < len) n2 <<= 1;
        for (int i = tid; i < n2; i += 256) sortbuf[i] = i < len ? s.vlist[beg + i] : 0xffffffffu;
        __syncthreads();
        s6_sort_lds(sortbuf, n2, tid);
    } else if (sorted && len == 1 && tid == 0) {
        sortbuf[0] = s.vlist[beg];
    }
    __syncthreads();
    const bool wide = k == K;  // rows of K entries: 16-byte loads and stores
    for (int i = tid; i < len; i += 256) {
        const uint32_t v = sorted ? sortbuf[i] : s.vlist[beg + i];
        const size_t p   = (size_t)(beg + i);
        s.vperm[p]       = v;
#pragma unroll
        for (int c = 0; c < 3; ++c) s.canon_own[3 * p + c] = canon_user[3 * (size_t)v + c];
        if (canon_n_user)
#pragma unroll
            for (int c = 0; c < 3; ++c) s.canon_n_own[3 * p + c] = canon_n_user[3 * (size_t)v + c];
        float w[K];
        int32_t id[K];
        if (wide) {
#pragma unroll
            for (int q = 0; q < K / 4; ++q) {
                const float4 w4 = reinterpret_cast<const float4*>(raw_w + (size_t)v * K)[q];
                const int4 i4   = reinterpret_cast<const int4*>(s.idx_nat + (size_t)v * K)[q];
                w[4 * q] = w4.x, w[4 * q + 1] = w4.y, w[4 * q + 2] = w4.z, w[4 * q + 3] = w4.w;
                id[4 * q] = i4.x, id[4 * q + 1] = i4.y, id[4 * q + 2] = i4.z, id[4 * q + 3] = i4.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) w[j] = j < k ? raw_w[(size_t)v * k + j] : 0.f, id[j] = j < k ? s.idx_nat[(size_t)v * k + j] : -1;
        }
        float sum = 0.f;  // the row normalisation of blend6_device.hpp
#pragma unroll
        for (int j = 0; j < K; ++j) sum = weight_sum_add(sum, &w[j], j < k);
#pragma unroll
        for (int j = 0; j < K; ++j) w[j] = normalised_weight(&w[j], sum);
        if (wide) {
#pragma unroll
            for (int q = 0; q < K / 4; ++q) {
                reinterpret_cast<float4*>(s.wn + p * K)[q] = make_float4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
                reinterpret_cast<int4*>(s.idx + p * K)[q]  = make_int4(id[4 * q], id[4 * q + 1], id[4 * q + 2], id[4 * q + 3]);
            }
        } else {
            for (int j = 0; j < k; ++j) s.idx[p * k + j] = id[j], s.wn[p * k + j] = w[j];
        }
    }
}

// k nearest OTHER nodes from a (k + 1)-NN list of the nodes among themselves
__global__ __launch_bounds__(256) void s6_reg_graph_kernel(const int32_t* __restrict__ raw, int D, int kreg, int k,
                                                           int32_t* __restrict__ reg_idx) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= D) return;
    int o = 0;
    for (int j = 0; j < kreg && o < k; ++j) {
        const int m = raw[(size_t)n * kreg + j];
        if (m >= 0 && m != n) reg_idx[(size_t)n * k + o++] = m;
    }
    for (; o < k; ++o) reg_idx[(size_t)n * k + o] = -1;
}

__global__ void s6_pattern_reset_kernel(Solve6State* st) { st->overflow = 0, st->max_row_blocks = 0; }

// a caller's per-vertex mask brought into the solver's vertex order (what s6_warp does the other way round): a lane per
// sorted position, bytes normalised to 0 / 1
__global__ __launch_bounds__(256) void s6_gather_mask_kernel(const uint32_t* __restrict__ vperm, int N,
                                                             const uint8_t* __restrict__ mask, uint8_t* __restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < N) out[v] = mask[vperm[v]] != 0;
}

}  // namespace

hipError_t s6_gather_mask(const Solve6View& s, const uint8_t* mask, uint8_t* out, hipStream_t st) {
    if (s.N == 0) return hipSuccess;
    s6_gather_mask_kernel<<<(s.N + 255) / 256, 256, 0, st>>>(s.vperm, s.N, mask, out);
    return hipGetLastError();
}

hipError_t s6_build_graph(const Solve6View& s, Solve6State* state, const float* canon_user, const float* canon_n_user,
                          const float* raw_w, const int32_t* raw_reg, int kreg, hipStream_t st,
                          const S6RegHierarchy* hierarchy) {
    s6_pattern_reset_kernel<<<1, 1, 0, st>>>(state);
    hipError_t e = hipSuccess;
    if (s.N > 0) {
        // the solver's vertex order: by nearest node (counting sort), by index inside a node
        s6_near_kernel<<<(s.N + 255) / 256, 256, 0, st>>>(s.idx_nat, s.N, s.k, s.D, s.near);
        e = solve_transpose_graph(s.near, (size_t)s.N, s.D, s.blk_hist, s.vptr, s.vlist, st);
        if (e != hipSuccess) return e;
        K6DISPATCH(s6_permute_kernel, s.k, <<<s.D, 256, 0, st>>>(s, canon_user, canon_n_user, raw_w));
    }
    if (hierarchy) {  // the rows of the multi-level graph instead (reg_hierarchy.hip)
        e = reg_hierarchy_rows(s.node_pos, s.D, raw_reg, kreg, *hierarchy, s.k, s.reg_idx, st);
        if (e != hipSuccess) return e;
    } else
        s6_reg_graph_kernel<<<(s.D + 255) / 256, 256, 0, st>>>(raw_reg, s.D, kreg, s.k, s.reg_idx);
    e = solve_transpose_graph(s.idx, (size_t)s.N * s.k, s.D, s.blk_hist, s.node_ptr, s.node_list, st);
    if (e != hipSuccess) return e;
    e = solve_transpose_graph(s.reg_idx, (size_t)s.D * s.k, s.D, s.blk_hist, s.rnode_ptr, s.rnode_list, st);
    if (e != hipSuccess) return e;
    return s6_launch_pattern(s, state, st);
}

}  // namespace dfa
