// knn.hip — dfa_knn: the k nearest deformation nodes of every query and their RBF transformation weights
// (Warpfield::getWeightsAndNearestNeighbours, warp_field.cpp:99-125), by the exact searches of knn_device.hpp: one wave per
// query for a few queries over the grid, one lane per query otherwise — over the grid (knn_grid.hip) or by the exhaustive scan.
#include <hip/hip_runtime.h>

#include "dev_switch.hpp"
#include "dq_device.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"

namespace dfa {

template <int K>
__global__ __launch_bounds__(256) void knn_wave_kernel(const float* __restrict__ node_pos,
                                                       const float* __restrict__ node_w, int D,
                                                       const float* __restrict__ query, int n_query, int k,
                                                       int32_t* __restrict__ idx, float* __restrict__ weights,
                                                       KnnGridView grid) {
    const int v    = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= n_query) return;
    const KnnGridDesc g = *grid.desc;
    const f3 q = mk3(query[3 * (size_t)v], query[3 * (size_t)v + 1], query[3 * (size_t)v + 2]);
    int near[K];
    knn_wave_search<K>(g, grid.cell_start, grid.sorted, q, lane, near);
    if (lane != 0) return;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) {
            const int node         = near[j];
            idx[(size_t)v * k + j] = node;
            if (weights) {
                float w = 0.f;
                if (node >= 0)
                    w = transformation_weight(mk3(node_pos[3 * node], node_pos[3 * node + 1], node_pos[3 * node + 2]),
                                              node_w[node], q);
                weights[(size_t)v * k + j] = w;
            }
        }
}

// ONE_LOOP (grid searches): a lane walks the nine rows around its cell in one loop (knn_walk.hpp); false — development builds,
// DFA_KNN_ONE_LOOP=0 — keeps the nine wave-wide loops
template <int K, bool GRID, bool ONE_LOOP = GRID>
__global__ __launch_bounds__(256) void knn_kernel(const float* __restrict__ node_pos,
                                                  const float* __restrict__ node_w, int D,
                                                  const float* __restrict__ query, int n_query, int k,
                                                  int32_t* __restrict__ idx, float* __restrict__ weights,
                                                  KnnGridView grid) {
    static_assert(GRID || !ONE_LOOP, "the walk is the grid search's");
    __shared__ float4 tile[GRID ? 1 : KNN_TILE];
    __shared__ KnnWalkSlots<ONE_LOOP> slots;
    const int v       = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = v < n_query;
    f3 q              = mk3(0.f, 0.f, 0.f);
    if (active) q = mk3(query[3 * (size_t)v], query[3 * (size_t)v + 1], query[3 * (size_t)v + 2]);
    KnnList<K> best;
    if (GRID) {
        if (!active) return;
        knn_grid_query<K, false, ONE_LOOP>(*grid.desc, grid.cell_start, grid.sorted, q, best, false, D, slots.of_lane());
    } else {
        knn_scan<K>(node_pos, D, q, best, tile);
        if (!active) return;
    }
    int out_i[K];
    float out_w[K];
    knn_ids_weights<K>(best, k, node_pos, node_w, weights != nullptr, q, out_i, out_w);
    // (uniform) a query's k ids / weights are 16 or 32 contiguous bytes: 16-byte stores where the caller's arrays allow them
    if (k == K && K % 4 == 0 && ((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(weights)) & 15u) == 0) {
#pragma unroll
        for (int h = 0; h < K / 4; ++h) {
            reinterpret_cast<int4*>(idx + (size_t)v * K)[h] = make_int4(out_i[4 * h], out_i[4 * h + 1], out_i[4 * h + 2], out_i[4 * h + 3]);
            if (weights)
                reinterpret_cast<float4*>(weights + (size_t)v * K)[h] = make_float4(out_w[4 * h], out_w[4 * h + 1], out_w[4 * h + 2], out_w[4 * h + 3]);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) {
            idx[(size_t)v * k + j] = out_i[j];
            if (weights) weights[(size_t)v * k + j] = out_w[j];
        }
}

hipError_t launch_knn(const float* node_pos, const float* node_w, int D, const float* query, int n_query, int k,
                      int32_t* idx, float* weights, const KnnGridView* grid, hipStream_t s) {
    if (n_query == 0) return hipSuccess;
    dim3 block(256), gridDim((n_query + 255) / 256);
    const bool use_grid = grid != nullptr;
    KnnGridView g       = use_grid ? *grid : KnnGridView{};
    if (use_grid && n_query <= 32768) {  // few queries: one wave per query
        dim3 wgrid((n_query + 3) / 4);
        if (k <= 4) knn_wave_kernel<4><<<wgrid, block, 0, s>>>(node_pos, node_w, D, query, n_query, k, idx, weights, g);
        else if (k <= 8) knn_wave_kernel<8><<<wgrid, block, 0, s>>>(node_pos, node_w, D, query, n_query, k, idx, weights, g);
        else knn_wave_kernel<16><<<wgrid, block, 0, s>>>(node_pos, node_w, D, query, n_query, k, idx, weights, g);
        return hipGetLastError();
    }
#ifdef DFA_DEV_AB
    if (use_grid && !knn_one_loop()) {
        if (k <= 4) knn_kernel<4, true, false><<<gridDim, block, 0, s>>>(node_pos, node_w, D, query, n_query, k, idx, weights, g);
        else if (k <= 8) knn_kernel<8, true, false><<<gridDim, block, 0, s>>>(node_pos, node_w, D, query, n_query, k, idx, weights, g);
        else knn_kernel<16, true, false><<<gridDim, block, 0, s>>>(node_pos, node_w, D, query, n_query, k, idx, weights, g);
        return hipGetLastError();
    }
#endif
    KGDISPATCH(knn_kernel, k, use_grid, <<<gridDim, block, 0, s>>>(node_pos, node_w, D, query, n_query, k, idx, weights, g));
    return hipGetLastError();
}

}  // namespace dfa
