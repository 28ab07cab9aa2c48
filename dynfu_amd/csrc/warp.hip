// warp.hip — gfx950 kernels for the warp itself: what a point does with its k nearest deformation nodes.  Warpfield::warpToLive
// with its own search (warp_to_live_kernel) or with a neighbour list that is already known (warp_graph_kernel), and the blended
// transform / the support flags at arbitrary points (dqb_support_kernel).  The searches are knn_device.hpp's, the ordered
// dual-quaternion blend and the support rule dqb_device.hpp's.
#include <hip/hip_runtime.h>

#include "dq_device.hpp"
#include "dqb_device.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"

namespace dfa {

// Warpfield::warpToLive (warp_field.cpp:150-171)
template <int K, bool GRID>
__global__ __launch_bounds__(256) void warp_to_live_kernel(const float* __restrict__ node_pos,
                                                           const float* __restrict__ node_dq,
                                                           const float* __restrict__ node_w, int D, int k,
                                                           const float* __restrict__ verts,
                                                           const float* __restrict__ normals, int N,
                                                           float* __restrict__ out_verts,
                                                           float* __restrict__ out_normals, KnnGridView grid) {
    __shared__ float4 tile[GRID ? 1 : KNN_TILE];
    const int v       = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = v < N;
    f3 p              = mk3(0.f, 0.f, 0.f);
    if (active) p = mk3(verts[3 * (size_t)v], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2]);
    KnnList<K> best;
    if (GRID) {
        if (!active) return;
        knn_grid_query<K>(*grid.desc, grid.cell_start, grid.sorted, p, best);
    } else {
        knn_scan<K>(node_pos, D, p, best, tile);
        if (!active) return;
    }
    const DQ dq = calc_dqb<K>(best, k, node_pos, node_dq, node_w, p);
    const f3 o  = dq_transform(dq, p);
    out_verts[3 * (size_t)v] = o.x, out_verts[3 * (size_t)v + 1] = o.y, out_verts[3 * (size_t)v + 2] = o.z;
    if (normals && out_normals) {
        // transformNormal == transformVertex formula (dual_quaternion.hpp:217-228)
        const f3 nn = dq_transform(dq, mk3(normals[3 * (size_t)v], normals[3 * (size_t)v + 1],
                                           normals[3 * (size_t)v + 2]));
        out_normals[3 * (size_t)v] = nn.x, out_normals[3 * (size_t)v + 1] = nn.y,
                                out_normals[3 * (size_t)v + 2] = nn.z;
    }
}

// warpToLive with a neighbour list that is already known (the solver plan's data graph of the same vertices and
// nodes): the same calcDQB and transform as warp_to_live_kernel, without searching again
template <int K>
__global__ __launch_bounds__(256) void warp_graph_kernel(const float* __restrict__ node_pos,
                                                         const float* __restrict__ node_dq,
                                                         const float* __restrict__ node_w, int k,
                                                         const int32_t* __restrict__ idx, const float* __restrict__ verts,
                                                         const float* __restrict__ normals, int N,
                                                         float* __restrict__ out_verts, float* __restrict__ out_normals) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    KnnList<K> nb;
    nb.init();
    if (k == K && K % 4 == 0 && (reinterpret_cast<uintptr_t>(idx) & 15u) == 0) {  // (uniform) the vertex's k neighbours by 16-byte loads
#pragma unroll
        for (int h = 0; h < K / 4; ++h) {
            const int4 n4 = reinterpret_cast<const int4*>(idx + (size_t)v * K)[h];
            nb.set_index(4 * h, n4.x), nb.set_index(4 * h + 1, n4.y), nb.set_index(4 * h + 2, n4.z), nb.set_index(4 * h + 3, n4.w);
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) {
                const int n = idx[(size_t)v * k + j];
                nb.set_index(j, n);
            }
    }
    const f3 p  = mk3(verts[3 * (size_t)v], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2]);
    const DQ dq = calc_dqb<K>(nb, k, node_pos, node_dq, node_w, p);
    const f3 o  = dq_transform(dq, p);
    out_verts[3 * (size_t)v] = o.x, out_verts[3 * (size_t)v + 1] = o.y, out_verts[3 * (size_t)v + 2] = o.z;
    if (normals && out_normals) {
        const f3 nn = dq_transform(dq, mk3(normals[3 * (size_t)v], normals[3 * (size_t)v + 1], normals[3 * (size_t)v + 2]));
        out_normals[3 * (size_t)v] = nn.x, out_normals[3 * (size_t)v + 1] = nn.y, out_normals[3 * (size_t)v + 2] = nn.z;
    }
}

// Warpfield::calcDQB (warp_field.cpp:127-148) at arbitrary points: the blended transform itself (new nodes
// are seeded with it, warp_field.cpp:78) — and Warpfield::getUnsupportedVertices (warp_field.cpp:34-62):
// a vertex is unsupported when min_j |v - g_j| / dg_w_j >= 1 over its k nearest nodes.
// FLAGS_ONLY: the instantiation of Warpfield::getUnsupportedVertices (no blended transform: 117 -> ~60 VGPRs at K = 8, twice
// the waves per SIMD for a kernel that is a chain of dependent loads)
template <int K, bool GRID, bool FLAGS_ONLY>
__global__ __launch_bounds__(256) void dqb_support_kernel(const float* __restrict__ node_pos,
                                                          const float* __restrict__ node_dq,
                                                          const float* __restrict__ node_w, int D, int k,
                                                          const float* __restrict__ pts, int n,
                                                          float* __restrict__ out_dq, uint8_t* __restrict__ out_flag,
                                                          KnnGridView grid) {
    __shared__ float4 tile[GRID ? 1 : KNN_TILE];
    const int v       = blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = v < n;
    f3 p              = mk3(0.f, 0.f, 0.f);
    if (active) p = mk3(pts[3 * (size_t)v], pts[3 * (size_t)v + 1], pts[3 * (size_t)v + 2]);
    auto quotient = [&](int m) __attribute__((always_inline)) { return support_quotient(p, node_pos, node_w, m); };
    KnnList<K> best;
    if (GRID) {
        if (!active) return;
        if (FLAGS_ONLY && k >= 1) {
            // Flags only (Warpfield::getUnsupportedVertices): the NEAREST node is one of the k nearest whatever k is, so a
            // vertex inside that node's radius is supported (min <= its quotient < 1) without the other k - 1 — the 1-NN
            // search stops in shell 0 / 1 and keeps no sorted list.  Almost every vertex of a tracked surface ends here; the
            // others (a farther node with a wider radius may still support them) take the full search below.
            KnnList<1> near;
            knn_grid_query<1, true>(*grid.desc, grid.cell_start, grid.sorted, p, near);
            const int m = near.index(0);
            if (m >= 0 && quotient(m) < 1.f) {
                out_flag[v] = 0;
                return;
            }
        }
        knn_grid_query<K>(*grid.desc, grid.cell_start, grid.sorted, p, best);
    } else {
        knn_scan<K>(node_pos, D, p, best, tile);
        if (!active) return;
    }
    if (!FLAGS_ONLY && out_dq) dq_store(out_dq + 8 * (size_t)v, calc_dqb<K>(best, k, node_pos, node_dq, node_w, p));
    if (out_flag) {
        float mn = __builtin_huge_valf();  // :40
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (j < k && best.index(j) >= 0) {
                const float q = quotient(best.index(j));
                if (q <= mn) mn = q;  // :48-50
            }
        }
        out_flag[v] = mn >= 1.f ? 1 : 0;  // :53
    }
}

// ------------------------------------------------------------------------------ launchers

hipError_t launch_warp_to_live(const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                               const float* verts, const float* normals, int N, float* out_verts, float* out_normals,
                               const KnnGridView* grid, hipStream_t s) {
    if (N == 0) return hipSuccess;
    dim3 block(256), gridDim((N + 255) / 256);
    const bool use_grid = grid != nullptr;
    KnnGridView g       = use_grid ? *grid : KnnGridView{};
    KGDISPATCH(warp_to_live_kernel, k, use_grid,
               <<<gridDim, block, 0, s>>>(node_pos, node_dq, node_w, D, k, verts, normals, N, out_verts, out_normals, g));
    return hipGetLastError();
}

hipError_t launch_dqb_support(const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                              const float* pts, int n, float* out_dq, uint8_t* out_flag, const KnnGridView* grid,
                              hipStream_t s) {
    if (n == 0) return hipSuccess;
    dim3 block(256), gridDim((n + 255) / 256);
    const bool use_grid = grid != nullptr;
    KnnGridView g       = use_grid ? *grid : KnnGridView{};
#define DQBK(KK, GG)                                                                                                         \
    do {                                                                                                                    \
        if (out_flag && !out_dq) dqb_support_kernel<KK, GG, true><<<gridDim, block, 0, s>>>(node_pos, node_dq, node_w, D, k, pts, n, out_dq, out_flag, g);  \
        else dqb_support_kernel<KK, GG, false><<<gridDim, block, 0, s>>>(node_pos, node_dq, node_w, D, k, pts, n, out_dq, out_flag, g);                     \
    } while (0)
    if (use_grid) {
        if (k <= 4) DQBK(4, true);
        else if (k <= 8) DQBK(8, true);
        else DQBK(16, true);
    } else {
        if (k <= 4) DQBK(4, false);
        else if (k <= 8) DQBK(8, false);
        else DQBK(16, false);
    }
#undef DQBK
    return hipGetLastError();
}

hipError_t launch_warp_graph(const float* node_pos, const float* node_dq, const float* node_w, int k, const int32_t* idx,
                             const float* verts, const float* normals, int N, float* out_verts, float* out_normals,
                             hipStream_t s) {
    if (N == 0) return hipSuccess;
    dim3 block(256), gridDim((N + 255) / 256);
    if (k <= 4) warp_graph_kernel<4><<<gridDim, block, 0, s>>>(node_pos, node_dq, node_w, k, idx, verts, normals, N, out_verts, out_normals);
    else if (k <= 8) warp_graph_kernel<8><<<gridDim, block, 0, s>>>(node_pos, node_dq, node_w, k, idx, verts, normals, N, out_verts, out_normals);
    else warp_graph_kernel<16><<<gridDim, block, 0, s>>>(node_pos, node_dq, node_w, k, idx, verts, normals, N, out_verts, out_normals);
    return hipGetLastError();
}

}  // namespace dfa
