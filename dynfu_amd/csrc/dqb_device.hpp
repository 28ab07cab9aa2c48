// dqb_device.hpp — what a point does with its neighbour list (KnnList, knn_device.hpp): the reference's ordered dual-quaternion
// blend (calc_dqb) and the support rule of Warpfield::getUnsupportedVertices (support_quotient, support_min).  Shared by the warp
// kernels (warp.hip) and the warped TSDF sweeps (warped_sweep_device.hpp, warped_color_device.hpp), which blend and decide with
// the same functions.
#pragma once
#include <hip/hip_runtime.h>

#include "dq_device.hpp"
#include "knn_device.hpp"

namespace dfa {

// Warpfield::calcDQB (warp_field.cpp:127-148) given the neighbour list
template <int K>
__device__ __forceinline__ DQ calc_dqb(const KnnList<K>& nb, int k, const float* __restrict__ node_pos,
                                       const float* __restrict__ node_dq, const float* __restrict__ node_w, f3 p) {
    DQ sum = dq_identity();  // :133
    // the neighbours' positions, radii and transforms four at a time by unconditional loads (an absent neighbour reads node 0
    // and is skipped): with the loads inside the `if` they were k dependent round trips.  Same products in the same order.
    constexpr int G = K < 4 ? K : 4;
#pragma unroll
    for (int h = 0; h < K; h += G) {
        f3 g[G];
        float r[G];
        DQ q[G];
        bool on[G];
#pragma unroll
        for (int jj = 0; jj < G; ++jj) {
            const int j = h + jj;
            on[jj]      = j < k && nb.index(j) >= 0;
            const int n = on[jj] ? nb.index(j) : 0;
            g[jj] = mk3(node_pos[3 * n], node_pos[3 * n + 1], node_pos[3 * n + 2]), r[jj] = node_w[n];
            q[jj] = dq_load(node_dq + 8 * (size_t)n);
        }
#pragma unroll
        for (int jj = 0; jj < G; ++jj)
            if (on[jj]) sum = dq_mul(sum, dq_scale(q[jj], transformation_weight(g[jj], r[jj], p)));  // :139-141
    }
    return dq_normalize(sum);  // :145
}

// Warpfield::getUnsupportedVertices (warp_field.cpp:34-62): the support quotient |p - g_m| / dg_w_m of one node (:45-46 —
// pow(float, int) is double arithmetic, the root is rounded to float on assignment) ...
__device__ __forceinline__ float support_quotient(f3 p, const float* __restrict__ node_pos, const float* __restrict__ node_w, int m) {
    const double dx = (double)(p.x - node_pos[3 * m]), dy = (double)(p.y - node_pos[3 * m + 1]),
                 dz = (double)(p.z - node_pos[3 * m + 2]);
    return (float)sqrt(dx * dx + dy * dy + dz * dz) / node_w[m];
}
// ... and its minimum over the neighbour list: the point is unsupported when this is >= 1 (:53)
template <int K>
__device__ __forceinline__ float support_min(const KnnList<K>& best, int k, const float* __restrict__ node_pos,
                                             const float* __restrict__ node_w, f3 p) {
    float mn = __builtin_huge_valf();  // :40
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k && best.index(j) >= 0) {
            const float q = support_quotient(p, node_pos, node_w, best.index(j));
            if (q <= mn) mn = q;  // :48-50
        }
    }
    return mn;
}

}  // namespace dfa
