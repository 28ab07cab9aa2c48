// blend6_device.hpp — the north-star (6-DoF) blend of a point's k nearest nodes, shared by its two users: the solve and its
// warp (solve6_graph.hip: s6_permute normalises the weights once per plan; solve6_linearise.hip, solve6_update.hip:
// s6_linearise and s6_warp blend) and the warped TSDF
// sweep (warped_sweep_device.hpp: NorthStarWarp, one normalisation and blend per voxel).  Weights are the radial basis weights divided
// by their row sum; a neighbour takes part when its id is >= 0 and its normalised weight is not 0; every transform is taken
// to the hemisphere of the first such neighbour; a = sum w~ s r, b = sum w~ s d; the point is (a c a* + 2 b a*) / |a|^2.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "dq_device.hpp"

namespace dfa {

__device__ __forceinline__ Quat qconj(Quat a) { return Quat{a.w, -a.x, -a.y, -a.z}; }
__device__ __forceinline__ float qdot(Quat a, Quat b) { return a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ Quat pureq(f3 v) { return Quat{0.f, v.x, v.y, v.z}; }
__device__ __forceinline__ f3 qvec(Quat a) { return mk3(a.x, a.y, a.z); }

// The row normalisation: the float32 sum of the k raw weights in slot order, then every weight divided by the sum, or 0
// when the sum is not positive.  Two per-slot steps, run by the caller over its K slots (slots from k on hold 0):
//     float sum = 0.f;
//     for (j < K) sum = weight_sum_add(sum, &w[j], j < k);
//     for (j < K) w[j] = normalised_weight(&w[j], sum);
// A slot is taken by address and the loops stay with the caller on purpose: that is the form under which s6_permute_kernel
// compiles to the instructions it had with the arithmetic written in place (a whole-row function, or the weight by value,
// is simplified on its own before it is inlined and comes out as other code: tools/kernel_isa_diff.py).
__device__ __forceinline__ float weight_sum_add(float sum, const float* w, bool in_row) { return sum + (in_row ? *w : 0.f); }
__device__ __forceinline__ float normalised_weight(const float* w, float sum) { return sum > 0.f ? *w / sum : 0.f; }

// ------------------------------------------------------------------------------------ blend
template <int K>
struct Blend {
    Quat a, b;   // un-normalised blended real / dual parts
    float m;     // |a|^2
    float s[K];  // hemisphere sign of each neighbour (0 = unused slot)
};

template <int K>
__device__ __forceinline__ void blend(const float* __restrict__ dq, const int32_t* idx, const float* wn, int k,
                                      Blend<K>& B) {
    B.a = Quat{0.f, 0.f, 0.f, 0.f}, B.b = B.a;
    Quat r0   = Quat{1.f, 0.f, 0.f, 0.f};
    bool have = false;
    // the node transforms four at a time, by unconditional loads (a neighbour that is not there reads node 0 and is not
    // used): with the load inside the `if` the k gathers were k dependent round trips to L2
#pragma unroll
    for (int h = 0; h < K; h += 4) {
        DQ q[4];
        bool on[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = h + jj;
            on[jj]      = j < k && idx[j] >= 0 && wn[j] != 0.f;
            q[jj]       = dq_load(dq + 8 * (size_t)(on[jj] ? idx[j] : 0));
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = h + jj;
            B.s[j]      = 0.f;
            if (!on[jj]) continue;
            if (!have) r0 = q[jj].r, have = true;
            const float sg = qdot(q[jj].r, r0) < 0.f ? -1.f : 1.f;
            B.s[j]         = sg;
            const float w  = wn[j] * sg;
            B.a = qadd(B.a, qscale(q[jj].r, w)), B.b = qadd(B.b, qscale(q[jj].d, w));
        }
    }
    B.m = qdot(B.a, B.a);
}

template <int K>
__device__ __forceinline__ f3 blend_point(const Blend<K>& B, f3 c) {
    const Quat ac = qconj(B.a);
    const f3 u    = qvec(qmul(qmul(B.a, pureq(c)), ac));
    const f3 t    = qvec(qmul(B.b, ac));
    const float im = 1.f / B.m;
    return mk3((u.x + 2.f * t.x) * im, (u.y + 2.f * t.y) * im, (u.z + 2.f * t.z) * im);
}
template <int K>
__device__ __forceinline__ f3 blend_normal(const Blend<K>& B, f3 n) {
    const f3 u     = qvec(qmul(qmul(B.a, pureq(n)), qconj(B.a)));
    const float im = 1.f / B.m;
    return mk3(u.x * im, u.y * im, u.z * im);
}

}  // namespace dfa
