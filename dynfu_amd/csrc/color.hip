// color.hip — dfa_color_sample on gfx950: the colour of the canonical model at its vertices, read from the colour volume
// dfa_tsdf_integrate_warped6_color fuses (one uint32 per voxel: bytes b, g, r and an 8-bit weight; 0 = no colour).
//
// One lane per vertex p, float32 throughout:
//   q = R p + t (to_volume: mulR's fused dot, then + t), or q = p without one;
//   g = q / voxel_size per axis (voxels sit at (x, y, z) * voxel_size, as in the sweeps); i0 = floor(g), f = g - i0;
//   over the 8 corners i0 + (dx, dy, dz) of the cell: t = (wx wy) wz with each factor f (d = 1) or 1 - f (d = 0); a corner
//   COUNTS when it lies inside the volume and the weight byte of its word is > 0; den = sum of t, s_c = sum of t c per
//   channel (fmaf(t, c, s_c)), both over the counting corners in the order dz, dy, dx (dx fastest);
//   den < 0.25 or a coordinate of g not finite: the output is 0, 0, 0, 0 — a vertex the colour volume has next to nothing
//   to say about; otherwise b, g, r = rintf(s_c / den) and a = 255.
// (A g outside [-1, dim) on some axis has no corner inside: den = 0, decided before anything is converted to int.)
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"

namespace dfa {

__global__ __launch_bounds__(256) void color_sample_kernel(const uint32_t* __restrict__ colors, int X, int Y, int Z, float vsx,
                                                           float vsy, float vsz, const float* __restrict__ vertices, int stride,
                                                           int N, const Aff3 to_volume, int has_frame, uint32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* v = vertices + (size_t)i * stride;
    f3 q           = mk3(v[0], v[1], v[2]);
    if (has_frame) q = mulR(to_volume, q) + mk3(to_volume.t[0], to_volume.t[1], to_volume.t[2]);
    const float g[3] = {q.x / vsx, q.y / vsy, q.z / vsz};
    const int dim[3] = {X, Y, Z};
    uint32_t word    = 0u;
    // (NaN fails the comparisons; +-inf lies outside)
    if (g[0] >= -1.f && g[0] < (float)X && g[1] >= -1.f && g[1] < (float)Y && g[2] >= -1.f && g[2] < (float)Z) {
        int i0[3];
        float f[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float fl = floorf(g[a]);
            i0[a] = (int)fl, f[a] = g[a] - fl;
        }
        float den = 0.f, s[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int d[3] = {c & 1, (c >> 1) & 1, c >> 2};
            bool in = true;
            int at[3];
            float w[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                at[a] = i0[a] + d[a];
                in    = in && at[a] >= 0 && at[a] < dim[a];
                w[a]  = d[a] ? f[a] : 1.f - f[a];
            }
            if (!in) continue;
            const uint32_t o = colors[(size_t)at[0] + (size_t)X * ((size_t)at[1] + (size_t)Y * (size_t)at[2])];
            if ((o >> 24) == 0u) continue;
            const float t = (w[0] * w[1]) * w[2];
            den += t;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s[ch] = fmaf(t, (float)((o >> (8 * ch)) & 255u), s[ch]);
        }
        if (den >= 0.25f) {
            word = 255u << 24;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) word |= ((uint32_t)rintf(s[ch] / den) & 255u) << (8 * ch);
        }
    }
    out[i] = word;
}

hipError_t launch_color_sample(const uint32_t* colors, int X, int Y, int Z, const float voxel_size[3], const float* vertices,
                               int stride, int N, const float* to_volume, uint8_t* out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    color_sample_kernel<<<(N + 255) / 256, 256, 0, s>>>(colors, X, Y, Z, voxel_size[0], voxel_size[1], voxel_size[2], vertices, stride,
                                                        N, aff3_from(to_volume), to_volume ? 1 : 0, (uint32_t*)out);
    return hipGetLastError();
}

}  // namespace dfa
