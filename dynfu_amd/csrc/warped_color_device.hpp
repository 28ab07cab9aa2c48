// warped_color_device.hpp — colour fused through the north-star warp field: the body of the coloured sweeps of
// tsdf_warped_color.hip (dfa_tsdf_integrate_warped6_color).  It is warped_sweep_brick (warped_sweep_device.hpp) — the same
// policies, the same expressions on the same values up to voxel_tsdf and voxel_update<false> — with the colour rule added
// behind the distance, in a body of its own: the four kernels of tsdf_warped.hip keep their code.
//
// Colour volume: one uint32 per voxel in the TSDF volume's order; bytes 0, 1, 2 = b, g, r (the byte order of the images,
// pixels b, g, r, x), byte 3 an 8-bit colour weight; 0 = no colour.
//
// The rule, for a voxel whose voxel_tsdf returned true with tsdf < 1.0f (inside the truncation band, not clamped):
//   pixel  the texel (px, py) voxel_tsdf fetched the distance from;  o the old word, w = o >> 24;
//   per channel c with input byte in:  c' = (c w + in + ((w + 1) >> 1)) / (w + 1), integers, truncating division
//          (c w + in + ((w + 1) >> 1) <= 255 (w + 1) + (w + 1) / 2: c' <= 255);
//   w' = min(w + 1, max_color_weight);  the word is stored only when it changed.
// The colour word is read only here — a few percent of the updated voxels —, never up front beside cur[]: the sweep's
// reads on a brick without a surface stay the TSDF row alone, and no second row of registers is held across the search.
#pragma once
#include <hip/hip_runtime.h>

#include "dqb_device.hpp"
#include "warped_sweep_device.hpp"

namespace dfa {

// The texel of voxel_tsdf at vc, for a voxel voxel_tsdf returned true for: its expressions on its values (the compiler
// merges the two; stated again so that voxel_tsdf — and every kernel built on it — stays as it is).
__device__ __forceinline__ void voxel_texel(const IntegrateArgs& a, f3 vc, int& px, int& py) {
    float qx, qy;
    div_xy_by_z(vc.x, vc.y, vc.z, qx, qy);
    px = (int)fmaf(a.fx, qx, a.cx);
    py = (int)fmaf(a.fy, qy, a.cy);
}

// the rule above on the word *word with the pixel pix (b, g, r, x)
__device__ __forceinline__ void color_update(uint32_t* word, uint32_t pix, int max_color_weight) {
    const uint32_t o = *word;
    const uint32_t w = o >> 24, den = w + 1u, half = den >> 1;
    uint32_t n = (uint32_t)min((int)den, max_color_weight) << 24;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const uint32_t c = (o >> (8 * ch)) & 255u, in = (pix >> (8 * ch)) & 255u;
        n |= ((c * w + in + half) / den) << (8 * ch);
    }
    if (n != o) *word = n;
}

// One lane of block = (64, 4), as warped_sweep_brick.  TSDF: the volume is given — its words and the occupancy map come out
// as warped_sweep_brick leaves them; otherwise no TSDF word is read or written and the map is not touched.
template <int K, bool TSDF, class Neighbours, class Warp>
__device__ __forceinline__ void warped_color_brick(const IntegrateArgs& a, const ColorArgs& c, int rigid, Neighbours& nb,
                                                   const Warp& warp, int k, const float* __restrict__ node_pos,
                                                   const float* __restrict__ node_dq, const float* __restrict__ node_w) {
    const int x = nb.x(), y = nb.y();
    if (x >= a.X || y >= a.Y) return;
    const int z0 = nb.z0();
    const int nz = min(WBZ, a.Z - z0);

    const size_t slice = (size_t)a.X * a.Y;
    const size_t first = (size_t)x + (size_t)a.X * y + slice * z0;
    uint32_t* ptr      = TSDF ? a.vol + first : nullptr;
    uint32_t cur[WBZ];
#pragma unroll
    for (int u = 0; u < WBZ; ++u) cur[u] = TSDF && u < nz ? ptr[slice * u] : 0u;

    nb.begin();
    bool any = false;  // an update happened: the voxel may hold a weight now
    for (int u = 0; u < nz; ++u) {
        const f3 q = warp.position(voxel_position(x, y, z0 + u, a.vsx, a.vsy, a.vsz));
        f3 p       = q;
        bool go    = rigid != 0;
        if (nb.active) {
            KnnList<K> best;
            nb.list(u, q, best);
            if (support_min<K>(best, k, node_pos, node_w, q) < 1.f) {
                p  = warp.template move<K>(best, k, node_pos, node_dq, node_w, q);
                go = true;
            }
        }
        if (!go) continue;
        const f3 vc = warp.to_camera(p);
        float tsdf;
        if (!voxel_tsdf(a, vc, tsdf)) continue;
        if (TSDF) {
            const uint32_t upd = voxel_update<false>(a, cur[u], tsdf);
            if (upd != cur[u]) ptr[slice * u] = upd;
            any = true;
        }
        if (tsdf < 1.0f) {
            int px, py;
            voxel_texel(a, vc, px, py);
            const uint32_t pix = *(const uint32_t*)(c.image + (size_t)py * c.image_step + (size_t)px * 4);
            color_update(c.colors + first + slice * u, pix, c.max_color_weight);
        }
    }
    if (TSDF && a.occ) {
        // (warped_sweep_brick's: lanes 0 and 32 write the box of their half of the row when a lane of it updated a voxel)
        const unsigned long long m = __ballot(any);
        if ((threadIdx.x & 31) == 0 && ((m >> threadIdx.x) & 0xffffffffull) != 0ull)
            a.occ[(size_t)(x / 32) + (size_t)a.ox * ((size_t)(y / 2) + (size_t)a.oy * (size_t)(z0 / 8))] = 3;
    }
}

}  // namespace dfa
