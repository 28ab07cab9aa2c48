// warped_mark_device.hpp — the brick marking shared by the support pre-pass of the warped sweeps (tsdf_warped.hip: every
// node at the largest radius) and the stored set of the k-NN field (knn_field.hip: every node at its own radius): the bricks
// near a point, and the ONE statement of how far "near" has to reach for the marked set to be a superset.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "warped_bricks.hpp"

namespace dfa {

// The bricks whose box of voxel POSITIONS comes within r of the point g (volume frame), marked by the 64 lanes of one wave.
// The candidate range is widened by a voxel either side.
__device__ __forceinline__ void mark_bricks_near(const float (&g)[3], float r, int X, int Y, int Z, float vsx, float vsy,
                                                 float vsz, uint8_t* __restrict__ bricks) {
    const float vs[3] = {vsx, vsy, vsz};
    const int dim[3]  = {X, Y, Z};
    const int bs[3]   = {WBX, WBY, WBZ};
    int b0[3], nb[3];
    for (int c = 0; c < 3; ++c) {
        // voxel indices whose position can lie in [g - r, g + r]; the clamps also make the conversions safe (a NaN or an
        // infinite radius ends as the whole axis)
        const float inv = 1.f / fabsf(vs[c]);
        float lo = (g[c] - r) * inv - 1.f, hi = (g[c] + r) * inv + 1.f;
        if (vs[c] < 0.f) {
            const float t = -lo;
            lo = -hi, hi = t;
        }
        if (!(lo >= 0.f)) lo = 0.f;
        if (!(hi <= (float)(dim[c] - 1))) hi = (float)(dim[c] - 1);
        if (lo > hi) return;  // (uniform) the node is farther than w_max from the volume along this axis
        b0[c] = (int)lo / bs[c];
        nb[c] = (int)hi / bs[c] - b0[c] + 1;
    }
    const int nbx = (X + WBX - 1) / WBX, nby = (Y + WBY - 1) / WBY;
    const long total = (long)nb[0] * nb[1] * nb[2];
    for (long i = threadIdx.x; i < total; i += 64) {
        const int b[3] = {b0[0] + (int)(i % nb[0]), b0[1] + (int)((i / nb[0]) % nb[1]), b0[2] + (int)(i / ((long)nb[0] * nb[1]))};
        float d2 = 0.f;
        for (int c = 0; c < 3; ++c) {
            // the brick's first and last voxel position on this axis
            const float pa = (float)(b[c] * bs[c]) * vs[c], pb = (float)min(b[c] * bs[c] + bs[c] - 1, dim[c] - 1) * vs[c];
            const float d  = fmaxf(fmaxf(fminf(pa, pb) - g[c], g[c] - fmaxf(pa, pb)), 0.f);
            d2 += d * d;
        }
        if (!(d2 > r * r)) bricks[((size_t)b[2] * nby + b[1]) * nbx + b[0]] = 1;  // (racing stores of the same byte)
    }
}

// ---- the marking radius.  A voxel at v is supported by the node at g with reach w when |v - g| < w in float arithmetic
// (w: the largest node radius for the sweeps' pre-pass — no node within w_max of a voxel means every quotient
// |v - g| / w >= |v - g| / w_max >= 1 —, the node's own radius for the field).  The radius r handed to mark_bricks_near must
// not be smaller than any |v - g| the support rule can accept.

// the longest edge of the volume, in metres
__device__ __forceinline__ float volume_extent(int X, int Y, int Z, float vsx, float vsy, float vsz) {
    return fmaxf(fmaxf(fabsf(vsx) * (float)X, fabsf(vsy) * (float)Y), fabsf(vsz) * (float)Z);
}
__device__ __forceinline__ float max_abs(f3 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fabsf(v.z)); }

// A node in the volume's frame.  Conservative: the reach is widened by 1e-3 relative and a millionth of the largest
// coordinate in play (the positions, differences and roots of the support rule are rounded at 1e-7 relative).
__device__ __forceinline__ float mark_radius(float w, f3 g, float ext) { return w * 1.001f + 1e-6f * fmaxf(ext, max_abs(g)); }

// A node at gn in a node frame, taken back to gv = R' gn + t' in the volume's (node2vol = vol2node^-1; stretch and tmax:
// warped6_frame's).  A supported voxel has |c - gn| < w in the node frame, hence |v - gv| <= stretch w in the volume's, up to
// the rounding of the two products: c = R_n v + t_n in the sweep and gv = R' gn + t' in the marking kernel, each a few ulp of
// the coordinates that enter it.  The reach is widened by the 1e-3 relative of mark_radius times the stretch, and by a
// millionth of the SUM of the coordinates in play in either frame: the volume's extent (twice: |R_n v| reaches sqrt 3 of
// it), the node's coordinates in both frames and the translation.
__device__ __forceinline__ float mark_radius_framed(float w, f3 gn, f3 gv, float ext, float stretch, float tmax) {
    const float L = 2.f * ext + max_abs(gn) + max_abs(gv) + tmax;
    return w * 1.001f * stretch + 1e-6f * L;
}

}  // namespace dfa
