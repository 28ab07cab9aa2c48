// vol_rows.hpp — row loads of the packed TSDF volume shared by the streaming sweeps of mc.hip (marching cubes) and
// extract.hip (point-cloud extraction).  A wave owns a row segment of 64 VX consecutive x voxels, a lane VX of them
// (one 16-byte load per row when VX = 4); the voxel after a lane's last one comes from the next lane by a shuffle.
// `A` is any argument block with the members vol, X, Y, Z.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dfa {
namespace {

// the VX voxels a lane owns in one row plus the voxel after them; zeros (weight 0) wherever the row or the voxel does
// not exist
template <int VX>
struct Row {
    uint32_t v[VX + 1];
};

template <int VX, class A>
__device__ __forceinline__ Row<VX> load_row(const A& a, int x0, int y, int z) {
    Row<VX> r;
#pragma unroll
    for (int i = 0; i <= VX; ++i) r.v[i] = 0u;
    const bool row_ok = y < a.Y && z < a.Z;
    const uint32_t* p = a.vol + (size_t)a.X * ((size_t)y + (size_t)a.Y * (size_t)z);
    if (row_ok && x0 < a.X) {
        if (VX == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(p + x0);
            r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
        } else {
            r.v[0] = p[x0];
        }
    }
    // the neighbour's first voxel; the last lane of the wave reads it from memory
    const uint32_t next = __shfl_down(r.v[0], 1, 64);
    if ((threadIdx.x & 63) == 63) {
        if (row_ok && x0 + VX < a.X) r.v[VX] = p[x0 + VX];
    } else {
        r.v[VX] = next;
    }
    return r;
}

// NR consecutive rows y .. y + NR - 1 of slice z.  The voxel after the wave's last one is fetched for
// all NR rows by ONE load instruction (lane r reads row r's) and handed to lane 63 by a readlane —
// the sweeps are bound by vector-memory instruction issue, not by bytes.
template <int VX, int NR, class A>
__device__ __forceinline__ void load_rows(const A& a, int x0, int y, int z, Row<VX> (&out)[NR]) {
    const int lane = threadIdx.x & 63;
    const bool z_ok = z < a.Z;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        Row<VX>& o = out[r];
#pragma unroll
        for (int i = 0; i <= VX; ++i) o.v[i] = 0u;
        const uint32_t* p = a.vol + (size_t)a.X * ((size_t)(y + r) + (size_t)a.Y * (size_t)z);
        if (z_ok && y + r < a.Y && x0 < a.X) {
            if (VX == 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(p + x0);
                o.v[0] = q.x, o.v[1] = q.y, o.v[2] = q.z, o.v[3] = q.w;
            } else {
                o.v[0] = p[x0];
            }
        }
    }
    const int xend = (x0 - lane * VX) + 64 * VX;  // first voxel of the next segment
    uint32_t extra = 0u;
    if (lane < NR && z_ok && y + lane < a.Y && xend < a.X)
        extra = a.vol[(size_t)xend + (size_t)a.X * ((size_t)(y + lane) + (size_t)a.Y * (size_t)z)];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const uint32_t next = __shfl_down(out[r].v[0], 1, 64);
        const uint32_t last = __shfl(extra, r, 64);
        out[r].v[VX]        = lane == 63 ? last : next;
    }
}

}  // namespace
}  // namespace dfa
