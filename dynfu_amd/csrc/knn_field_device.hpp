// knn_field_device.hpp — what the k-NN field's own kernels (knn_field.hip) and the warped sweeps (tsdf_warped.hip, through
// warped_sweep_device.hpp) share: the ONE expression of a voxel's position, the field as a kernel takes it, the brick a
// workgroup of a cached sweep works on and the read of a stored row; and, for the hosts of both units, the brick grid.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"
#include "warped_bricks.hpp"

namespace dfa {

// The voxel's corner (tsdf_volume.cu:60), by multiplication.  Every search, merge and sweep forms a voxel's position by
// this expression and no other: the field's rows are exact only because all of them see the same bits.
__device__ __forceinline__ f3 voxel_position(int x, int y, int z, float vsx, float vsy, float vsz) {
    return mk3((float)x * vsx, (float)y * vsy, (float)z * vsz);
}
// ... taken to the node frame, c = R_n v + t_n, where there is one (uniform)
__device__ __forceinline__ f3 to_node_frame(const Aff3& vol2node, int has_frame, f3 v) {
    return has_frame ? mulR(vol2node, v) + mk3(vol2node.t[0], vol2node.t[1], vol2node.t[2]) : v;
}

// the field as the kernels take it
struct FieldGeom {
    int X, Y, Z, k;
    int nbx, nby;  // bricks along x and y
    float vsx, vsy, vsz;
    int has_frame;
    Aff3 vol2node;
};

inline FieldGeom field_geom(const KnnFieldView& f) {
    FieldGeom g;
    g.X = f.X, g.Y = f.Y, g.Z = f.Z, g.k = f.k;
    g.nbx = (f.X + WBX - 1) / WBX, g.nby = (f.Y + WBY - 1) / WBY;
    g.vsx = f.vs[0], g.vsy = f.vs[1], g.vsz = f.vs[2];
    g.has_frame = f.has_frame;
    g.vol2node  = aff3_from(f.has_frame ? f.vol2node : nullptr);
    return g;
}

// a voxel's search position
__device__ __forceinline__ f3 field_position(const FieldGeom& g, int x, int y, int z) {
    return to_node_frame(g.vol2node, g.has_frame, voxel_position(x, y, z, g.vsx, g.vsy, g.vsz));
}

// brick index of the table -> the brick's first voxel
__device__ __forceinline__ void brick_origin(const FieldGeom& g, int b, int& x0, int& y0, int& z0) {
    x0 = (b % g.nbx) * WBX, y0 = ((b / g.nbx) % g.nby) * WBY, z0 = (b / (g.nbx * g.nby)) * WBZ;
}

// What a workgroup of the cached sweeps works on.  LIST (SKIP mode): workgroup i takes stored brick i of the compact list —
// the bricks not stored hold no supported voxel and are never launched.  Otherwise (RIGID mode) the grid covers every brick
// and the table says which are stored.
struct FieldBrick {
    int x0, y0, z0, rec;
};
__device__ __forceinline__ FieldBrick field_brick(const FieldGeom& g, const int32_t* __restrict__ table,
                                                  const int32_t* __restrict__ coords, int list) {
    FieldBrick b;
    if (list) {
        b.rec = (int)blockIdx.x;
        brick_origin(g, coords[b.rec], b.x0, b.y0, b.z0);
    } else {
        b.x0 = blockIdx.x * WBX, b.y0 = blockIdx.y * WBY, b.z0 = blockIdx.z * WBZ;
        b.rec = table ? table[((size_t)blockIdx.z * g.nby + blockIdx.y) * g.nbx + blockIdx.x] : -1;  // (null: an empty field)
    }
    return b;
}

// this lane's row of slice u of record rec: slot j is at [j * WB_VOXELS]
template <class Id>  // (int32_t to write a row, const int32_t to read one)
__device__ __forceinline__ Id* field_row(Id* ids, int rec, int k, int u) {
    return ids + (size_t)rec * k * WB_VOXELS + ((u * WBY + threadIdx.y) * WBX + threadIdx.x);
}
// the voxel's stored row as the list the shared rules read (they read index(j) only)
template <int K>
__device__ __forceinline__ void field_list(const int32_t* __restrict__ row, int k, KnnList<K>& best) {
    int id[K];
#pragma unroll
    for (int j = 0; j < K; ++j) id[j] = j < k ? row[(size_t)j * WB_VOXELS] : -1;
#pragma unroll
    for (int j = 0; j < K; ++j) best.set_index(j, id[j]);
}

// ---- host side
// one workgroup per brick of the volume (here and not beside the brick in warped_bricks.hpp: that header is plain C++, no dim3)
inline dim3 brick_grid(int X, int Y, int Z) { return dim3((X + WBX - 1) / WBX, (Y + WBY - 1) / WBY, (Z + WBZ - 1) / WBZ); }

}  // namespace dfa
