// tsdf_warped.hip — non-rigid TSDF fusion on gfx950: one depth frame integrated into the canonical volume THROUGH the warp
// field (DynamicFusion's "dense non-rigid surface fusion"; the reference lists the step and never does it,
// src/dynfu/dyn_fusion.cpp:39-47, :107-116).  All four sweeps and their launchers: through the reference-mode or the north-star
// (6-DoF) warp field, with a search per voxel or served from the k-NN field of knn_field.hip.
//
// Per voxel (warped_sweep_device.hpp, the one body of the four): v = (x, y, z) * voxel_size; its k nearest nodes
// (knn_device.hpp, dfa_knn's contract); the support rule of Warpfield::getUnsupportedVertices (support_min); a supported voxel
// moves to p = dq_transform(calcDQB(v), v) — the reference-mode blend of Warpfield::warpToLive (calc_dqb) — or by the blend of
// blend6_device.hpp in the nodes' own frame, an unsupported one is left alone (DFA_WARPED_SKIP) or stays at p = v
// (DFA_WARPED_RIGID); from the camera frame on, the reference's integrate (tsdf_integrate_device.hpp), unchanged.
//
// Layout.  A search per voxel is the cost of the searching form, so the voxels that cannot be supported never search:
//   * a BRICK is the footprint of one workgroup of the sweep, 64 x 4 x 1 voxels (two occupancy boxes wide, two high:
//     kernels.hpp OccDims).  A pre-pass (one wave per node) marks every brick whose box lies within w_max — the
//     largest node radius — of the node, by byte stores of 1 (warped_mark_device.hpp): the marked bricks are a superset of
//     the bricks with a supported voxel;
//   * an unmarked brick does no search: it returns at once in SKIP mode (no memory touched) and takes p = v in RIGID mode;
//   * a marked brick: one lane per voxel, a wave along x (its loads and stores are 256-byte row segments; the load is
//     issued before the search), then the search, the rule, the blend and the update.
// The cached form reads the list the field stores for the voxel where the searching form searches; its bricks are the
// field's stored ones (SKIP: one workgroup per stored brick and no other; RIGID: every brick, the table says which are stored).
// Node radii are positive (a radius <= 0 has no meaning in the support rule).  No fused contraction beyond the fmaf()s of
// the shared headers, no fast-math; vector stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.hpp"
#include "knn_field_device.hpp"
#include "warped_mark_device.hpp"
#include "warped_sweep_device.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------ support pre-pass
// the largest node radius (NaN radii are ignored: fmaxf)
__global__ __launch_bounds__(1024) void node_wmax_kernel(const float* __restrict__ node_w, int D, float* __restrict__ wmax) {
    __shared__ float part[16];
    float m = 0.f;
    for (int i = threadIdx.x; i < D; i += blockDim.x) m = fmaxf(m, node_w[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = fmaxf(m, part[w]);
        *wmax = m;
    }
}

// One wave per node: the bricks whose box of voxel POSITIONS comes within w_max of the node (mark_radius, mark_bricks_near).
__global__ __launch_bounds__(64) void mark_bricks_kernel(const float* __restrict__ node_pos, int D,
                                                         const float* __restrict__ wmax, int X, int Y, int Z, float vsx,
                                                         float vsy, float vsz, uint8_t* __restrict__ bricks) {
    const int node = blockIdx.x;
    if (node >= D) return;
    const float g[3] = {node_pos[3 * (size_t)node], node_pos[3 * (size_t)node + 1], node_pos[3 * (size_t)node + 2]};
    const float ext  = volume_extent(X, Y, Z, vsx, vsy, vsz);
    const float r    = mark_radius(*wmax, mk3(g[0], g[1], g[2]), ext);
    mark_bricks_near(g, r, X, Y, Z, vsx, vsy, vsz, bricks);
}

// As mark_bricks_kernel for nodes of the north-star warp field, each taken back to the volume's frame (node2vol =
// vol2node^-1) first (mark_radius_framed).
__global__ __launch_bounds__(64) void mark_bricks6_kernel(const float* __restrict__ node_pos, int D,
                                                          const float* __restrict__ wmax, const Aff3 node2vol, int has_frame,
                                                          float stretch, float tmax, int X, int Y, int Z, float vsx, float vsy,
                                                          float vsz, uint8_t* __restrict__ bricks) {
    const int node = blockIdx.x;
    if (node >= D) return;
    const f3 gn = mk3(node_pos[3 * (size_t)node], node_pos[3 * (size_t)node + 1], node_pos[3 * (size_t)node + 2]);
    const f3 gv = has_frame ? mulR(node2vol, gn) + mk3(node2vol.t[0], node2vol.t[1], node2vol.t[2]) : gn;
    const float g[3] = {gv.x, gv.y, gv.z};
    const float ext  = volume_extent(X, Y, Z, vsx, vsy, vsz);
    const float r    = mark_radius_framed(*wmax, gn, gv, ext, stretch, tmax);
    mark_bricks_near(g, r, X, Y, Z, vsx, vsy, vsz, bricks);
}

// ------------------------------------------------------------------------------------------ the sweeps
// block = (64, 4), one brick per workgroup: each kernel finds its brick, says where the neighbours come from and which warp
// moves a supported voxel, and runs warped_sweep_brick.  K holds k: 4, 8 or 16 in reference mode, 4 or 8 (k = 1..8) for the
// north-star field.

template <int K, bool GRID>
__global__ __launch_bounds__(256) void integrate_warped_kernel(const IntegrateArgs a, const float* __restrict__ node_pos,
                                                               const float* __restrict__ node_dq,
                                                               const float* __restrict__ node_w, int D, int k, int rigid,
                                                               const uint8_t* __restrict__ bricks, KnnGridView grid) {
    const bool marked = brick_marked(bricks);
    if (!marked && !rigid) return;
    SearchedNeighbours<K, GRID> nb{marked, node_pos, D, grid};
    const ReferenceWarp warp(a.vol2cam);
    warped_sweep_brick<K>(a, rigid, nb, warp, k, node_pos, node_dq, node_w);
}

template <int K, bool GRID>
__global__ __launch_bounds__(256) void integrate_warped6_kernel(const IntegrateArgs a, const Warped6Frames f,
                                                                const float* __restrict__ node_pos,
                                                                const float* __restrict__ node_dq,
                                                                const float* __restrict__ node_w, int D, int k, int rigid,
                                                                const uint8_t* __restrict__ bricks, KnnGridView grid) {
    const bool marked = brick_marked(bricks);
    if (!marked && !rigid) return;
    SearchedNeighbours<K, GRID> nb{marked, node_pos, D, grid};
    const NorthStarWarp warp{f.vol2node, f.has_vol2node, f.node2cam, f.has_node2cam};
    warped_sweep_brick<K>(a, rigid, nb, warp, k, node_pos, node_dq, node_w);
}

template <int K>
__global__ __launch_bounds__(256) void integrate_warped_field_kernel(const IntegrateArgs a, const FieldGeom g,
                                                                     const float* __restrict__ node_pos,
                                                                     const float* __restrict__ node_dq,
                                                                     const float* __restrict__ node_w, int rigid,
                                                                     const int32_t* __restrict__ table,
                                                                     const int32_t* __restrict__ coords,
                                                                     const int32_t* __restrict__ ids) {
    StoredNeighbours<K> nb(field_brick(g, table, coords, !rigid), ids, g.k);
    const ReferenceWarp warp(a.vol2cam);
    warped_sweep_brick<K>(a, rigid, nb, warp, g.k, node_pos, node_dq, node_w);
}

template <int K>
__global__ __launch_bounds__(256) void integrate_warped6_field_kernel(const IntegrateArgs a, const FieldGeom g, const Aff3 node2cam,
                                                                      int has_node2cam, const float* __restrict__ node_pos,
                                                                      const float* __restrict__ node_dq,
                                                                      const float* __restrict__ node_w, int rigid,
                                                                      const int32_t* __restrict__ table,
                                                                      const int32_t* __restrict__ coords,
                                                                      const int32_t* __restrict__ ids) {
    StoredNeighbours<K> nb(field_brick(g, table, coords, !rigid), ids, g.k);
    const NorthStarWarp warp{g.vol2node, g.has_frame, node2cam, has_node2cam};
    warped_sweep_brick<K>(a, rigid, nb, warp, g.k, node_pos, node_dq, node_w);
}

// ------------------------------------------------------------------------------------------ launchers
hipError_t launch_tsdf_integrate_warped(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, int X, int Y,
                                        int Z, uint8_t* occ, const float voxel_size[3], float trunc_dist, int max_weight,
                                        const float vol2cam[12], float fx, float fy, float cx, float cy, const float* node_pos,
                                        const float* node_dq, const float* node_w, int D, int k, bool rigid,
                                        const KnnGridView* grid, uint8_t* bricks, float* wmax, hipStream_t s) {
    const IntegrateArgs a = warped_args(dists, dists_step, cols, rows, vol, X, Y, Z, occ, voxel_size, trunc_dist, max_weight, vol2cam,
                                        fx, fy, cx, cy);
    hipError_t e = hipMemsetAsync(bricks, 0, knn_field_bricks(X, Y, Z), s);
    if (e != hipSuccess) return e;
    if (D > 0) {
        node_wmax_kernel<<<1, 1024, 0, s>>>(node_w, D, wmax);
        mark_bricks_kernel<<<D, 64, 0, s>>>(node_pos, D, wmax, X, Y, Z, a.vsx, a.vsy, a.vsz, bricks);
    }
    const dim3 block(WBX, WBY), g3 = brick_grid(X, Y, Z);
    const KnnGridView gv = grid ? *grid : KnnGridView{};
    if (grid) KDISPATCH16(k, integrate_warped_kernel<KK, true><<<g3, block, 0, s>>>(a, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv));
    else KDISPATCH16(k, integrate_warped_kernel<KK, false><<<g3, block, 0, s>>>(a, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv));
    return hipGetLastError();
}

// vol2node checked and inverted on the host, in double: false when |R^T R - I| exceeds 1e-3 in some entry (the pre-pass
// measures distances in the volume's frame, so the product has to keep them).  node2vol: the inverse, rounded to float;
// stretch: 1 + twice the largest entry of |R^T R - I| found — x^T (R^T R - I) x <= 3 dev |x|^2, so a distance in the
// volume's frame is at most 1 / sqrt(1 - 3 dev) <= 1 + 2 dev times the distance of the images in the node frame;
// tmax: the largest |t_n|.  vol2node == nullptr: the identity.
bool warped6_frame(const float* vol2node, float node2vol[12], float* stretch, float* tmax) {
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (!vol2node) {
        for (int i = 0; i < 12; ++i) node2vol[i] = i < 9 ? (float)I[i] : 0.f;
        *stretch = 1.f, *tmax = 0.f;
        return true;
    }
    double R[9], t[3], dev = 0.0;
    for (int i = 0; i < 9; ++i) R[i] = vol2node[i];
    for (int i = 0; i < 3; ++i) t[i] = vol2node[9 + i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double e = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j] - I[3 * i + j];
            if (!(std::fabs(e) <= 1e-3)) return false;  // (NaN entries end here too)
            dev = std::max(dev, std::fabs(e));
        }
    // the inverse by cofactors (det is within 2e-3 of +-1 here)
    const double c[9] = {R[4] * R[8] - R[5] * R[7], R[2] * R[7] - R[1] * R[8], R[1] * R[5] - R[2] * R[4],
                         R[5] * R[6] - R[3] * R[8], R[0] * R[8] - R[2] * R[6], R[2] * R[3] - R[0] * R[5],
                         R[3] * R[7] - R[4] * R[6], R[1] * R[6] - R[0] * R[7], R[0] * R[4] - R[1] * R[3]};
    const double det = R[0] * c[0] + R[1] * c[3] + R[2] * c[6];
    for (int i = 0; i < 9; ++i) node2vol[i] = (float)(c[i] / det);
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(t[i])) return false;
        node2vol[9 + i] = (float)(-(c[3 * i] * t[0] + c[3 * i + 1] * t[1] + c[3 * i + 2] * t[2]) / det);
    }
    *stretch = (float)(1.0 + 2.0 * dev);
    *tmax    = (float)std::max(std::max(std::fabs(t[0]), std::fabs(t[1])), std::fabs(t[2]));
    return true;
}

// the support pre-pass of the searching north-star sweeps (here and in tsdf_warped_color.hip): the flags cleared, then marked
hipError_t launch_warped6_mark_bricks(const float* node_pos, const float* node_w, int D, bool has_vol2node, const float node2vol[12],
                                      float stretch, float tmax, int X, int Y, int Z, const float voxel_size[3], uint8_t* bricks,
                                      float* wmax, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(bricks, 0, knn_field_bricks(X, Y, Z), s);
    if (e != hipSuccess) return e;
    if (D > 0) {
        node_wmax_kernel<<<1, 1024, 0, s>>>(node_w, D, wmax);
        mark_bricks6_kernel<<<D, 64, 0, s>>>(node_pos, D, wmax, aff3_from(node2vol), has_vol2node ? 1 : 0, stretch, tmax, X, Y, Z,
                                             voxel_size[0], voxel_size[1], voxel_size[2], bricks);
    }
    return hipSuccess;
}

hipError_t launch_tsdf_integrate_warped6(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, int X, int Y,
                                         int Z, uint8_t* occ, const float voxel_size[3], float trunc_dist, int max_weight,
                                         const float* vol2node, const float* node2cam, const float node2vol[12], float stretch,
                                         float tmax, float fx, float fy, float cx, float cy, const float* node_pos,
                                         const float* node_dq, const float* node_w, int D, int k, bool rigid,
                                         const KnnGridView* grid, uint8_t* bricks, float* wmax, hipStream_t s) {
    const IntegrateArgs a = warped_args(dists, dists_step, cols, rows, vol, X, Y, Z, occ, voxel_size, trunc_dist, max_weight, nullptr,
                                        fx, fy, cx, cy);  // (vol2cam is not read: the frames are in f)
    const Warped6Frames f{aff3_from(vol2node), aff3_from(node2cam), vol2node ? 1 : 0, node2cam ? 1 : 0};
    const hipError_t e = launch_warped6_mark_bricks(node_pos, node_w, D, vol2node != nullptr, node2vol, stretch, tmax, X, Y, Z,
                                                    voxel_size, bricks, wmax, s);
    if (e != hipSuccess) return e;
    const dim3 block(WBX, WBY), g3 = brick_grid(X, Y, Z);
    const KnnGridView gv = grid ? *grid : KnnGridView{};
    if (grid) KDISPATCH8(k, integrate_warped6_kernel<KK, true><<<g3, block, 0, s>>>(a, f, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv));
    else KDISPATCH8(k, integrate_warped6_kernel<KK, false><<<g3, block, 0, s>>>(a, f, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv));
    return hipGetLastError();
}

// the two sweeps with the neighbours read from the field f (records: its stored bricks; none in SKIP mode: nothing to do)
hipError_t launch_tsdf_integrate_warped_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol,
                                              uint8_t* occ, float trunc_dist, int max_weight, const float vol2cam[12], float fx,
                                              float fy, float cx, float cy, const float* node_pos, const float* node_dq,
                                              const float* node_w, bool rigid, const KnnFieldView& f, size_t records,
                                              hipStream_t s) {
    if (!rigid && records == 0) return hipSuccess;
    const IntegrateArgs a = warped_args(dists, dists_step, cols, rows, vol, f.X, f.Y, f.Z, occ, f.vs, trunc_dist, max_weight, vol2cam,
                                        fx, fy, cx, cy);
    const FieldGeom g = field_geom(f);
    const dim3 block(WBX, WBY), g3 = field_sweep_grid(f, rigid, records);
    KDISPATCH16(f.k, integrate_warped_field_kernel<KK><<<g3, block, 0, s>>>(a, g, node_pos, node_dq, node_w, rigid ? 1 : 0, f.table,
                                                                             f.coords, f.ids));
    return hipGetLastError();
}

hipError_t launch_tsdf_integrate_warped6_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol,
                                               uint8_t* occ, float trunc_dist, int max_weight, const float* node2cam, float fx,
                                               float fy, float cx, float cy, const float* node_pos, const float* node_dq,
                                               const float* node_w, bool rigid, const KnnFieldView& f, size_t records,
                                               hipStream_t s) {
    if (!rigid && records == 0) return hipSuccess;
    const IntegrateArgs a = warped_args(dists, dists_step, cols, rows, vol, f.X, f.Y, f.Z, occ, f.vs, trunc_dist, max_weight, nullptr,
                                        fx, fy, cx, cy);  // (vol2cam is not read: the frames are the field's and node2cam)
    const FieldGeom g = field_geom(f);
    const dim3 block(WBX, WBY), g3 = field_sweep_grid(f, rigid, records);
    KDISPATCH8(f.k, integrate_warped6_field_kernel<KK><<<g3, block, 0, s>>>(a, g, aff3_from(node2cam), node2cam ? 1 : 0, node_pos, node_dq,
                                                                             node_w, rigid ? 1 : 0, f.table, f.coords, f.ids));
    return hipGetLastError();
}

}  // namespace dfa
