// tsdf_warped.hip — non-rigid TSDF fusion on gfx950: one depth frame integrated into the canonical volume THROUGH the warp
// field (DynamicFusion's "dense non-rigid surface fusion"; the reference lists the step and never does it,
// src/dynfu/dyn_fusion.cpp:39-47, :107-116).
//
// Per voxel: v = (x, y, z) * voxel_size; its k nearest nodes (knn_device.hpp, dfa_knn's contract); the support rule of
// Warpfield::getUnsupportedVertices (support_min); a supported voxel moves to p = dq_transform(calcDQB(v), v) — the
// reference-mode blend of Warpfield::warpToLive (calc_dqb) —, an unsupported one is left alone (DFA_WARPED_SKIP) or stays at
// p = v (DFA_WARPED_RIGID); from vc = R p + t on, the reference's integrate (tsdf_integrate_device.hpp: voxel_tsdf,
// voxel_update<false>), unchanged.
//
// Layout.  A search per voxel is the cost of this first form, so the voxels that cannot be supported never search:
//   * a BRICK is the footprint of one workgroup of the sweep, 64 x 4 x 1 voxels (two occupancy boxes wide, two high:
//     kernels.hpp OccDims).  A pre-pass (one wave per node) marks every brick whose box lies within w_max — the
//     largest node radius — of the node, by byte stores of 1.  No node within w_max of a voxel means every quotient
//     |v - g| / w >= |v - g| / w_max >= 1: the marked bricks are a superset of the bricks with a supported voxel;
//   * an unmarked brick does no search: it returns at once in SKIP mode (no memory touched) and takes p = v in RIGID mode;
//   * a marked brick: one lane per voxel, a wave along x (its loads and stores are 256-byte row segments; the load is
//     issued before the search), then the search, the rule, the blend and the update.  A voxel is stored only when the
//     update changed it.
// Node radii are positive (a radius <= 0 has no meaning in the support rule).  No fused contraction beyond the fmaf()s of
// the shared headers, no fast-math; vector stores only.
//
// The second half of the file is the same sweep for the north-star (6-DoF) warp field (dfa_tsdf_integrate_warped6): nodes in
// their own frame, the blend of blend6_device.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "blend6_device.hpp"
#include "device_math.hpp"
#include "dq_device.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"
#include "tsdf_integrate_device.hpp"
#include "warped_mark_device.hpp"

namespace dfa {

// (the brick, 64 x 4 x 1 voxels: warped_bricks.hpp, shared with the k-NN field of knn_field.hip)
size_t warped_brick_count(int X, int Y, int Z) {
    return (size_t)((X + WBX - 1) / WBX) * (size_t)((Y + WBY - 1) / WBY) * (size_t)((Z + WBZ - 1) / WBZ);
}

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

// (mark_bricks_near — the bricks within r of a point, marked by one wave: warped_mark_device.hpp)

// One wave per node: the bricks whose box of voxel POSITIONS comes within w_max of the node.  Conservative: the radius
// is widened by 1e-3 relative and a millionth of the largest coordinate in play (the positions, differences and roots of
// the support rule are rounded at 1e-7 relative), the candidate range by a voxel either side.
__global__ __launch_bounds__(64) void mark_bricks_kernel(const float* __restrict__ node_pos, int D,
                                                         const float* __restrict__ wmax, int X, int Y, int Z, float vsx,
                                                         float vsy, float vsz, uint8_t* __restrict__ bricks) {
    const int node = blockIdx.x;
    if (node >= D) return;
    const float g[3] = {node_pos[3 * (size_t)node], node_pos[3 * (size_t)node + 1], node_pos[3 * (size_t)node + 2]};
    const float ext  = fmaxf(fmaxf(fabsf(vsx) * (float)X, fabsf(vsy) * (float)Y), fabsf(vsz) * (float)Z);
    const float r = *wmax * 1.001f + 1e-6f * fmaxf(ext, fmaxf(fmaxf(fabsf(g[0]), fabsf(g[1])), fabsf(g[2])));
    mark_bricks_near(g, r, X, Y, Z, vsx, vsy, vsz, bricks);
}

// ------------------------------------------------------------------------------------------ the sweep
// block = (64, 4): a wave spans 64 voxels in x, the block 4 rows in y, a lane WBZ voxels in z — one brick per workgroup.
// GRID: the neighbours come from the node grid (knn_grid_query); otherwise (few nodes) from a scan of all of them.
template <int K, bool GRID>
__global__ __launch_bounds__(256) void integrate_warped_kernel(const IntegrateArgs a, const float* __restrict__ node_pos,
                                                               const float* __restrict__ node_dq,
                                                               const float* __restrict__ node_w, int D, int k, int rigid,
                                                               const uint8_t* __restrict__ bricks, KnnGridView grid) {
    // (uniform) a brick no node marked holds no supported voxel
    const bool marked = bricks[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] != 0;
    if (!marked && !rigid) return;
    const int x = blockIdx.x * WBX + threadIdx.x;
    const int y = blockIdx.y * WBY + threadIdx.y;
    if (x >= a.X || y >= a.Y) return;
    const int z0 = blockIdx.z * WBZ;
    const int nz = min(WBZ, a.Z - z0);

    const size_t slice = (size_t)a.X * a.Y;
    uint32_t* ptr      = a.vol + (size_t)x + (size_t)a.X * y + slice * z0;
    uint32_t cur[WBZ];
#pragma unroll
    for (int u = 0; u < WBZ; ++u) cur[u] = u < nz ? ptr[slice * u] : 0u;

    KnnGridDesc g{};
    if (GRID && marked) g = *grid.desc;
    const f3 t = mk3(a.vol2cam.t[0], a.vol2cam.t[1], a.vol2cam.t[2]);
    bool any   = false;  // an update happened: the voxel may hold a weight now
    for (int u = 0; u < nz; ++u) {
        const f3 v = mk3((float)x * a.vsx, (float)y * a.vsy, (float)(z0 + u) * a.vsz);  // the voxel's corner (tsdf_volume.cu:60), by multiplication
        f3 p       = v;
        bool go    = rigid != 0;
        if (marked) {
            KnnList<K> best;
            if (GRID) {
                knn_grid_query<K>(g, grid.cell_start, grid.sorted, v, best);
            } else {
                best.init();
                for (int j = 0; j < D; ++j) best.push(dist2(v, node_pos[3 * j], node_pos[3 * j + 1], node_pos[3 * j + 2]), j);
            }
            if (support_min<K>(best, k, node_pos, node_w, v) < 1.f) {  // Warpfield::getUnsupportedVertices' rule
                p  = dq_transform(calc_dqb<K>(best, k, node_pos, node_dq, node_w, v), v);  // Warpfield::warpToLive, vertex only
                go = true;
            }
        }
        if (!go) continue;
        const f3 vc = mulR(a.vol2cam, p) + t;
        float tsdf;
        if (!voxel_tsdf(a, vc, tsdf)) continue;
        const uint32_t upd = voxel_update<false>(a, cur[u], tsdf);
        if (upd != cur[u]) ptr[slice * u] = upd;
        any = true;
    }
    if (a.occ) {
        // the two occupancy boxes a wave's row crosses (32 voxels each): lanes 0 and 32 write theirs when a lane of that half
        // updated a voxel.  Both bits: the update may have left a negative distance.  Rows y and y + 1 share a byte and store
        // the same value.
        const unsigned long long m = __ballot(any);
        if ((threadIdx.x & 31) == 0 && ((m >> threadIdx.x) & 0xffffffffull) != 0ull)
            a.occ[(size_t)(x / 32) + (size_t)a.ox * ((size_t)(y / 2) + (size_t)a.oy * (size_t)(z0 / 8))] = 3;
    }
}

// ------------------------------------------------------------------------------------------ launcher
hipError_t launch_tsdf_integrate_warped(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, int X, int Y,
                                        int Z, uint8_t* occ, const float voxel_size[3], float trunc_dist, int max_weight,
                                        const float vol2cam[12], float fx, float fy, float cx, float cy, const float* node_pos,
                                        const float* node_dq, const float* node_w, int D, int k, bool rigid,
                                        const KnnGridView* grid, uint8_t* bricks, float* wmax, hipStream_t s) {
    IntegrateArgs a;
    a.dists = dists, a.dists_step = dists_step, a.cols = cols, a.rows = rows;
    a.vol = vol, a.X = X, a.Y = Y, a.Z = Z;
    const OccDims od = occ_dims(X, Y, Z);
    a.occ = occ, a.ox = od.ox, a.oy = od.oy, a.occ_known = 0;
    a.vsx = voxel_size[0], a.vsy = voxel_size[1], a.vsz = voxel_size[2];
    a.trunc      = trunc_dist;
    a.trunc_inv  = 1.f / trunc_dist;  // tsdf_volume.cu:106
    a.max_weight = max_weight;
    for (int i = 0; i < 9; ++i) a.vol2cam.m[i] = vol2cam[i];
    for (int i = 0; i < 3; ++i) a.vol2cam.t[i] = vol2cam[9 + i];
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.zchunk = WBZ;

    hipError_t e = hipMemsetAsync(bricks, 0, warped_brick_count(X, Y, Z), s);
    if (e != hipSuccess) return e;
    if (D > 0) {
        node_wmax_kernel<<<1, 1024, 0, s>>>(node_w, D, wmax);
        mark_bricks_kernel<<<D, 64, 0, s>>>(node_pos, D, wmax, X, Y, Z, a.vsx, a.vsy, a.vsz, bricks);
    }
    dim3 block(WBX, WBY), g3((X + WBX - 1) / WBX, (Y + WBY - 1) / WBY, (Z + WBZ - 1) / WBZ);
    const KnnGridView gv = grid ? *grid : KnnGridView{};
#define WARPED(KK)                                                                                                                   \
    do {                                                                                                                             \
        if (grid) integrate_warped_kernel<KK, true><<<g3, block, 0, s>>>(a, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv);  \
        else integrate_warped_kernel<KK, false><<<g3, block, 0, s>>>(a, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv);      \
    } while (0)
    if (k <= 4) WARPED(4);
    else if (k <= 8) WARPED(8);
    else WARPED(16);
#undef WARPED
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ the north-star sweep
// dfa_tsdf_integrate_warped6: the same bricks, pre-pass idea, occupancy rule and store rule with the north-star (6-DoF)
// blend of blend6_device.hpp.  North-star nodes live in the camera frame of frame 0, not in the volume's, so a voxel is
// taken to the node frame first: c = R_n v + t_n (vol2node), the search, the support rule and the blend happen at c, and
// the blended point goes on to the camera by node2cam.  Either transform may be absent (identity: no product is made).
struct Warped6Frames {
    Aff3 vol2node, node2cam;  // read only where the flag below is set
    int has_vol2node, has_node2cam;
};

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

// One wave per node, as mark_bricks_kernel, with the node taken back to the volume's frame (node2vol = vol2node^-1) first.
// A supported voxel has |c - g| < w <= w_max in the node frame, hence |v - g'| <= stretch w_max in the volume's, up to
// the rounding of the two products: c = R_n v + t_n in the sweep and g' = R' g + t' here, each a few ulp of the
// coordinates that enter it.  The radius is widened by the 1e-3 relative of mark_bricks_kernel times the stretch, and by a
// millionth of the SUM of the coordinates in play in either frame: the volume's extent (twice: |R_n v| reaches sqrt 3 of
// it), the node's coordinates in both frames and the translation.
__global__ __launch_bounds__(64) void mark_bricks6_kernel(const float* __restrict__ node_pos, int D,
                                                          const float* __restrict__ wmax, const Aff3 node2vol, int has_frame,
                                                          float stretch, float tmax, int X, int Y, int Z, float vsx, float vsy,
                                                          float vsz, uint8_t* __restrict__ bricks) {
    const int node = blockIdx.x;
    if (node >= D) return;
    const f3 gn = mk3(node_pos[3 * (size_t)node], node_pos[3 * (size_t)node + 1], node_pos[3 * (size_t)node + 2]);
    const f3 gv = has_frame ? mulR(node2vol, gn) + mk3(node2vol.t[0], node2vol.t[1], node2vol.t[2]) : gn;
    const float g[3] = {gv.x, gv.y, gv.z};
    const float ext  = fmaxf(fmaxf(fabsf(vsx) * (float)X, fabsf(vsy) * (float)Y), fabsf(vsz) * (float)Z);
    const float L    = 2.f * ext + fmaxf(fmaxf(fabsf(gn.x), fabsf(gn.y)), fabsf(gn.z)) +
                    fmaxf(fmaxf(fabsf(gv.x), fabsf(gv.y)), fabsf(gv.z)) + tmax;
    const float r = *wmax * 1.001f * stretch + 1e-6f * L;
    mark_bricks_near(g, r, X, Y, Z, vsx, vsy, vsz, bricks);
}

// block = (64, 4), one brick per workgroup, GRID as in integrate_warped_kernel.  K is 4 or 8 (k = 1..8).
template <int K, bool GRID>
__global__ __launch_bounds__(256) void integrate_warped6_kernel(const IntegrateArgs a, const Warped6Frames f,
                                                                const float* __restrict__ node_pos,
                                                                const float* __restrict__ node_dq,
                                                                const float* __restrict__ node_w, int D, int k, int rigid,
                                                                const uint8_t* __restrict__ bricks, KnnGridView grid) {
    // (uniform) a brick no node marked holds no supported voxel
    const bool marked = bricks[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] != 0;
    if (!marked && !rigid) return;
    const int x = blockIdx.x * WBX + threadIdx.x;
    const int y = blockIdx.y * WBY + threadIdx.y;
    if (x >= a.X || y >= a.Y) return;
    const int z0 = blockIdx.z * WBZ;
    const int nz = min(WBZ, a.Z - z0);

    const size_t slice = (size_t)a.X * a.Y;
    uint32_t* ptr      = a.vol + (size_t)x + (size_t)a.X * y + slice * z0;
    uint32_t cur[WBZ];
#pragma unroll
    for (int u = 0; u < WBZ; ++u) cur[u] = u < nz ? ptr[slice * u] : 0u;

    KnnGridDesc g{};
    if (GRID && marked) g = *grid.desc;
    bool any = false;  // an update happened: the voxel may hold a weight now
    for (int u = 0; u < nz; ++u) {
        const f3 v = mk3((float)x * a.vsx, (float)y * a.vsy, (float)(z0 + u) * a.vsz);  // the voxel's corner, by multiplication
        // (uniform) the voxel in the node frame
        const f3 c = f.has_vol2node ? mulR(f.vol2node, v) + mk3(f.vol2node.t[0], f.vol2node.t[1], f.vol2node.t[2]) : v;
        f3 p       = c;
        bool go    = rigid != 0;
        if (marked) {
            KnnList<K> best;
            if (GRID) {
                knn_grid_query<K>(g, grid.cell_start, grid.sorted, c, best);
            } else {
                best.init();
                for (int j = 0; j < D; ++j) best.push(dist2(c, node_pos[3 * j], node_pos[3 * j + 1], node_pos[3 * j + 2]), j);
            }
            if (support_min<K>(best, k, node_pos, node_w, c) < 1.f) {  // Warpfield::getUnsupportedVertices' rule, at c
                // the plan's graph row of a vertex at c (dfa_knn's ids and weights, s6_permute's normalisation), then
                // s6_warp_kernel's rule
                int id[K];
                float wn[K];
                knn_ids_weights<K>(best, k, node_pos, node_w, true, c, id, wn);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < K; ++j) sum = weight_sum_add(sum, &wn[j], j < k);
#pragma unroll
                for (int j = 0; j < K; ++j) wn[j] = normalised_weight(&wn[j], sum);
                Blend<K> B;
                blend<K>(node_dq, id, wn, k, B);
                if (B.m > 0.f) p = blend_point<K>(B, c);
                go = true;
            }
        }
        if (!go) continue;
        // (uniform) on to the camera
        const f3 vc = f.has_node2cam ? mulR(f.node2cam, p) + mk3(f.node2cam.t[0], f.node2cam.t[1], f.node2cam.t[2]) : p;
        float tsdf;
        if (!voxel_tsdf(a, vc, tsdf)) continue;
        const uint32_t upd = voxel_update<false>(a, cur[u], tsdf);
        if (upd != cur[u]) ptr[slice * u] = upd;
        any = true;
    }
    if (a.occ) {
        // as integrate_warped_kernel: lanes 0 and 32 write the occupancy box of their half of the row when it updated a voxel
        const unsigned long long m = __ballot(any);
        if ((threadIdx.x & 31) == 0 && ((m >> threadIdx.x) & 0xffffffffull) != 0ull)
            a.occ[(size_t)(x / 32) + (size_t)a.ox * ((size_t)(y / 2) + (size_t)a.oy * (size_t)(z0 / 8))] = 3;
    }
}

hipError_t launch_tsdf_integrate_warped6(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, int X, int Y,
                                         int Z, uint8_t* occ, const float voxel_size[3], float trunc_dist, int max_weight,
                                         const float* vol2node, const float* node2cam, const float node2vol[12], float stretch,
                                         float tmax, float fx, float fy, float cx, float cy, const float* node_pos,
                                         const float* node_dq, const float* node_w, int D, int k, bool rigid,
                                         const KnnGridView* grid, uint8_t* bricks, float* wmax, hipStream_t s) {
    IntegrateArgs a;
    a.dists = dists, a.dists_step = dists_step, a.cols = cols, a.rows = rows;
    a.vol = vol, a.X = X, a.Y = Y, a.Z = Z;
    const OccDims od = occ_dims(X, Y, Z);
    a.occ = occ, a.ox = od.ox, a.oy = od.oy, a.occ_known = 0;
    a.vsx = voxel_size[0], a.vsy = voxel_size[1], a.vsz = voxel_size[2];
    a.trunc      = trunc_dist;
    a.trunc_inv  = 1.f / trunc_dist;  // tsdf_volume.cu:106
    a.max_weight = max_weight;
    a.vol2cam    = Aff3{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};  // (not read: the frames are in f)
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.zchunk = WBZ;
    Warped6Frames f{a.vol2cam, a.vol2cam, vol2node ? 1 : 0, node2cam ? 1 : 0};
    Aff3 back = a.vol2cam;
    for (int i = 0; i < 12; ++i) {
        if (vol2node) (i < 9 ? f.vol2node.m[i] : f.vol2node.t[i - 9]) = vol2node[i];
        if (node2cam) (i < 9 ? f.node2cam.m[i] : f.node2cam.t[i - 9]) = node2cam[i];
        (i < 9 ? back.m[i] : back.t[i - 9]) = node2vol[i];
    }

    hipError_t e = hipMemsetAsync(bricks, 0, warped_brick_count(X, Y, Z), s);
    if (e != hipSuccess) return e;
    if (D > 0) {
        node_wmax_kernel<<<1, 1024, 0, s>>>(node_w, D, wmax);
        mark_bricks6_kernel<<<D, 64, 0, s>>>(node_pos, D, wmax, back, vol2node ? 1 : 0, stretch, tmax, X, Y, Z, a.vsx, a.vsy,
                                             a.vsz, bricks);
    }
    dim3 block(WBX, WBY), g3((X + WBX - 1) / WBX, (Y + WBY - 1) / WBY, (Z + WBZ - 1) / WBZ);
    const KnnGridView gv = grid ? *grid : KnnGridView{};
#define WARPED6(KK)                                                                                                                     \
    do {                                                                                                                                \
        if (grid) integrate_warped6_kernel<KK, true><<<g3, block, 0, s>>>(a, f, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv);  \
        else integrate_warped6_kernel<KK, false><<<g3, block, 0, s>>>(a, f, node_pos, node_dq, node_w, D, k, rigid ? 1 : 0, bricks, gv);      \
    } while (0)
    if (k <= 4) WARPED6(4);  // (as K6DISPATCH of solve6_internal.hpp)
    else WARPED6(8);
#undef WARPED6
    return hipGetLastError();
}

}  // namespace dfa
