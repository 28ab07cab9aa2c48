// warped_sweep_device.hpp — the body of the warped TSDF sweeps, once: what a lane does with its WBZ voxels of a brick.  The
// four kernel families of tsdf_warped.hip are this body under two compile-time policies:
//   * where a voxel's neighbour list comes from: a search (SearchedNeighbours: the node grid, or a scan of all the nodes) or
//     the stored row of the k-NN field (StoredNeighbours);
//   * how a supported voxel moves, and through which frames: the reference-mode blend in the volume's frame (ReferenceWarp)
//     or the north-star (6-DoF) blend in the node frame (NorthStarWarp).
// The support rule and the blends read index(j) of a list only, so a stored row and a searched list are the same to them.
#pragma once
#include <hip/hip_runtime.h>

#include "blend6_device.hpp"
#include "device_math.hpp"
#include "dq_device.hpp"
#include "dqb_device.hpp"
#include "knn_device.hpp"
#include "knn_field_device.hpp"
#include "tsdf_integrate_device.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------ neighbour sources
// A source knows the workgroup's brick — the lane's column x(), y() and the brick's first slice z0() —, says whether the brick
// is `active` — may hold a supported voxel; an inactive brick asks for no list — and fills the list of the lane's voxel of
// slice u, at the search position q.

// The brick is the workgroup's place in the launch grid, active when the support pre-pass marked it.  GRID: the neighbours
// come from the node grid (knn_grid_query); otherwise (few nodes) from a scan of all of them.  The grid's descriptor is read
// only by an active brick of the grid form.
template <int K, bool GRID>
struct SearchedNeighbours {
    const bool active;  // (uniform)
    const float* __restrict__ node_pos;
    const int D;
    const KnnGridView& grid;
    KnnGridDesc g{};
    __device__ __forceinline__ int x() const { return blockIdx.x * WBX + threadIdx.x; }
    __device__ __forceinline__ int y() const { return blockIdx.y * WBY + threadIdx.y; }
    __device__ __forceinline__ int z0() const { return blockIdx.z * WBZ; }
    __device__ __forceinline__ void begin() {
        if (GRID && active) g = *grid.desc;
    }
    __device__ __forceinline__ void list(int, f3 q, KnnList<K>& best) const {
        if (GRID) {
            knn_grid_query<K>(g, grid.cell_start, grid.sorted, q, best);
        } else {
            best.init();
            for (int j = 0; j < D; ++j) best.push(dist2(q, node_pos[3 * j], node_pos[3 * j + 1], node_pos[3 * j + 2]), j);
        }
    }
};

// The brick is the field's (field_brick), active when it has a record; the list is the row the field stores for the voxel
// (the field's frame is the call's: the C ABI compares the 12 floats).
template <int K>
struct StoredNeighbours {
    const FieldBrick b;
    const bool active;  // (uniform)
    const int32_t* __restrict__ ids;
    const int k;
    __device__ __forceinline__ StoredNeighbours(const FieldBrick& b_, const int32_t* __restrict__ ids_, int k_)
        : b(b_), active(b_.rec >= 0), ids(ids_), k(k_) {}
    __device__ __forceinline__ int x() const { return b.x0 + threadIdx.x; }
    __device__ __forceinline__ int y() const { return b.y0 + threadIdx.y; }
    __device__ __forceinline__ int z0() const { return b.z0; }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void list(int u, f3, KnnList<K>& best) const { field_list<K>(field_row(ids, b.rec, k, u), k, best); }
};

// ------------------------------------------------------------------------------------------ warps
// A warp gives the search position of a voxel at v, moves a supported voxel from there, and takes the result to the camera.

// Reference mode: nodes in the volume's frame; p = dq_transform(calcDQB(v), v) — Warpfield::warpToLive, vertex only —, then
// vc = R p + t.
struct ReferenceWarp {
    const Aff3& vol2cam;
    const f3 t;
    __device__ __forceinline__ explicit ReferenceWarp(const Aff3& vol2cam_)
        : vol2cam(vol2cam_), t(mk3(vol2cam_.t[0], vol2cam_.t[1], vol2cam_.t[2])) {}
    __device__ __forceinline__ f3 position(f3 v) const { return v; }
    template <int K>
    __device__ __forceinline__ f3 move(const KnnList<K>& best, int k, const float* __restrict__ node_pos,
                                       const float* __restrict__ node_dq, const float* __restrict__ node_w, f3 v) const {
        return dq_transform(calc_dqb<K>(best, k, node_pos, node_dq, node_w, v), v);
    }
    __device__ __forceinline__ f3 to_camera(f3 p) const { return mulR(vol2cam, p) + t; }
};

// North-star nodes live in the camera frame of frame 0, not in the volume's, so a voxel is taken to the node frame first:
// c = R_n v + t_n (vol2node); the search, the support rule and the blend happen at c, and the blended point goes on to the
// camera by node2cam.  Either transform may be absent (identity: no product is made).
struct NorthStarWarp {
    const Aff3& vol2node;
    const int has_vol2node;
    const Aff3& node2cam;
    const int has_node2cam;
    __device__ __forceinline__ f3 position(f3 v) const { return to_node_frame(vol2node, has_vol2node, v); }
    // the plan's graph row of a vertex at c (dfa_knn's ids and weights, s6_permute's normalisation), then s6_warp_kernel's rule
    template <int K>
    __device__ __forceinline__ f3 move(const KnnList<K>& best, int k, const float* __restrict__ node_pos,
                                       const float* __restrict__ node_dq, const float* __restrict__ node_w, f3 c) const {
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
        f3 p = c;
        if (B.m > 0.f) p = blend_point<K>(B, c);
        return p;
    }
    // (uniform)
    __device__ __forceinline__ f3 to_camera(f3 p) const {
        return has_node2cam ? mulR(node2cam, p) + mk3(node2cam.t[0], node2cam.t[1], node2cam.t[2]) : p;
    }
};

// ------------------------------------------------------------------------------------------ the body
// One lane of block = (64, 4): a wave spans 64 voxels in x, the block 4 rows in y, a lane the WBZ voxels (x, y, z0 ..) — one
// brick per workgroup.  The lane's voxels are loaded before any search (256-byte row segments per wave); per slice: the
// voxel's position, its list, Warpfield::getUnsupportedVertices' rule (support_min), the move; an unsupported voxel — every
// voxel of an inactive brick — is left alone (!rigid: DFA_WARPED_SKIP) or stays where it is (rigid: DFA_WARPED_RIGID); from
// the camera frame on, the reference's integrate (tsdf_integrate_device.hpp), unchanged.  A voxel is stored only when the
// update changed it.  The policies are objects of the kernel, taken by reference: handed over by value, the searching
// reference-mode sweep came out 3.4 % slower at 512^3 (profiles/warped_sweep_body.md).
template <int K, class Neighbours, class Warp>
__device__ __forceinline__ void warped_sweep_brick(const IntegrateArgs& a, int rigid, Neighbours& nb, const Warp& warp, int k,
                                                   const float* __restrict__ node_pos, const float* __restrict__ node_dq,
                                                   const float* __restrict__ node_w) {
    const int x = nb.x(), y = nb.y();
    if (x >= a.X || y >= a.Y) return;
    const int z0 = nb.z0();
    const int nz = min(WBZ, a.Z - z0);

    const size_t slice = (size_t)a.X * a.Y;
    uint32_t* ptr      = a.vol + (size_t)x + (size_t)a.X * y + slice * z0;
    uint32_t cur[WBZ];
#pragma unroll
    for (int u = 0; u < WBZ; ++u) cur[u] = u < nz ? ptr[slice * u] : 0u;

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

// ------------------------------------------------------------------------------------------ what the sweeps' units share
// (tsdf_warped.hip and tsdf_warped_color.hip: the kernels' small parts and the launchers' argument block)

// (uniform) the pre-pass's mark of this workgroup's brick: a brick no node marked holds no supported voxel
__device__ __forceinline__ bool brick_marked(const uint8_t* __restrict__ bricks) {
    return bricks[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] != 0;
}

// the transforms of the north-star sweep
struct Warped6Frames {
    Aff3 vol2node, node2cam;  // read only where the flag below is set
    int has_vol2node, has_node2cam;
};

// the argument block of a warped sweep; vol2cam null: the identity (the sweep's frames are elsewhere and it is not read)
inline IntegrateArgs warped_args(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, int X, int Y, int Z,
                                 uint8_t* occ, const float voxel_size[3], float trunc_dist, int max_weight, const float* vol2cam,
                                 float fx, float fy, float cx, float cy) {
    IntegrateArgs a;
    a.dists = dists, a.dists_step = dists_step, a.cols = cols, a.rows = rows;
    a.vol = vol, a.X = X, a.Y = Y, a.Z = Z;
    const OccDims od = occ_dims(X, Y, Z);
    a.occ = occ, a.ox = od.ox, a.oy = od.oy, a.occ_known = 0;
    a.vsx = voxel_size[0], a.vsy = voxel_size[1], a.vsz = voxel_size[2];
    a.trunc      = trunc_dist;
    a.trunc_inv  = 1.f / trunc_dist;  // tsdf_volume.cu:106
    a.max_weight = max_weight;
    a.vol2cam    = aff3_from(vol2cam);
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.zchunk = WBZ;
    return a;
}

// the grid of a cached sweep.  SKIP: one workgroup per stored brick.  RIGID: every brick.
inline dim3 field_sweep_grid(const KnnFieldView& f, bool rigid, size_t records) {
    return rigid ? brick_grid(f.X, f.Y, f.Z) : dim3((unsigned)records);
}

}  // namespace dfa
