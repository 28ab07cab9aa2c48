// tsdf_warped_color.hip — dfa_tsdf_integrate_warped6_color on gfx950: one registered depth + colour frame fused into the
// canonical TSDF volume and its colour volume THROUGH the north-star (6-DoF) warp field, in one sweep.  The warped sweep
// already pays, per voxel, for everything colour needs — the warp, the projection, the texel —, so colour rides on it; a pass
// of its own would search (or read the field) a second time.
//
// The kernels are the two north-star sweeps of tsdf_warped.hip — searching, and served from the k-NN field — over the body
// of warped_color_device.hpp (the colour rule is stated there), each with and without the TSDF half (TSDF false: colours
// only — frame 0's volume is a copy, only its colours are missing).  Bricks, the support pre-pass, the grids of the launches
// and every refusal are those of the plain sweeps.  Vector stores only, no fast-math.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "knn_field_device.hpp"
#include "warped_color_device.hpp"

namespace dfa {

template <int K, bool GRID, bool TSDF>
__global__ __launch_bounds__(256) void integrate_warped6_color_kernel(const IntegrateArgs a, const ColorArgs c, const Warped6Frames f,
                                                                      const float* __restrict__ node_pos,
                                                                      const float* __restrict__ node_dq,
                                                                      const float* __restrict__ node_w, int D, int k, int rigid,
                                                                      const uint8_t* __restrict__ bricks, KnnGridView grid) {
    const bool marked = brick_marked(bricks);
    if (!marked && !rigid) return;
    SearchedNeighbours<K, GRID> nb{marked, node_pos, D, grid};
    const NorthStarWarp warp{f.vol2node, f.has_vol2node, f.node2cam, f.has_node2cam};
    warped_color_brick<K, TSDF>(a, c, rigid, nb, warp, k, node_pos, node_dq, node_w);
}

template <int K, bool TSDF>
__global__ __launch_bounds__(256) void integrate_warped6_color_field_kernel(const IntegrateArgs a, const ColorArgs c, const FieldGeom g,
                                                                            const Aff3 node2cam, int has_node2cam,
                                                                            const float* __restrict__ node_pos,
                                                                            const float* __restrict__ node_dq,
                                                                            const float* __restrict__ node_w, int rigid,
                                                                            const int32_t* __restrict__ table,
                                                                            const int32_t* __restrict__ coords,
                                                                            const int32_t* __restrict__ ids) {
    StoredNeighbours<K> nb(field_brick(g, table, coords, !rigid), ids, g.k);
    const NorthStarWarp warp{g.vol2node, g.has_frame, node2cam, has_node2cam};
    warped_color_brick<K, TSDF>(a, c, rigid, nb, warp, g.k, node_pos, node_dq, node_w);
}

// a statement that names TT, true when the volume is given
#define TSDF_DISPATCH(vol, ...)          \
    do {                                 \
        if (vol) {                       \
            constexpr bool TT = true;    \
            __VA_ARGS__;                 \
        } else {                         \
            constexpr bool TT = false;   \
            __VA_ARGS__;                 \
        }                                \
    } while (0)

hipError_t launch_tsdf_integrate_warped6_color(const uint16_t* dists, int dists_step, int cols, int rows, const ColorArgs& color,
                                               uint32_t* vol, int X, int Y, int Z, uint8_t* occ, const float voxel_size[3],
                                               float trunc_dist, int max_weight, const float* vol2node, const float* node2cam,
                                               const float node2vol[12], float stretch, float tmax, float fx, float fy, float cx,
                                               float cy, const float* node_pos, const float* node_dq, const float* node_w, int D,
                                               int k, bool rigid, const KnnGridView* grid, uint8_t* bricks, float* wmax,
                                               hipStream_t s) {
    const IntegrateArgs a = warped_args(dists, dists_step, cols, rows, vol, X, Y, Z, vol ? occ : nullptr, voxel_size, trunc_dist,
                                        max_weight, nullptr, fx, fy, cx, cy);  // (vol2cam is not read: the frames are in f)
    const Warped6Frames f{aff3_from(vol2node), aff3_from(node2cam), vol2node ? 1 : 0, node2cam ? 1 : 0};
    const hipError_t e = launch_warped6_mark_bricks(node_pos, node_w, D, vol2node != nullptr, node2vol, stretch, tmax, X, Y, Z,
                                                    voxel_size, bricks, wmax, s);
    if (e != hipSuccess) return e;
    const dim3 block(WBX, WBY), g3 = brick_grid(X, Y, Z);
    const KnnGridView gv = grid ? *grid : KnnGridView{};
    const int r = rigid ? 1 : 0;
    if (grid) TSDF_DISPATCH(vol, KDISPATCH8(k, integrate_warped6_color_kernel<KK, true, TT><<<g3, block, 0, s>>>(a, color, f, node_pos, node_dq, node_w, D, k, r, bricks, gv)));
    else TSDF_DISPATCH(vol, KDISPATCH8(k, integrate_warped6_color_kernel<KK, false, TT><<<g3, block, 0, s>>>(a, color, f, node_pos, node_dq, node_w, D, k, r, bricks, gv)));
    return hipGetLastError();
}

hipError_t launch_tsdf_integrate_warped6_color_field(const uint16_t* dists, int dists_step, int cols, int rows, const ColorArgs& color,
                                                     uint32_t* vol, uint8_t* occ, float trunc_dist, int max_weight,
                                                     const float* node2cam, float fx, float fy, float cx, float cy,
                                                     const float* node_pos, const float* node_dq, const float* node_w, bool rigid,
                                                     const KnnFieldView& f, size_t records, hipStream_t s) {
    if (!rigid && records == 0) return hipSuccess;
    const IntegrateArgs a = warped_args(dists, dists_step, cols, rows, vol, f.X, f.Y, f.Z, vol ? occ : nullptr, f.vs, trunc_dist,
                                        max_weight, nullptr, fx, fy, cx, cy);  // (vol2cam is not read: the field's frame and node2cam)
    const FieldGeom g = field_geom(f);
    const dim3 block(WBX, WBY), g3 = field_sweep_grid(f, rigid, records);
    TSDF_DISPATCH(vol, KDISPATCH8(f.k, integrate_warped6_color_field_kernel<KK, TT><<<g3, block, 0, s>>>(
                                           a, color, g, aff3_from(node2cam), node2cam ? 1 : 0, node_pos, node_dq, node_w, rigid ? 1 : 0,
                                           f.table, f.coords, f.ids)));
    return hipGetLastError();
}

}  // namespace dfa
