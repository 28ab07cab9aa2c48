// knn_field.hip — the k-NN field of a TSDF volume on gfx950: the neighbour lists of the volume's voxels searched ONCE and kept
// beside the volume, and the two warped sweeps of tsdf_warped.hip served from them without a search.
//
// The voxels of a volume never move and the nodes of a warp field only grow in number (Warpfield::update appends), so the
// search every voxel of every marked brick repeats every frame in dfa_tsdf_integrate_warped / _warped6 has the same answer
// until nodes are appended.  What dfa_warp_to_live_graph is to dfa_warp_to_live, this is to the warped sweeps.
//
// Layout.  Bricks are the sweeps' (warped_bricks.hpp: 64 x 4 x 1 voxels, one workgroup).  A brick is STORED when its box of
// voxel positions comes within a node's own radius of that node (the marking of the sweeps' pre-pass with w_m in place of
// w_max: a supported voxel has a node with |v - g_m| < w_m, so the stored bricks hold every supported voxel); each node marks
// on its own, which makes an append local.  A stored brick has a record of k slots x 256 ids, slot-major: the wave that owns
// a row of 64 voxels reads slot j as one 256-byte segment.  Rows are the first k ids of dfa_knn's contract at the voxel's
// search position — v = (x, y, z) * voxel_size, or c = R_n v + t_n with vol2node, by the sweeps' expressions —, ascending
// by (distance, index), -1 padded; voxels of a partial brick beyond the volume's edge hold -1.  Unsupported voxels of stored
// bricks keep their lists (an append needs them); support is not stored: the sweeps evaluate the rule as they always did.
//
// An append of nodes [D_old, D): bricks the new nodes reach and the table does not hold get records and a full search over all
// D nodes; every voxel stored before takes the top k, by (distance, index), of its list and the new nodes — exact, the order
// being total, with the distances recomputed by dist2 from the same float positions the search saw.  A build is an append to
// the empty field.
//
// No fused contraction beyond the fmaf()s of the shared headers, no fast-math; vector stores only.
#include <hip/hip_runtime.h>

#include "blend6_device.hpp"
#include "device_math.hpp"
#include "dq_device.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"
#include "tsdf_integrate_device.hpp"
#include "warped_mark_device.hpp"

namespace dfa {

namespace {

// the field as the kernels take it
struct FieldGeom {
    int X, Y, Z, k;
    int nbx, nby;  // bricks along x and y
    float vsx, vsy, vsz;
    int has_frame;
    Aff3 vol2node;
};

FieldGeom field_geom(const KnnFieldView& f) {
    FieldGeom g;
    g.X = f.X, g.Y = f.Y, g.Z = f.Z, g.k = f.k;
    g.nbx = (f.X + WBX - 1) / WBX, g.nby = (f.Y + WBY - 1) / WBY;
    g.vsx = f.vs[0], g.vsy = f.vs[1], g.vsz = f.vs[2];
    g.has_frame = f.has_frame;
    for (int i = 0; i < 12; ++i) (i < 9 ? g.vol2node.m[i] : g.vol2node.t[i - 9]) = f.has_frame ? f.vol2node[i] : (i % 4 == 0 && i < 9 ? 1.f : 0.f);
    return g;
}

// a voxel's search position: its corner by multiplication and, with a frame, c = R_n v + t_n — the expressions of
// integrate_warped_kernel / integrate_warped6_kernel, hence their bits
__device__ __forceinline__ f3 field_position(const FieldGeom& g, int x, int y, int z) {
    const f3 v = mk3((float)x * g.vsx, (float)y * g.vsy, (float)z * g.vsz);
    return g.has_frame ? mulR(g.vol2node, v) + mk3(g.vol2node.t[0], g.vol2node.t[1], g.vol2node.t[2]) : v;
}

// brick index of the table -> the brick's first voxel
__device__ __forceinline__ void brick_origin(const FieldGeom& g, int b, int& x0, int& y0, int& z0) {
    x0 = (b % g.nbx) * WBX, y0 = ((b / g.nbx) % g.nby) * WBY, z0 = (b / (g.nbx * g.nby)) * WBZ;
}

}  // namespace

// ------------------------------------------------------------------------------------------ the stored set
// One wave per node of [first, D): the bricks whose box comes within the node's OWN radius.  The widening terms are those of
// mark_bricks_kernel (no frame) and mark_bricks6_kernel (frame: the node taken back to the volume by node2vol), with w_m where
// they have w_max.  A NaN radius ends as every brick (mark_bricks_near), which is a superset still.
__global__ __launch_bounds__(64) void field_mark_kernel(const float* __restrict__ node_pos, const float* __restrict__ node_w,
                                                        int first, int D, const Aff3 node2vol, int has_frame, float stretch,
                                                        float tmax, int X, int Y, int Z, float vsx, float vsy, float vsz,
                                                        uint8_t* __restrict__ bricks) {
    const int node = first + (int)blockIdx.x;
    if (node >= D) return;
    const f3 gn     = mk3(node_pos[3 * (size_t)node], node_pos[3 * (size_t)node + 1], node_pos[3 * (size_t)node + 2]);
    const float w   = node_w[node];
    const float ext = fmaxf(fmaxf(fabsf(vsx) * (float)X, fabsf(vsy) * (float)Y), fabsf(vsz) * (float)Z);
    if (!has_frame) {
        const float g[3] = {gn.x, gn.y, gn.z};
        const float r    = w * 1.001f + 1e-6f * fmaxf(ext, fmaxf(fmaxf(fabsf(g[0]), fabsf(g[1])), fabsf(g[2])));
        mark_bricks_near(g, r, X, Y, Z, vsx, vsy, vsz, bricks);
    } else {
        const f3 gv      = mulR(node2vol, gn) + mk3(node2vol.t[0], node2vol.t[1], node2vol.t[2]);
        const float g[3] = {gv.x, gv.y, gv.z};
        const float L    = 2.f * ext + fmaxf(fmaxf(fabsf(gn.x), fabsf(gn.y)), fabsf(gn.z)) +
                        fmaxf(fmaxf(fabsf(gv.x), fabsf(gv.y)), fabsf(gv.z)) + tmax;
        const float r = w * 1.001f * stretch + 1e-6f * L;
        mark_bricks_near(g, r, X, Y, Z, vsx, vsy, vsz, bricks);
    }
}

// 1 for a marked brick the table does not hold yet
__global__ __launch_bounds__(256) void field_flag_kernel(const uint8_t* __restrict__ marks, const int32_t* __restrict__ table,
                                                         int32_t* __restrict__ flags, long n) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b < n) flags[b] = marks[b] != 0 && table[b] < 0 ? 1 : 0;
}

// behind the scan of the flags: new brick b becomes record base + offsets[b]
__global__ __launch_bounds__(256) void field_assign_kernel(const int32_t* __restrict__ offsets, long n, int base,
                                                           int32_t* __restrict__ table, int32_t* __restrict__ coords) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= n || offsets[b + 1] == offsets[b]) return;
    const int rec = base + offsets[b];
    table[b]      = rec;
    coords[rec]   = (int)b;
}

// ------------------------------------------------------------------------------------------ search and merge
// block = (64, 4): one workgroup per NEW record, one lane per voxel as in the sweeps; the search of the sweeps (GRID: the node
// grid, else a scan of all nodes).  Lanes beyond the volume's edge store -1.
template <int K, bool GRID>
__global__ __launch_bounds__(256) void field_search_kernel(const FieldGeom g, const float* __restrict__ node_pos, int D,
                                                           const int32_t* __restrict__ coords, int first,
                                                           int32_t* __restrict__ ids, KnnGridView grid) {
    const int rec = first + (int)blockIdx.x;
    int x0, y0, z0;
    brick_origin(g, coords[rec], x0, y0, z0);
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    KnnGridDesc gd{};
    if (GRID) gd = *grid.desc;
    for (int u = 0; u < WBZ; ++u) {
        KnnList<K> best;
        best.init();
        if (x < g.X && y < g.Y && z0 + u < g.Z) {
            const f3 q = field_position(g, x, y, z0 + u);
            if (GRID) {
                knn_grid_query<K>(gd, grid.cell_start, grid.sorted, q, best);
            } else {
                for (int j = 0; j < D; ++j) best.push(dist2(q, node_pos[3 * j], node_pos[3 * j + 1], node_pos[3 * j + 2]), j);
            }
        }
        int32_t* out = ids + (size_t)rec * g.k * WB_VOXELS + ((u * WBY + threadIdx.y) * WBX + threadIdx.x);
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < g.k) out[(size_t)j * WB_VOXELS] = best.index(j);
    }
}

// one workgroup per record stored BEFORE the append: every voxel's list with the nodes [D_old, D) merged in
template <int K>
__global__ __launch_bounds__(256) void field_merge_kernel(const FieldGeom g, const float* __restrict__ node_pos, int D_old, int D,
                                                          const int32_t* __restrict__ coords, int32_t* __restrict__ ids) {
    const int rec = (int)blockIdx.x;
    int x0, y0, z0;
    brick_origin(g, coords[rec], x0, y0, z0);
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= g.X || y >= g.Y) return;  // (beyond the edge: the row stays -1)
    for (int u = 0; u < WBZ && z0 + u < g.Z; ++u) {
        int32_t* row = ids + (size_t)rec * g.k * WB_VOXELS + ((u * WBY + threadIdx.y) * WBX + threadIdx.x);
        const f3 q   = field_position(g, x, y, z0 + u);
        int old[K];
#pragma unroll
        for (int j = 0; j < K; ++j) old[j] = j < g.k ? row[(size_t)j * WB_VOXELS] : -1;
        KnnList<K> best;
        best.init();
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int n = old[j] >= 0 ? old[j] : 0;  // (an absent neighbour reads node 0 and is not pushed)
            const float d = dist2(q, node_pos[3 * n], node_pos[3 * n + 1], node_pos[3 * n + 2]);
            if (old[j] >= 0) best.push(d, old[j]);
        }
        for (int j = D_old; j < D; ++j) best.push(dist2(q, node_pos[3 * j], node_pos[3 * j + 1], node_pos[3 * j + 2]), j);
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < g.k && best.index(j) != old[j]) row[(size_t)j * WB_VOXELS] = best.index(j);
    }
}

// one lane per queried voxel: its row, or -1 where the voxel lies outside the volume or in a brick not stored
__global__ __launch_bounds__(256) void field_lookup_kernel(const FieldGeom g, const int32_t* __restrict__ table,
                                                           const int32_t* __restrict__ ids, const int32_t* __restrict__ voxels,
                                                           int n, int32_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = voxels[3 * (size_t)i], y = voxels[3 * (size_t)i + 1], z = voxels[3 * (size_t)i + 2];
    int rec = -1;
    if (table && x >= 0 && y >= 0 && z >= 0 && x < g.X && y < g.Y && z < g.Z)  // (null: an empty field)
        rec = table[((size_t)(z / WBZ) * g.nby + y / WBY) * g.nbx + x / WBX];
    const int t = ((z % WBZ) * WBY + y % WBY) * WBX + x % WBX;
    for (int j = 0; j < g.k; ++j)
        out[(size_t)i * g.k + j] = rec >= 0 ? ids[((size_t)rec * g.k + j) * WB_VOXELS + t] : -1;
}

// ------------------------------------------------------------------------------------------ the sweeps from the field
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

// the voxel's stored row as the list the shared rules read (they read index(j) only)
template <int K>
__device__ __forceinline__ void field_list(const int32_t* __restrict__ row, int k, KnnList<K>& best) {
    int id[K];
#pragma unroll
    for (int j = 0; j < K; ++j) id[j] = j < k ? row[(size_t)j * WB_VOXELS] : -1;
#pragma unroll
    for (int j = 0; j < K; ++j) best.set_index(j, id[j]);
}

// integrate_warped_kernel with the search replaced by the stored row: the same support rule, blend, update, store rule and
// occupancy rule on the same values.  block = (64, 4), one brick per workgroup.
template <int K>
__global__ __launch_bounds__(256) void integrate_warped_field_kernel(const IntegrateArgs a, const FieldGeom g,
                                                                     const float* __restrict__ node_pos,
                                                                     const float* __restrict__ node_dq,
                                                                     const float* __restrict__ node_w, int rigid,
                                                                     const int32_t* __restrict__ table,
                                                                     const int32_t* __restrict__ coords,
                                                                     const int32_t* __restrict__ ids) {
    const FieldBrick b = field_brick(g, table, coords, !rigid);
    const bool stored  = b.rec >= 0;
    const int x = b.x0 + threadIdx.x, y = b.y0 + threadIdx.y, z0 = b.z0;
    if (x >= a.X || y >= a.Y) return;
    const int nz = min(WBZ, a.Z - z0);

    const size_t slice = (size_t)a.X * a.Y;
    uint32_t* ptr      = a.vol + (size_t)x + (size_t)a.X * y + slice * z0;
    uint32_t cur[WBZ];
#pragma unroll
    for (int u = 0; u < WBZ; ++u) cur[u] = u < nz ? ptr[slice * u] : 0u;

    const f3 t = mk3(a.vol2cam.t[0], a.vol2cam.t[1], a.vol2cam.t[2]);
    bool any   = false;  // an update happened: the voxel may hold a weight now
    for (int u = 0; u < nz; ++u) {
        const f3 v = mk3((float)x * a.vsx, (float)y * a.vsy, (float)(z0 + u) * a.vsz);
        f3 p       = v;
        bool go    = rigid != 0;
        if (stored) {
            KnnList<K> best;
            field_list<K>(ids + (size_t)b.rec * g.k * WB_VOXELS + ((u * WBY + threadIdx.y) * WBX + threadIdx.x), g.k, best);
            if (support_min<K>(best, g.k, node_pos, node_w, v) < 1.f) {
                p  = dq_transform(calc_dqb<K>(best, g.k, node_pos, node_dq, node_w, v), v);
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
        // as integrate_warped_kernel: lanes 0 and 32 write the occupancy box of their half of the row when it updated a voxel
        const unsigned long long m = __ballot(any);
        if ((threadIdx.x & 31) == 0 && ((m >> threadIdx.x) & 0xffffffffull) != 0ull)
            a.occ[(size_t)(x / 32) + (size_t)a.ox * ((size_t)(y / 2) + (size_t)a.oy * (size_t)(z0 / 8))] = 3;
    }
}

// integrate_warped6_kernel likewise.  The field's frame is the call's vol2node (the C ABI compares the 12 floats).
template <int K>
__global__ __launch_bounds__(256) void integrate_warped6_field_kernel(const IntegrateArgs a, const FieldGeom g, const Aff3 node2cam,
                                                                      int has_node2cam, const float* __restrict__ node_pos,
                                                                      const float* __restrict__ node_dq,
                                                                      const float* __restrict__ node_w, int rigid,
                                                                      const int32_t* __restrict__ table,
                                                                      const int32_t* __restrict__ coords,
                                                                      const int32_t* __restrict__ ids) {
    const FieldBrick b = field_brick(g, table, coords, !rigid);
    const bool stored  = b.rec >= 0;
    const int x = b.x0 + threadIdx.x, y = b.y0 + threadIdx.y, z0 = b.z0;
    if (x >= a.X || y >= a.Y) return;
    const int nz = min(WBZ, a.Z - z0);

    const size_t slice = (size_t)a.X * a.Y;
    uint32_t* ptr      = a.vol + (size_t)x + (size_t)a.X * y + slice * z0;
    uint32_t cur[WBZ];
#pragma unroll
    for (int u = 0; u < WBZ; ++u) cur[u] = u < nz ? ptr[slice * u] : 0u;

    const int k = g.k;
    bool any    = false;  // an update happened: the voxel may hold a weight now
    for (int u = 0; u < nz; ++u) {
        const f3 c = field_position(g, x, y, z0 + u);  // (uniform) the voxel in the node frame
        f3 p       = c;
        bool go    = rigid != 0;
        if (stored) {
            KnnList<K> best;
            field_list<K>(ids + (size_t)b.rec * g.k * WB_VOXELS + ((u * WBY + threadIdx.y) * WBX + threadIdx.x), g.k, best);
            if (support_min<K>(best, k, node_pos, node_w, c) < 1.f) {
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
        const f3 vc = has_node2cam ? mulR(node2cam, p) + mk3(node2cam.t[0], node2cam.t[1], node2cam.t[2]) : p;
        float tsdf;
        if (!voxel_tsdf(a, vc, tsdf)) continue;
        const uint32_t upd = voxel_update<false>(a, cur[u], tsdf);
        if (upd != cur[u]) ptr[slice * u] = upd;
        any = true;
    }
    if (a.occ) {
        const unsigned long long m = __ballot(any);
        if ((threadIdx.x & 31) == 0 && ((m >> threadIdx.x) & 0xffffffffull) != 0ull)
            a.occ[(size_t)(x / 32) + (size_t)a.ox * ((size_t)(y / 2) + (size_t)a.oy * (size_t)(z0 / 8))] = 3;
    }
}

// ------------------------------------------------------------------------------------------ launchers
hipError_t launch_knn_field_count(const KnnFieldView& f, const float* node_pos, const float* node_w, int first, int D,
                                  uint8_t* marks, int32_t* offsets, int32_t* chunk_sums, int32_t* total, hipStream_t s) {
    const long n = (long)knn_field_bricks(f.X, f.Y, f.Z);
    hipError_t e = hipMemsetAsync(marks, 0, (size_t)n, s);
    if (e != hipSuccess) return e;
    if (D > first) {
        Aff3 back;
        for (int i = 0; i < 12; ++i) (i < 9 ? back.m[i] : back.t[i - 9]) = f.node2vol[i];
        field_mark_kernel<<<D - first, 64, 0, s>>>(node_pos, node_w, first, D, back, f.has_frame, f.stretch, f.tmax, f.X, f.Y, f.Z,
                                                   f.vs[0], f.vs[1], f.vs[2], marks);
    }
    field_flag_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(marks, f.table, offsets, n);
    launch_segment_scan(offsets, n, chunk_sums, total, s);
    return hipGetLastError();
}

hipError_t launch_knn_field_extend(const KnnFieldView& f, const float* node_pos, int D_old, int D, size_t records, size_t fresh,
                                   const int32_t* offsets, const KnnGridView* grid, hipStream_t s) {
    const FieldGeom g = field_geom(f);
    const long n      = (long)knn_field_bricks(f.X, f.Y, f.Z);
    const dim3 block(WBX, WBY);
    const KnnGridView gv = grid ? *grid : KnnGridView{};
    // the records stored before first: their merge reads coords and ids of [0, records) only
#define FIELD_K(CALL)        \
    do {                     \
        if (f.k <= 4) CALL(4);      \
        else if (f.k <= 8) CALL(8); \
        else CALL(16);              \
    } while (0)
#define MERGE(KK) field_merge_kernel<KK><<<(unsigned)records, block, 0, s>>>(g, node_pos, D_old, D, f.coords, f.ids)
    if (records > 0 && D > D_old) FIELD_K(MERGE);
#undef MERGE
    if (fresh > 0) {
        field_assign_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(offsets, n, (int)records, f.table, f.coords);
#define SEARCH(KK)                                                                                                              \
    do {                                                                                                                        \
        if (grid) field_search_kernel<KK, true><<<(unsigned)fresh, block, 0, s>>>(g, node_pos, D, f.coords, (int)records, f.ids, gv);  \
        else field_search_kernel<KK, false><<<(unsigned)fresh, block, 0, s>>>(g, node_pos, D, f.coords, (int)records, f.ids, gv);      \
    } while (0)
        FIELD_K(SEARCH);
#undef SEARCH
    }
    return hipGetLastError();
}

hipError_t launch_knn_field_lookup(const KnnFieldView& f, const int32_t* voxels, int n, int32_t* out_idx, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    field_lookup_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(field_geom(f), f.table, f.ids, voxels, n, out_idx);
    return hipGetLastError();
}

namespace {
IntegrateArgs field_integrate_args(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol, uint8_t* occ,
                                   float trunc_dist, int max_weight, const float* vol2cam, float fx, float fy, float cx, float cy,
                                   const KnnFieldView& f) {
    IntegrateArgs a;
    a.dists = dists, a.dists_step = dists_step, a.cols = cols, a.rows = rows;
    a.vol = vol, a.X = f.X, a.Y = f.Y, a.Z = f.Z;
    const OccDims od = occ_dims(f.X, f.Y, f.Z);
    a.occ = occ, a.ox = od.ox, a.oy = od.oy, a.occ_known = 0;
    a.vsx = f.vs[0], a.vsy = f.vs[1], a.vsz = f.vs[2];
    a.trunc      = trunc_dist;
    a.trunc_inv  = 1.f / trunc_dist;  // tsdf_volume.cu:106
    a.max_weight = max_weight;
    a.vol2cam    = Aff3{{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};
    if (vol2cam)
        for (int i = 0; i < 12; ++i) (i < 9 ? a.vol2cam.m[i] : a.vol2cam.t[i - 9]) = vol2cam[i];
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.zchunk = WBZ;
    return a;
}
}  // namespace

// SKIP: one workgroup per stored brick (none: nothing to do).  RIGID: every brick.
hipError_t launch_tsdf_integrate_warped_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol,
                                              uint8_t* occ, float trunc_dist, int max_weight, const float vol2cam[12], float fx,
                                              float fy, float cx, float cy, const float* node_pos, const float* node_dq,
                                              const float* node_w, bool rigid, const KnnFieldView& f, size_t records,
                                              hipStream_t s) {
    if (!rigid && records == 0) return hipSuccess;
    const IntegrateArgs a = field_integrate_args(dists, dists_step, cols, rows, vol, occ, trunc_dist, max_weight, vol2cam, fx, fy,
                                                 cx, cy, f);
    const FieldGeom g = field_geom(f);
    const dim3 block(WBX, WBY);
    const dim3 g3 = rigid ? dim3(g.nbx, g.nby, (f.Z + WBZ - 1) / WBZ) : dim3((unsigned)records);
#define WARPED(KK) \
    integrate_warped_field_kernel<KK><<<g3, block, 0, s>>>(a, g, node_pos, node_dq, node_w, rigid ? 1 : 0, f.table, f.coords, f.ids)
    if (f.k <= 4) WARPED(4);
    else if (f.k <= 8) WARPED(8);
    else WARPED(16);
#undef WARPED
    return hipGetLastError();
}

hipError_t launch_tsdf_integrate_warped6_field(const uint16_t* dists, int dists_step, int cols, int rows, uint32_t* vol,
                                               uint8_t* occ, float trunc_dist, int max_weight, const float* node2cam, float fx,
                                               float fy, float cx, float cy, const float* node_pos, const float* node_dq,
                                               const float* node_w, bool rigid, const KnnFieldView& f, size_t records,
                                               hipStream_t s) {
    if (!rigid && records == 0) return hipSuccess;
    const IntegrateArgs a = field_integrate_args(dists, dists_step, cols, rows, vol, occ, trunc_dist, max_weight, nullptr, fx, fy,
                                                 cx, cy, f);  // (vol2cam is not read: the frames are the field's and node2cam)
    const FieldGeom g = field_geom(f);
    Aff3 n2c          = a.vol2cam;
    if (node2cam)
        for (int i = 0; i < 12; ++i) (i < 9 ? n2c.m[i] : n2c.t[i - 9]) = node2cam[i];
    const dim3 block(WBX, WBY);
    const dim3 g3 = rigid ? dim3(g.nbx, g.nby, (f.Z + WBZ - 1) / WBZ) : dim3((unsigned)records);
#define WARPED6(KK)                                                                                                              \
    integrate_warped6_field_kernel<KK><<<g3, block, 0, s>>>(a, g, n2c, node2cam ? 1 : 0, node_pos, node_dq, node_w, rigid ? 1 : 0, \
                                                            f.table, f.coords, f.ids)
    if (f.k <= 4) WARPED6(4);  // (k is 1..8 here)
    else WARPED6(8);
#undef WARPED6
    return hipGetLastError();
}

}  // namespace dfa
