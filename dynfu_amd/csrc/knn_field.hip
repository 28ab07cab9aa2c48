// knn_field.hip — the k-NN field of a TSDF volume on gfx950: the neighbour lists of the volume's voxels searched ONCE and kept
// beside the volume: its stored set, its rows (search, merge) and their lookup.  The two warped sweeps that read the rows where
// they would search are in tsdf_warped.hip with the searching ones (one body: warped_sweep_device.hpp); what they and the
// kernels here share — the voxel's position, the field as a kernel takes it, the row read — is knn_field_device.hpp.
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

#include "device_math.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"
#include "knn_field_device.hpp"
#include "warped_mark_device.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------ the stored set
// One wave per node of [first, D): the bricks whose box comes within the node's OWN radius — the marking radii of the sweeps'
// pre-pass (warped_mark_device.hpp: mark_radius without a frame, mark_radius_framed with the node taken back to the volume by
// node2vol) with w_m where they have w_max.  A NaN radius ends as every brick (mark_bricks_near), which is a superset still.
__global__ __launch_bounds__(64) void field_mark_kernel(const float* __restrict__ node_pos, const float* __restrict__ node_w,
                                                        int first, int D, const Aff3 node2vol, int has_frame, float stretch,
                                                        float tmax, int X, int Y, int Z, float vsx, float vsy, float vsz,
                                                        uint8_t* __restrict__ bricks) {
    const int node = first + (int)blockIdx.x;
    if (node >= D) return;
    const f3 gn     = mk3(node_pos[3 * (size_t)node], node_pos[3 * (size_t)node + 1], node_pos[3 * (size_t)node + 2]);
    const float w   = node_w[node];
    const float ext = volume_extent(X, Y, Z, vsx, vsy, vsz);
    if (!has_frame) {
        const float g[3] = {gn.x, gn.y, gn.z};
        mark_bricks_near(g, mark_radius(w, gn, ext), X, Y, Z, vsx, vsy, vsz, bricks);
    } else {
        const f3 gv      = mulR(node2vol, gn) + mk3(node2vol.t[0], node2vol.t[1], node2vol.t[2]);
        const float g[3] = {gv.x, gv.y, gv.z};
        mark_bricks_near(g, mark_radius_framed(w, gn, gv, ext, stretch, tmax), X, Y, Z, vsx, vsy, vsz, bricks);
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
        int32_t* out = field_row(ids, rec, g.k, u);
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
    // the brick's slices inside the volume, counted as the sweeps count them (warped_sweep_device.hpp).  Not a matter of taste:
    // the compiler bounds the arguments of min() over ALL its calls in a unit, and without one call of this kind beside them
    // the clamps of knn_grid_query in field_search_kernel<K, true> compile to other, 2 % slower code
    // (profiles/warped_sweep_body.md; tools/kernel_isa_diff.py against the commit before shows it)
    const int nz = min(WBZ, g.Z - z0);
    for (int u = 0; u < WBZ && u < nz; ++u) {
        int32_t* row = field_row(ids, rec, g.k, u);
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

// ------------------------------------------------------------------------------------------ launchers
hipError_t launch_knn_field_count(const KnnFieldView& f, const float* node_pos, const float* node_w, int first, int D,
                                  uint8_t* marks, int32_t* offsets, int32_t* chunk_sums, int32_t* total, hipStream_t s) {
    const long n = (long)knn_field_bricks(f.X, f.Y, f.Z);
    hipError_t e = hipMemsetAsync(marks, 0, (size_t)n, s);
    if (e != hipSuccess) return e;
    if (D > first)
        field_mark_kernel<<<D - first, 64, 0, s>>>(node_pos, node_w, first, D, aff3_from(f.node2vol), f.has_frame, f.stretch, f.tmax,
                                                   f.X, f.Y, f.Z, f.vs[0], f.vs[1], f.vs[2], marks);
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
    if (records > 0 && D > D_old)
        KDISPATCH16(f.k, field_merge_kernel<KK><<<(unsigned)records, block, 0, s>>>(g, node_pos, D_old, D, f.coords, f.ids));
    if (fresh > 0) {
        field_assign_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(offsets, n, (int)records, f.table, f.coords);
        if (grid) KDISPATCH16(f.k, field_search_kernel<KK, true><<<(unsigned)fresh, block, 0, s>>>(g, node_pos, D, f.coords, (int)records, f.ids, gv));
        else KDISPATCH16(f.k, field_search_kernel<KK, false><<<(unsigned)fresh, block, 0, s>>>(g, node_pos, D, f.coords, (int)records, f.ids, gv));
    }
    return hipGetLastError();
}

hipError_t launch_knn_field_lookup(const KnnFieldView& f, const int32_t* voxels, int n, int32_t* out_idx, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    field_lookup_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(field_geom(f), f.table, f.ids, voxels, n, out_idx);
    return hipGetLastError();
}

}  // namespace dfa
