// knn_device.hpp — device side of the exact k-NN searches of the deformation nodes, shared by the kernels of knn.hip, warp.hip
// and correspond.hip, the fused graph-build kernel of solve_graph.hip, the regularisation hierarchy, the k-NN field and the warped
// sweeps: the sorted candidate list, the distance expression, the exhaustive scan (knn_scan), the one-lane-per-query grid search
// (knn_grid_query) and the one-wave-per-query search (knn_wave_search).
//
// Reference semantics: src/dynfu/warp_field.cpp:99-171 (nanoflann KD-tree k-NN per vertex on
// the CPU, three std::vector allocations per query) and src/dynfu/utils/node.cpp:29-36.
//
// MI355X design.  The result contract is "the k nodes with the smallest (squared distance,
// node index) pairs, ascending" — what nanoflann returns up to the order of exact ties.  Two
// exact searches produce it:
//   * brute force (small problems): one lane per query, node positions staged through LDS in
//     1024-node tiles (a wave reads one node per step -> LDS broadcast), the k best kept in
//     registers as a sorted list updated by an unrolled compare-exchange chain;
//   * uniform grid (n_query * D large): nodes are bucketed by a counting sort into at most 32^3
//     cells sized ~2 node spacings (the grid geometry is computed ON the device from the node
//     bounding box, no host round trip); a query walks Chebyshev shells of cells around its own
//     cell and stops once its k-th distance is below the distance to the next shell.  At
//     262 k vertices x 2 k nodes that is ~50 candidates per query instead of 2048.
// Both use the same distance expression (nanoflann L2_Simple_Adaptor order of operations) so
// the neighbour lists are bit-identical to the CPU oracle's.
// The solver plan's graph build runs both of its searches inside one launch of its own (solve_graph.hip: graph_rows_kernel);
// launch_knn (knn.hip) serves everyone else (dfa_knn, the host adaptor, plans whose nodes are not in the grid).  What a point
// does with its list — the blend and the support rule — is in dqb_device.hpp.  The grid itself is built in knn_grid.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_switch.hpp"
#include "device_math.hpp"
#include "dq_device.hpp"
#include "kernels.hpp"
#include "knn_walk.hpp"

namespace dfa {

// sorted (ascending by (distance, index)) list of the K nearest candidates.  An entry is ONE 64-bit key — the bits of the
// (non-negative) squared distance above the node index — so that "(d, i) before (d', i')" is one unsigned compare and an
// exchange is a min / max pair: the 8-NN search of 1.08 M vertices is bound by vector-ALU issue, and the insertion is most of
// what it issues (profiles/r05_sq_hostseq_ref.md).  The order of non-negative floats is the order of their bits; +inf
// (empty) sorts behind every finite distance, a NaN distance (a vertex with NaN coordinates) behind +inf: never inserted.
template <int K>
struct KnnList {
    unsigned long long key[K];
    static constexpr unsigned long long EMPTY = 0x7f8000007fffffffull;  // (+inf, index 0x7fffffff)
    __device__ __forceinline__ static unsigned long long pack(float dist, int idx) {
        return ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned int)idx;
    }
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < K; ++j) key[j] = EMPTY;
    }
    __device__ __forceinline__ void push(float dist, int idx) {
        const unsigned long long x = pack(dist, idx);
        if (x < key[K - 1]) {
            key[K - 1] = x;
#pragma unroll
            for (int j = K - 1; j > 0; --j) {
                const unsigned long long a = key[j - 1], b = key[j];
                key[j - 1] = a < b ? a : b, key[j] = a < b ? b : a;
            }
        }
    }
    __device__ __forceinline__ float dist(int j) const { return __uint_as_float((unsigned int)(key[j] >> 32)); }
    __device__ __forceinline__ int raw_index(int j) const { return (int)(unsigned int)key[j]; }  // 0x7fffffff: empty
    __device__ __forceinline__ int index(int j) const { return raw_index(j) == 0x7fffffff ? -1 : raw_index(j); }
    __device__ __forceinline__ void set_index(int j, int n) { key[j] = pack(__builtin_inff(), n < 0 ? 0x7fffffff : n); }
};

// L2_Simple_Adaptor::evalMetric (nanoflann.hpp:338-345): ((0 + d0^2) + d1^2) + d2^2
__device__ __forceinline__ float dist2(f3 q, float gx, float gy, float gz) {
    const float d0 = q.x - gx, d1 = q.y - gy, d2 = q.z - gz;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// ---------------------------------------------------------------------------- brute force
constexpr int KNN_TILE = 1024;
// scans all D nodes (block-cooperative LDS staging); every thread of the block must call it
template <int K>
__device__ __forceinline__ void knn_scan(const float* __restrict__ node_pos, int D, f3 q, KnnList<K>& best,
                                         float4* tile) {
    best.init();
    for (int base = 0; base < D; base += KNN_TILE) {
        const int n = min(KNN_TILE, D - base);
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            const float* p = node_pos + 3 * (size_t)(base + j);
            tile[j]        = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 g = tile[j];
            best.push(dist2(q, g.x, g.y, g.z), base + j);
        }
    }
}

// a kernel<K, GRID> by the bucket of k (4, 8, 16) and the search: the grid's or the exhaustive scan (launch_knn, launch_warp_to_live)
#define KGDISPATCH(kernel, k, use_grid, ...)                         \
    do {                                                             \
        if (use_grid) {                                              \
            if ((k) <= 4) kernel<4, true> __VA_ARGS__;               \
            else if ((k) <= 8) kernel<8, true> __VA_ARGS__;          \
            else kernel<16, true> __VA_ARGS__;                       \
        } else {                                                     \
            if ((k) <= 4) kernel<4, false> __VA_ARGS__;              \
            else if ((k) <= 8) kernel<8, false> __VA_ARGS__;         \
            else kernel<16, false> __VA_ARGS__;                      \
        }                                                            \
    } while (0)

// the first k entries of a query's list as node ids and RBF weights (Warpfield::getWeightsAndNearestNeighbours,
// warp_field.cpp:99-125); -1 / 0 for an absent neighbour and for the slots from k on
template <int K>
__device__ __forceinline__ void knn_ids_weights(const KnnList<K>& best, int k, const float* __restrict__ node_pos,
                                                const float* __restrict__ node_w, bool with_weights, f3 q,
                                                int (&out_i)[K], float (&out_w)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        out_i[j] = -1, out_w[j] = 0.f;
        if (j < k) {
            const int n = best.index(j);
            out_i[j]    = n;
            if (with_weights && n >= 0)
                out_w[j] = transformation_weight(mk3(node_pos[3 * n], node_pos[3 * n + 1], node_pos[3 * n + 2]), node_w[n], q);
        }
    }
}

__device__ __forceinline__ void cell_of(const KnnGridDesc& g, f3 p, int& cx, int& cy, int& cz) {
    // clamped: queries outside the node bounding box are projected onto it (the projection is
    // never farther from any node than the query itself, so shell bounds stay valid)
    cx = min(max((int)floorf((p.x - g.bmin[0]) * g.inv_cs), 0), g.dim[0] - 1);
    cy = min(max((int)floorf((p.y - g.bmin[1]) * g.inv_cs), 0), g.dim[1] - 1);
    cz = min(max((int)floorf((p.z - g.bmin[2]) * g.inv_cs), 0), g.dim[2] - 1);
}

// exact k-NN through the grid: Chebyshev shells r = 0, 1, 2, ... around the query's cell
// TIGHT: the stop bound also counts the query's distance to the nearest wall of its own cell (the
// visited block of cells extends r cells beyond that wall), which lets a 1-NN search stop inside
// shell 0 / 1 of a fine grid.  Same result either way — the bound only decides when to stop.
// ONE_LOOP: the nine rows of the 3 x 3 x 3 block in one candidate loop per lane (knn_walk.hpp) instead of nine wave-wide
// loops.  `count` is the length of the sorted array, `walk` the lane's own column of KNN_WALK_ROWS slots in LDS, KNN_WALK_STRIDE
// entries apart (the kernel declares KnnWalkSlots<true> and passes slots.of_lane()).  The same candidates, hence — the list
// keeps the K smallest of unique keys, in whatever order they are pushed — the same list.
constexpr int KNN_WALK_STRIDE = 256;  // threads of a workgroup of every kernel that walks
inline bool knn_one_loop() { return dev_env_int("DFA_KNN_ONE_LOOP", 1) != 0; }  // (development builds: 0 keeps the nine loops)
template <bool ONE_LOOP>
struct KnnWalkSlots {
    int2 slot[ONE_LOOP ? KNN_WALK_ROWS * KNN_WALK_STRIDE : 1];
    __device__ __forceinline__ int2* of_lane() { return ONE_LOOP ? slot + threadIdx.x : nullptr; }  // block = (256)
};

template <int K, bool TIGHT = false, bool ONE_LOOP = false>
__device__ __forceinline__ void knn_grid_query(const KnnGridDesc& g, const int32_t* __restrict__ cell_start,
                                               const float4* __restrict__ sorted, f3 q, KnnList<K>& best, bool rescan = false,
                                               int count = 0, int2* walk = nullptr) {
    static_assert(!(TIGHT && ONE_LOOP), "the tight search keeps its own loops");
    // TIGHT scans the query's own cell twice (alone, then inside the 3 x 3 x 3 block): harmless for K = 1, where a repeated
    // candidate cannot displace anything, but a K > 1 list would hold the same node twice
    static_assert(!TIGHT || K == 1, "the tight stop bound re-scans the own cell: 1-NN only");
    best.init();
    int cx, cy, cz;
    cell_of(g, q, cx, cy, cz);
    float margin = 0.f;  // in cells; 0 for queries outside the grid (clamped above)
    float wall[3][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};  // TIGHT: distance to the low / high wall of the own cell per axis (m)
    bool inside      = false;
    if (TIGHT) {
        const float ux = (q.x - g.bmin[0]) * g.inv_cs - (float)cx, uy = (q.y - g.bmin[1]) * g.inv_cs - (float)cy,
                    uz = (q.z - g.bmin[2]) * g.inv_cs - (float)cz;
        const float m = fminf(fminf(fminf(ux, 1.f - ux), fminf(uy, 1.f - uy)), fminf(uz, 1.f - uz));
        margin        = m > 0.f ? m : 0.f;  // negative (outside) or NaN -> 0
        inside        = m >= 0.f;           // (false for NaN)
        const float u[3] = {ux, uy, uz};
        // (1e-3 cells off every wall: the rounding of the cell assignment, as in the stop bounds below)
#pragma unroll
        for (int c = 0; c < 3; ++c) wall[c][0] = fmaxf(u[c] - 1e-3f, 0.f) * g.cs, wall[c][1] = fmaxf(1.f - u[c] - 1e-3f, 0.f) * g.cs;
    }
    const int rmax = max(g.dim[0], max(g.dim[1], g.dim[2]));
    int r_first    = 0;
    // candidates [beg, end) of the sorted node array, four at a time from clamped indices
    auto scan_range = [&](int beg, int end) __attribute__((always_inline)) {
        constexpr int KNN_BATCH = 4;  // (8: the same 48 us at C2, 16: 64; one by one: 54)
        for (int j = beg; j < end; j += KNN_BATCH) {
            float4 n[KNN_BATCH];
#pragma unroll
            for (int t = 0; t < KNN_BATCH; ++t) n[t] = sorted[min(j + t, end - 1)];
#pragma unroll
            for (int t = 0; t < KNN_BATCH; ++t)
                if (j + t < end) best.push(dist2(q, n[t].x, n[t].y, n[t].z), __float_as_int(n[t].w));
        }
    };
    // the 3 x 3 x 3 block around the query's cell as nine x-rows of cells (the cells of an x-row are consecutive in the sorted
    // node array): the rows' ranges requested together — unconditional loads from clamped cells, a row outside the grid is
    // empty —, then every row's candidates
    auto block3_rows = [&](int (&rbeg)[9], int (&rend)[9]) __attribute__((always_inline)) {
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const int z = cz - 1 + i / 3, y = cy - 1 + i % 3;
            const bool in = z >= 0 && z < g.dim[2] && y >= 0 && y < g.dim[1];
            const int c   = in ? g.dim[0] * (y + g.dim[1] * z) : 0;
            const int b = cell_start[c + x0], e = cell_start[c + x1 + 1];
            rbeg[i] = in ? b : 0, rend[i] = in ? e : 0;
        }
    };
    auto scan_block3 = [&]() __attribute__((always_inline)) {
        int rbeg[9], rend[9];
        block3_rows(rbeg, rend);
        // (the row of the query's own cell first, then the four rows that share a face with it, then the corners: the list
        // fills with near candidates early, and a late candidate that no lane of the wave accepts skips the insertion)
        constexpr int order[9] = {4, 1, 3, 5, 7, 0, 2, 6, 8};
#pragma unroll
        for (int i = 0; i < 9; ++i) scan_range(rbeg[order[i]], rend[order[i]]);
    };
    // the same nine rows in the same order as ONE loop: every lane walks its own ranges, a batch of four inside one range at a
    // time, and the wave leaves when its last lane has finished.  A lane's trip count is fixed before the loop from the
    // eighteen table words, the ranges clamped to the array (knn_walk_plan): a damaged table can neither keep a wave here
    // nor send a load outside `sorted`.  The ranges wait in the lane's LDS column, where a computed slot is an address.
    auto walk_block3 = [&]() __attribute__((always_inline)) {
        int rbeg[9], rend[9];
        block3_rows(rbeg, rend);
        const int steps = knn_walk_plan(rbeg, rend, count, [&](int slot, int b, int e) { walk[slot * KNN_WALK_STRIDE] = make_int2(b, e); });
        const int cap   = KNN_WALK_ROWS * ((count + KNN_WALK_BATCH - 1) / KNN_WALK_BATCH);  // (uniform; steps <= cap)
        KnnWalk w;
        knn_walk_begin(w);
        for (int s = 0; s < cap && __any(s < steps); ++s) {
            if (s < steps) {
                int j, end;
                knn_walk_step(w, [&](int slot, int& b, int& e) { const int2 r = walk[slot * KNN_WALK_STRIDE]; b = r.x, e = r.y; }, j, end);
                float4 n[KNN_WALK_BATCH];
#pragma unroll
                for (int t = 0; t < KNN_WALK_BATCH; ++t) n[t] = sorted[min(j + t, end - 1)];
#pragma unroll
                for (int t = 0; t < KNN_WALK_BATCH; ++t)
                    if (j + t < end) best.push(dist2(q, n[t].x, n[t].y, n[t].z), __float_as_int(n[t].w));
            }
        }
    };
    if (TIGHT) {
        // shell 0 (the query's own cell) — a 1-NN search on a fine grid usually ends here —, then, if it does not, shells 0
        // and 1 together as the nine rows (the own cell's candidates a second time: a set, the order and repeats do not
        // matter), each followed by the stop rule of its shell; further shells in the loop below
        const int c0 = cx + g.dim[0] * (cy + g.dim[1] * cz);
        scan_range(cell_start[c0], cell_start[c0 + 1]);
        const float b0 = fmaxf(margin - 1e-3f, 0.f) * g.cs;
        if (best.dist(K - 1) < b0 * b0 * 0.9999f) return;
        // Shell 1, without the cells that cannot hold anything nearer than what the own cell gave (d0): a query that fails
        // the test above sits near ONE wall or edge of its cell, and of the 26 neighbours only the few across that wall are
        // within d0 — a cell whose nearest point is farther than d0 is skipped by the rule that ends the search (strictly
        // farther, with the same margins), so the result, ties included, is that of the full block.  The own cell is not
        // scanned again unless both x neighbours of its row are.  On a million-point surface (~20 points per cell at the
        // 256-cell cap) the full block is ~180 candidates; this is the part of it across the near walls.
        {
            const float d0 = best.dist(K - 1);
            int rbeg[9], rend[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const int dz = i / 3 - 1, dy = i % 3 - 1, z = cz + dz, y = cy + dy;
                const float ey = dy < 0 ? wall[1][0] : dy > 0 ? wall[1][1] : 0.f, ez = dz < 0 ? wall[2][0] : dz > 0 ? wall[2][1] : 0.f;
                const float rb2 = ey * ey + ez * ez;
                const bool keep = !inside || !(d0 < rb2 * 0.9999f);
                const bool xl   = keep && (!inside || !(d0 < (rb2 + wall[0][0] * wall[0][0]) * 0.9999f));
                const bool xr   = keep && (!inside || !(d0 < (rb2 + wall[0][1] * wall[0][1]) * 0.9999f));
                const bool own  = dy == 0 && dz == 0;  // the row of the own cell: that cell is done
                const bool mid  = keep && (!own || (xl && xr));
                const bool in   = z >= 0 && z < g.dim[2] && y >= 0 && y < g.dim[1] && (xl || xr || mid);
                const int x0 = max(xl ? cx - 1 : (mid ? cx : cx + 1), 0), x1 = min(xr ? cx + 1 : (mid ? cx : cx - 1), g.dim[0] - 1);
                const int c  = in ? g.dim[0] * (y + g.dim[1] * z) : 0;
                const bool some = in && x0 <= x1;
                const int b = cell_start[c + (some ? x0 : 0)], e = cell_start[c + (some ? x1 + 1 : 0)];
                rbeg[i] = some ? b : 0, rend[i] = some ? e : 0;
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) scan_range(rbeg[i], rend[i]);  // (one key per lane: the order does not matter here)
        }
        const float b1 = fmaxf(1.f + margin - 1e-3f, 0.f) * g.cs;
        if (best.dist(K - 1) < b1 * b1 * 0.9999f) return;
        r_first = 2;
        // Not settled by shells 0 and 1 (the surface has moved by more than a cell): whatever they found is an upper bound d
        // of the answer, and everything at most that far away lies in the cells that meet the ball of radius sqrt(d) around
        // the query — per (dy, dz) row one contiguous x range of cells, the rows of a z layer requested together.  That is
        // the exact answer (ties included: the ball is closed, with the margins of the stop rules), for the price of the
        // ball's cells instead of whole Chebyshev shells walked cell by cell with two dependent table loads each (2.2 ms
        // against 0.13 ms per 262 k queries when the cloud had moved by a centimetre).  Balls wider than RB cells, queries
        // outside the grid and empty neighbourhoods take the shell loop below.
        constexpr int RB = 4;
        auto reach = [&](float r, float w) { return r > w ? (int)fminf((r - w) * g.inv_cs, 1e6f) + 1 : 0; };
        // (nothing within the block: the ball is tried at two cells and grown by one until it holds a point — then that point,
        // or one nearer inside the same ball, is the answer.  A ball that holds a known point settles at once, so only the
        // balls that were EMPTY grow — and a grown ball scans only the cells the larger radius adds: per row the two ends of
        // its x range beyond the range of the ball before, nothing of which held a point.  The first form scanned the whole
        // ball again on every growth; `rescan` — development builds — keeps that form for the comparison.)
        float rad   = best.dist(K - 1) < 3.0e38f ? sqrtf(best.dist(K - 1)) * 1.0001f : 2.f * g.cs;
        bool settled = false;
        for (int attempt = 0; attempt < RB; ++attempt) {
            const float rad_p = attempt > 0 && !rescan ? rad - g.cs : -1.f;  // the (empty) ball this lane scanned before
            const int nzl = reach(rad, wall[2][0]), nzh = reach(rad, wall[2][1]), nyl = reach(rad, wall[1][0]), nyh = reach(rad, wall[1][1]);
            const bool ball = inside && !settled && max(max(nzl, nzh), max(nyl, nyh)) <= RB &&
                              max(reach(rad, wall[0][0]), reach(rad, wall[0][1])) <= RB;
            if (__ballot(ball) == 0ull) break;
            int zl = 0, zh = 0;  // the wave's reach in z (ballots: lanes that left the search earlier take no part)
#pragma unroll
            for (int v = 1; v <= RB; ++v) {
                if (__ballot(ball && nzl >= v) != 0ull) zl = v;
                if (__ballot(ball && nzh >= v) != 0ull) zh = v;
            }
            for (int sz = 0; sz <= 2 * max(zl, zh); ++sz) {  // z layers nearest first: 0, +1, -1, +2, ...
                const int dz = (sz & 1) ? (sz + 1) / 2 : -(sz / 2);
                if (dz > zh || -dz > zl) continue;  // (wave-uniform)
                const float ez = dz == 0 ? 0.f : (dz < 0 ? wall[2][0] : wall[2][1]) + (float)(abs(dz) - 1) * g.cs;
                int rb[2 * RB + 1], re[2 * RB + 1], pb[2 * RB + 1], pe[2 * RB + 1];
#pragma unroll
                for (int i = 0; i <= 2 * RB; ++i) {
                    const int dy   = i - RB;
                    const float ey = dy == 0 ? 0.f : (dy < 0 ? wall[1][0] : wall[1][1]) + (float)(abs(dy) - 1) * g.cs;
                    const float rem = rad * rad - ey * ey - ez * ez;
                    const int z = cz + dz, y = cy + dy;
                    const bool row = ball && rem >= 0.f && dz <= nzh && -dz <= nzl && dy <= nyh && -dy <= nyl && z >= 0 &&
                                     z < g.dim[2] && y >= 0 && y < g.dim[1];
                    const float sx = sqrtf(fmaxf(rem, 0.f));
                    const int x0 = max(cx - reach(sx, wall[0][0]), 0), x1 = min(cx + reach(sx, wall[0][1]), g.dim[0] - 1);
                    const int c  = row ? g.dim[0] * (y + g.dim[1] * z) : 0;
                    const int b = cell_start[c + (row ? x0 : 0)], e = cell_start[c + (row ? x1 + 1 : 0)];
                    // the part of this row the ball before covered (same formulas at the radius before: a sub-range)
                    const float remp = rad_p * rad_p - ey * ey - ez * ez;
                    const bool prow  = row && rad_p > 0.f && remp >= 0.f;
                    const float sxp  = sqrtf(fmaxf(remp, 0.f));
                    const int x0p = max(cx - reach(sxp, wall[0][0]), x0), x1p = min(cx + reach(sxp, wall[0][1]), x1);
                    const int bp = cell_start[c + (prow ? x0p : 0)], ep = cell_start[c + (prow ? x1p + 1 : 0)];
                    rb[i] = row ? b : 0, re[i] = row ? e : 0;
                    pb[i] = prow ? bp : re[i], pe[i] = prow ? ep : re[i];  // (no ball before: [rb, re) and an empty second part)
                }
#pragma unroll
                for (int i = 0; i <= 2 * RB; ++i) scan_range(rb[i], pb[i]), scan_range(pe[i], re[i]);
            }
            // every point within `rad` of the query has been looked at: a best inside the ball is the nearest point
            if (ball && best.dist(K - 1) <= rad * rad * 0.9999f) settled = true;
            else rad += g.cs;  // (only balls that were empty so far get here: one more cell)
        }
        if (settled) return;
    }
    if (!TIGHT) {
        // Shells 0 and 1 together: the 3 x 3 x 3 block around the query's cell is nine x-rows of cells, and the cells of
        // an x-row are consecutive in the sorted node array — nine contiguous candidate ranges (18 cell_start loads)
        // instead of 27 cells (54) walked one by one.  Nearly every query ends here: the stop rule below is that of r = 1.
        // The query is a chain of dependent loads and little else (a wave of 64 queries is resident from launch to end:
        // 4 waves per SIMD at C2), so the loads are issued for memory-level parallelism (scan_block3 above).
        if (ONE_LOOP) walk_block3();
        else scan_block3();
        if (best.dist(K - 1) < g.cs * g.cs * 0.9999f) return;  // (r = 1: every node not visited is at least one cell away)
        r_first = 2;  // (a grid of at most 2 cells per axis has been visited completely: the loop below does not run)
    }
    for (int r = r_first; r < rmax; ++r) {
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dim[2] - 1);
        const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dim[1] - 1);
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dim[0] - 1);
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const bool face = (abs(z - cz) == r) || (abs(y - cy) == r);
                // on a z/y face of the shell every x belongs to it; otherwise only the two x ends
                const int xstep = face ? 1 : max(x1 - x0, 1);
                for (int x = x0; x <= x1; x += xstep) {
                    if (!face && abs(x - cx) != r) continue;
                    const int c   = x + g.dim[0] * (y + g.dim[1] * z);
                    const int beg = cell_start[c], end = cell_start[c + 1];
                    for (int j = beg; j < end; ++j) {
                        const float4 n = sorted[j];
                        best.push(dist2(q, n.x, n.y, n.z), __float_as_int(n.w));
                    }
                }
            }
        // every node not visited yet is at least r*cs away (from the query's projection onto
        // the grid, hence from the query); stop when the k-th candidate is strictly closer,
        // with a relative margin that absorbs the rounding of the cell assignment
        // (TIGHT: the cell coordinate of a point is rounded with an error ~1e-5 cells at 128 cells per
        // axis, twice that at 256; 1e-3 cells are taken off the bound before the relative margin)
        const float bound = TIGHT ? fmaxf((float)r + margin - 1e-3f, 0.f) * g.cs : (float)r * g.cs;
        if (best.dist(K - 1) < bound * bound * 0.9999f) break;
    }
}

// ---- wave-cooperative grid search: ONE WAVE PER QUERY -----------------------------------------
// For a few thousand queries (the node -> node regularisation graph) one lane per query leaves
// most of the chip idle and every lane walks ~100 cells serially.  Here the 64 lanes of a wave
// split the cells of each shell, keep private sorted lists, stop when at least K candidates lie
// strictly inside the shell bound, and merge their lists with K rounds of a 64-bit wave minimum
// on (distance bits << 32 | index) keys — the same (distance, index) order as the other paths.
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v                          = t < v ? t : v;
    }
    return v;
}

// the search and merge of one query by one wave: on return every lane holds the K nearest nodes (ascending by (distance,
// index), -1 = absent) in `out`
template <int K>
__device__ __forceinline__ void knn_wave_search(const KnnGridDesc& g, const int32_t* __restrict__ cell_start,
                                                const float4* __restrict__ sorted, f3 q, int lane, int (&out)[K]) {
    KnnList<K> best;
    best.init();
    int cx, cy, cz;
    cell_of(g, q, cx, cy, cz);
    const int rmax = max(g.dim[0], max(g.dim[1], g.dim[2]));
    for (int r = 0; r < rmax; ++r) {
        const int side = 2 * r + 1, ncell = side * side * side;
        for (int c = lane; c < ncell; c += 64) {
            const int dx = c % side - r, dy = (c / side) % side - r, dz = c / (side * side) - r;
            if (max(abs(dx), max(abs(dy), abs(dz))) != r) continue;  // interior: earlier shells
            const int x = cx + dx, y = cy + dy, z = cz + dz;
            if (x < 0 || y < 0 || z < 0 || x >= g.dim[0] || y >= g.dim[1] || z >= g.dim[2]) continue;
            const int cell = x + g.dim[0] * (y + g.dim[1] * z);
            const int beg = cell_start[cell], end = cell_start[cell + 1];
            for (int j = beg; j < end; ++j) {
                const float4 n = sorted[j];
                best.push(dist2(q, n.x, n.y, n.z), __float_as_int(n.w));
            }
        }
        // unvisited nodes are >= r*cs away: done once K candidates are strictly closer (margin as in
        // knn_grid_query)
        const float bound = (float)r * g.cs, b2 = bound * bound * 0.9999f;
        int inside = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) inside += best.dist(j) < b2 ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) inside += __shfl_xor(inside, o, 64);
        if (inside >= K) break;
    }
    // merge: K rounds of wave-min over each lane's current head
    int pos = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        unsigned long long key = KnnList<K>::EMPTY;
#pragma unroll
        for (int t = 0; t < K; ++t)
            if (t == pos) key = best.key[t];
        const int hi = (int)(unsigned int)key;
        const unsigned long long win = wave_min_u64(key);
        if (key == win && hi != 0x7fffffff) ++pos;
        const int n = (int)(win & 0xffffffffu);
        out[j]      = n == 0x7fffffff ? -1 : n;
    }
}

}  // namespace dfa
