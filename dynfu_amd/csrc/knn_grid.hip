// knn_grid.hip — construction of the uniform grids that the exact searches of knn_device.hpp walk: the node grid (at most 32^3
// cells; four launches, or one workgroup up to GRID_ONE_MAX nodes) and the point grid of large point sets (the same structure
// at up to 256^3 cells, built by multi-workgroup kernels).  Bounding box, geometry, cell histogram, exclusive scan and
// counting-sort fill, all on the device: desc / cell_start / sorted of a KnnGridView (kernels.hpp).
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"
#include "knn_device.hpp"

namespace dfa {

// ------------------------------------------------------------------------------ uniform grid
__global__ __launch_bounds__(1024) void grid_setup_kernel(const float* __restrict__ node_pos, int D,
                                                          KnnGridDesc* __restrict__ desc,
                                                          int32_t* __restrict__ cell_count) {
    __shared__ float smin[3][16], smax[3][16];
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = threadIdx.x; i < D; i += blockDim.x)
        for (int c = 0; c < 3; ++c) {
            const float v = node_pos[3 * (size_t)i + c];
            mn[c] = fminf(mn[c], v), mx[c] = fmaxf(mx[c], v);
        }
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
        }
        if ((threadIdx.x & 63) == 0) smin[c][threadIdx.x >> 6] = mn[c], smax[c][threadIdx.x >> 6] = mx[c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KNN_GRID_MAX_CELLS; i += blockDim.x) cell_count[i] = 0;
    if (threadIdx.x == 0) {
        float ext[3];
        for (int c = 0; c < 3; ++c) {
            float a = smin[c][0], b = smax[c][0];
            for (int w = 1; w < (int)(blockDim.x >> 6); ++w) a = fminf(a, smin[c][w]), b = fmaxf(b, smax[c][w]);
            desc->bmin[c] = a;
            ext[c]        = fmaxf(b - a, 0.f);
        }
        const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
        // ~2 node spacings for nodes on a surface; never more than 32 cells per axis
        float cs = cbrtf((ext[0] * ext[1] * ext[2]) / (float)D);
        cs       = fmaxf(cs, emax / (float)KNN_GRID_MAX_DIM);
        if (!(cs > 0.f)) cs = 1.f;  // all nodes coincide
        desc->cs     = cs;
        desc->inv_cs = 1.f / cs;
        for (int c = 0; c < 3; ++c) {
            int n = (int)(ext[c] * desc->inv_cs) + 1;
            desc->dim[c] = min(max(n, 1), KNN_GRID_MAX_DIM);
        }
    }
}

__global__ __launch_bounds__(256) void grid_count_kernel(const float* __restrict__ node_pos, int D,
                                                         const KnnGridDesc* __restrict__ desc,
                                                         int32_t* __restrict__ cell_count,
                                                         int32_t* __restrict__ node_cell) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    const KnnGridDesc g = *desc;
    int cx, cy, cz;
    cell_of(g, mk3(node_pos[3 * (size_t)i], node_pos[3 * (size_t)i + 1], node_pos[3 * (size_t)i + 2]), cx, cy, cz);
    const int c  = cx + g.dim[0] * (cy + g.dim[1] * cz);
    node_cell[i] = c;
    atomicAdd(&cell_count[c], 1);
}

// exclusive scan of KNN_GRID_MAX_CELLS counts by one workgroup (32 consecutive cells per thread)
__global__ __launch_bounds__(1024) void grid_scan_kernel(int32_t* __restrict__ cell_count /* in: counts, out: cursors */,
                                                         int32_t* __restrict__ cell_start) {
    __shared__ int32_t wave_tot[16];
    constexpr int PER = KNN_GRID_MAX_CELLS / 1024;
    const int base    = threadIdx.x * PER;
    int loc[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) loc[j] = cell_count[base + j], sum += loc[j];
    int incl        = sum;
    const int lane  = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int off = incl - sum;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        cell_start[base + j] = off;
        cell_count[base + j] = off;  // running cursor for the fill pass
        off += loc[j];
    }
    if (threadIdx.x == 1023) cell_start[KNN_GRID_MAX_CELLS] = off;
}

__global__ __launch_bounds__(256) void grid_fill_kernel(const float* __restrict__ node_pos, int D,
                                                        const int32_t* __restrict__ node_cell,
                                                        int32_t* __restrict__ cursor,
                                                        float4* __restrict__ sorted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    const int slot = atomicAdd(&cursor[node_cell[i]], 1);
    sorted[slot]   = make_float4(node_pos[3 * (size_t)i], node_pos[3 * (size_t)i + 1], node_pos[3 * (size_t)i + 2],
                                 __int_as_float(i));
}

// The same grid for a deformation-node set (D <= GRID_ONE_MAX nodes) built by ONE workgroup: bounding box, geometry,
// cell histogram, exclusive scan and the counting-sort fill all in LDS (the 32^3 counters are 128 KiB) — one launch of
// ~8 us instead of four (setup 6 + count 5 + scan 13 + fill 5 us and three kernel boundaries at C2, twice per frame in
// the pipelined schedule).  Same desc / cell_start / sorted as the four-kernel path (order inside a cell is that of the
// atomics in both: the searches order candidates by (distance, index) themselves).
constexpr int GRID_ONE_MAX = 8192;
__global__ __launch_bounds__(1024) void grid_build_one_kernel(const float* __restrict__ node_pos, int D,
                                                              KnnGridDesc* __restrict__ desc,
                                                              int32_t* __restrict__ cell_start,
                                                              float4* __restrict__ sorted) {
    extern __shared__ int32_t cnt[];  // KNN_GRID_MAX_CELLS counters, then cursors
    __shared__ float smin[3][16], smax[3][16];
    __shared__ int32_t wave_tot[16];
    __shared__ KnnGridDesc gsh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = tid; i < D; i += 1024)
        for (int c = 0; c < 3; ++c) {
            const float v = node_pos[3 * (size_t)i + c];
            mn[c] = fminf(mn[c], v), mx[c] = fmaxf(mx[c], v);
        }
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
        }
        if (lane == 0) smin[c][wave] = mn[c], smax[c][wave] = mx[c];
    }
    __syncthreads();
    if (tid == 0) {  // geometry: the arithmetic of grid_setup_kernel
        float ext[3];
        for (int c = 0; c < 3; ++c) {
            float a = smin[c][0], b = smax[c][0];
            for (int w = 1; w < 16; ++w) a = fminf(a, smin[c][w]), b = fmaxf(b, smax[c][w]);
            gsh.bmin[c] = a;
            ext[c]      = fmaxf(b - a, 0.f);
        }
        const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
        float cs = cbrtf((ext[0] * ext[1] * ext[2]) / (float)D);
        cs       = fmaxf(cs, emax / (float)KNN_GRID_MAX_DIM);
        if (!(cs > 0.f)) cs = 1.f;
        gsh.cs     = cs;
        gsh.inv_cs = 1.f / cs;
        for (int c = 0; c < 3; ++c) {
            const int n = (int)(ext[c] * gsh.inv_cs) + 1;
            gsh.dim[c]  = min(max(n, 1), KNN_GRID_MAX_DIM);
        }
        *desc = gsh;
    }
    __syncthreads();
    const KnnGridDesc g = gsh;
    // only the cells of this grid are cleared, scanned and published (the searches never index beyond dim x dim x dim):
    // wave w owns PER consecutive cells, 64 per step
    const int ncells = g.dim[0] * g.dim[1] * g.dim[2];
    const int PER    = ((ncells + 16 * 64 - 1) / (16 * 64)) * 64;  // <= KNN_GRID_MAX_CELLS / 16
    for (int j = 0; j < PER; j += 64) cnt[wave * PER + j + lane] = 0;
    __syncthreads();
    for (int i = tid; i < D; i += 1024) {
        int cx, cy, cz;
        cell_of(g, mk3(node_pos[3 * (size_t)i], node_pos[3 * (size_t)i + 1], node_pos[3 * (size_t)i + 2]), cx, cy, cz);
        atomicAdd(&cnt[cx + g.dim[0] * (cy + g.dim[1] * cz)], 1);
    }
    __syncthreads();
    // exclusive scan in cell order
    int carry = 0;
    for (int j = 0; j < PER; j += 64) {
        const int idx  = wave * PER + j + lane;
        const int v    = cnt[idx];
        const int incl = wave_inclusive_scan(v);
        cnt[idx]       = carry + incl - v;
        carry += __builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) wave_tot[wave] = carry;
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    for (int j = 0; j < PER; j += 64) {
        const int idx   = wave * PER + j + lane;
        const int start = cnt[idx] + off;
        cnt[idx]        = start;  // cursor of the fill
        if (idx <= ncells) cell_start[idx] = start;
    }
    if (tid == 1023 && 16 * PER <= ncells) cell_start[ncells] = off + carry;  // (16 PER == ncells: the end marker)
    __syncthreads();
    for (int i = tid; i < D; i += 1024) {
        const float px = node_pos[3 * (size_t)i], py = node_pos[3 * (size_t)i + 1], pz = node_pos[3 * (size_t)i + 2];
        int cx, cy, cz;
        cell_of(g, mk3(px, py, pz), cx, cy, cz);
        const int slot = atomicAdd(&cnt[cx + g.dim[0] * (cy + g.dim[1] * cz)], 1);
        sorted[slot]   = make_float4(px, py, pz, __int_as_float(i));
    }
}

// ---- large point sets (the canonical cloud of dfa_correspond): up to 128^3 cells, 256^3 above 500 k points ----
// Same data structure, built by multi-workgroup kernels: bounding box by per-block partials, the
// exclusive scan of the cell counts in chunks of PGRID_CHUNK cells (chunk sums, then a scan kernel
// that first adds up the sums of the chunks before it).
__global__ __launch_bounds__(256) void pgrid_bbox_kernel(const float* __restrict__ pts, int n,
                                                         float* __restrict__ partials /* gridDim.x x 6 */) {
    __shared__ float sh[6][4];
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        for (int c = 0; c < 3; ++c) {
            const float v = pts[3 * (size_t)i + c];
            mn[c] = fminf(mn[c], v), mx[c] = fmaxf(mx[c], v);
        }
    for (int c = 0; c < 3; ++c) {
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
        }
        if ((threadIdx.x & 63) == 0) sh[c][threadIdx.x >> 6] = mn[c], sh[3 + c][threadIdx.x >> 6] = mx[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int c = threadIdx.x;
        float a     = sh[c][0];
        for (int w = 1; w < 4; ++w) a = c < 3 ? fminf(a, sh[c][w]) : fmaxf(a, sh[c][w]);
        partials[6 * blockIdx.x + c] = a;
    }
}

__global__ __launch_bounds__(64) void pgrid_finalize_kernel(const float* __restrict__ partials, int nblocks, int n,
                                                            KnnGridDesc* __restrict__ desc) {
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int b = threadIdx.x; b < nblocks; b += 64)
        for (int c = 0; c < 3; ++c) mn[c] = fminf(mn[c], partials[6 * b + c]), mx[c] = fmaxf(mx[c], partials[6 * b + 3 + c]);
    for (int c = 0; c < 3; ++c)
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = fminf(mn[c], __shfl_xor(mn[c], o, 64));
            mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], o, 64));
        }
    if (threadIdx.x == 0) {
        float ext[3];
        for (int c = 0; c < 3; ++c) desc->bmin[c] = mn[c], ext[c] = fmaxf(mx[c] - mn[c], 0.f);
        const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
        // points of a surface: the volume rule over-estimates the spacing, so aim below it and let the
        // cells-per-axis cap decide for thin clouds.  Up to half a million points: 128 cells per axis (2 M cells, 8 MiB of
        // counters to clear and scan per build).  Above (a 512^3 volume's surface: a million vertices) the search
        // walks ~70 points per cell at that cap, so the cap doubles and the aim halves: ~20 points per cell, a search
        // 2.5x shorter for ~40 us more of clearing and scanning.
        const bool large = n > 500000;
        float cs = (large ? 0.5f : 0.7f) * cbrtf((ext[0] * ext[1] * ext[2]) / (float)n);
        cs       = fmaxf(cs, emax / (float)(large ? PGRID_MAX_DIM : 128));
        if (!(cs > 0.f)) cs = 1.f;
        desc->cs = cs, desc->inv_cs = 1.f / cs;
        // clamped with the SAME cap the cell size was derived from (and the host's chunk count assumes, point_grid_build):
        // dim[0] dim[1] dim[2] <= cap^3 whatever the rounding of ext / cs does
        const int cap = large ? PGRID_MAX_DIM : 128;
        for (int c = 0; c < 3; ++c) desc->dim[c] = min(max((int)(ext[c] * desc->inv_cs) + 1, 1), cap);
    }
}

__device__ __forceinline__ int pgrid_cells(const KnnGridDesc& g) { return g.dim[0] * g.dim[1] * g.dim[2]; }

__global__ __launch_bounds__(256) void pgrid_clear_kernel(const KnnGridDesc* __restrict__ desc,
                                                          int32_t* __restrict__ cell_count) {
    const int nc = pgrid_cells(*desc);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nc; i += gridDim.x * blockDim.x) cell_count[i] = 0;
}

__global__ __launch_bounds__(256) void pgrid_sum_kernel(const KnnGridDesc* __restrict__ desc,
                                                        const int32_t* __restrict__ cell_count,
                                                        int32_t* __restrict__ chunk_sums) {
    __shared__ int sh[4];
    const int nc = pgrid_cells(*desc), base = blockIdx.x * PGRID_CHUNK;
    int sum = 0;
    for (int i = base + threadIdx.x; i < min(base + PGRID_CHUNK, nc); i += 256) sum += cell_count[i];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// exclusive scan of the (at most PGRID_MAX_CELLS / PGRID_CHUNK = 2048) chunk totals, in place, by one workgroup
__global__ __launch_bounds__(256) void pgrid_chunkscan_kernel(int32_t* __restrict__ chunk_sums, int chunks) {
    __shared__ int wsum[4];
    constexpr int PER = (PGRID_MAX_CELLS / PGRID_CHUNK + 255) / 256;
    int loc[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = (int)threadIdx.x * PER + j;
        loc[j]      = i < chunks ? chunk_sums[i] : 0;
        sum += loc[j];
    }
    int incl       = sum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int off = incl - sum;
    for (int w = 0; w < wave; ++w) off += wsum[w];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = (int)threadIdx.x * PER + j;
        if (i < chunks) chunk_sums[i] = off;
        off += loc[j];
    }
}

__global__ __launch_bounds__(256) void pgrid_scan_kernel(const KnnGridDesc* __restrict__ desc,
                                                         int32_t* __restrict__ cell_count /* in: counts, out: cursors */,
                                                         int32_t* __restrict__ cell_start,
                                                         const int32_t* __restrict__ chunk_sums) {
    __shared__ int sh[4], sh2[4];
    const int nc = pgrid_cells(*desc), base = blockIdx.x * PGRID_CHUNK;
    if (base >= nc) return;
    // offset of this chunk: chunk_sums holds the exclusive scan of the chunk totals (pgrid_chunkscan_kernel)
    if (threadIdx.x < 4) sh[threadIdx.x] = threadIdx.x == 0 ? chunk_sums[blockIdx.x] : 0;
    constexpr int PER = PGRID_CHUNK / 256;
    const int first   = base + threadIdx.x * PER;
    // a thread's PER = 32 cells are 128 contiguous bytes: sixteen-byte accesses (dword accesses at a 128-byte lane stride were
    // 32 instructions of 64 cache lines each way: 84 us for the 16.7 M cells of a 256^3 grid)
    static_assert(PER % 4 == 0, "cells per thread in groups of four");
    const bool whole = first + PER <= nc;  // (all of the thread's cells exist: every thread but the grid's last few)
    int loc[PER], sum = 0;
    if (whole) {
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const int4 c4 = reinterpret_cast<const int4*>(cell_count + first)[q];
            loc[4 * q] = c4.x, loc[4 * q + 1] = c4.y, loc[4 * q + 2] = c4.z, loc[4 * q + 3] = c4.w;
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) sum += loc[j];
    } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) loc[j] = first + j < nc ? cell_count[first + j] : 0, sum += loc[j];
    }
    int incl       = sum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) sh2[wave] = incl;
    __syncthreads();
    int off = sh[0] + sh[1] + sh[2] + sh[3] + incl - sum;
    for (int w = 0; w < wave; ++w) off += sh2[w];
    if (whole) {
        int st[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) st[j] = off, off += loc[j];
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            const int4 v = make_int4(st[4 * q], st[4 * q + 1], st[4 * q + 2], st[4 * q + 3]);
            reinterpret_cast<int4*>(cell_start + first)[q] = v;
            reinterpret_cast<int4*>(cell_count + first)[q] = v;
        }
        if (first + PER == nc) cell_start[nc] = off;
        return;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (first + j < nc) {
            cell_start[first + j] = off;
            cell_count[first + j] = off;
            off += loc[j];
            if (first + j == nc - 1) cell_start[nc] = off;
        }
    }
}

// ------------------------------------------------------------------------------ launchers

hipError_t point_grid_build(const PointGridView& pg, const float* pts, int n, hipStream_t s) {
    const KnnGridView& g = pg.g;
    const int nb         = (n + 255) / 256;
    const int bbox_blocks = nb < PGRID_BBOX_BLOCKS ? nb : PGRID_BBOX_BLOCKS;
    pgrid_bbox_kernel<<<bbox_blocks, 256, 0, s>>>(pts, n, pg.bbox_partials);
    pgrid_finalize_kernel<<<1, 64, 0, s>>>(pg.bbox_partials, bbox_blocks, n, g.desc);
    pgrid_clear_kernel<<<1024, 256, 0, s>>>(g.desc, g.cell_count);
    grid_count_kernel<<<nb, 256, 0, s>>>(pts, n, g.desc, g.cell_count, g.node_cell);
    const int chunks = (n > 500000 ? PGRID_MAX_CELLS : 128 * 128 * 128) / PGRID_CHUNK;  // (the cap pgrid_finalize_kernel applies)
    pgrid_sum_kernel<<<chunks, 256, 0, s>>>(g.desc, g.cell_count, pg.chunk_sums);
    pgrid_chunkscan_kernel<<<1, 256, 0, s>>>(pg.chunk_sums, chunks);
    pgrid_scan_kernel<<<chunks, 256, 0, s>>>(g.desc, g.cell_count, g.cell_start, pg.chunk_sums);
    grid_fill_kernel<<<nb, 256, 0, s>>>(pts, n, g.node_cell, g.cell_count, g.sorted);
    return hipGetLastError();
}

hipError_t knn_grid_build(const KnnGridView& g, const float* node_pos, int D, hipStream_t s) {
    if (D <= GRID_ONE_MAX) {
        constexpr size_t lds = sizeof(int32_t) * KNN_GRID_MAX_CELLS;
        // 128 KiB of dynamic LDS needs the opt-in, once per device
        hipError_t e = allow_dynamic_lds((const void*)grid_build_one_kernel, (int)lds);
        if (e != hipSuccess) return e;
        grid_build_one_kernel<<<1, 1024, lds, s>>>(node_pos, D, g.desc, g.cell_start, g.sorted);
        return hipGetLastError();
    }
    grid_setup_kernel<<<1, 1024, 0, s>>>(node_pos, D, g.desc, g.cell_count);
    grid_count_kernel<<<(D + 255) / 256, 256, 0, s>>>(node_pos, D, g.desc, g.cell_count, g.node_cell);
    grid_scan_kernel<<<1, 1024, 0, s>>>(g.cell_count, g.cell_start);
    grid_fill_kernel<<<(D + 255) / 256, 256, 0, s>>>(node_pos, D, g.node_cell, g.cell_count, g.sorted);
    return hipGetLastError();
}

}  // namespace dfa
