// tsdf.hip — gfx950 kernels for the TSDF seam: compute_dists, clear, integrate,
// fused clear+integrate, raycast (points / depth).
//
// What they compute is kfusion's src/kfusion/cuda/tsdf_volume.cu + imgproc.cu:233-245
// (cited per kernel); how they are laid out is MI355X-specific:
//   * the volume is x-fastest, 4 B / voxel; one lane owns one voxel COLUMN and marches it over z, a 256-thread
//     block covers 64 x 4 columns, z is cut into chunks (grid.z) until >= 4 096 workgroups are in flight;
//   * the reference's running `vc += zstep` (tsdf_volume.cu:64) is kept bit-for-bit: a chunk that starts at
//     slice z0 replays the z0 additions in registers first rather than using z0*zstep;
//   * the sweeps classify runs of 8 voxels of a column at once (tsdf_classify.hpp: skipped / in front of the
//     surface / per-voxel arithmetic) from one projection and four min-max tiles of the depth image — most of a
//     volume never sees a division, a gather or a square root, and the fused clear+integrate sweep runs at the
//     speed of its stores;
//   * the depth ("dists") image (600 KiB at VGA) and its tile table (19 KiB) stay in L2 / L1 while the volume
//     streams past them.
// Every kernel is HBM-bound integer/half work; nothing here is GEMM-shaped, no MFMA.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "dev_switch.hpp"
#include "device_memory.hpp"
#include "kernels.hpp"
#include "raycast_device.hpp"
#include "tsdf_classify.hpp"
#include "tsdf_integrate_device.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------
// compute_dists — imgproc.cu:233-245.  2 pixels per lane (one dword in, one dword out).
__global__ __launch_bounds__(256) void compute_dists_kernel(const uint16_t* __restrict__ depth, int depth_step,
                                                            uint16_t* __restrict__ dists, int dists_step, int cols,
                                                            int rows, float finvx, float finvy, float cx, float cy) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const uint16_t* drow = (const uint16_t*)((const char*)depth + (size_t)y * depth_step);
    uint16_t* orow       = (uint16_t*)((char*)dists + (size_t)y * dists_step);
    float xl             = ((float)x - cx) * finvx;
    float yl             = ((float)y - cy) * finvy;
    float lambda         = sqrtf(fmaf(yl, yl, xl * xl) + 1.f);
    orow[x]              = (uint16_t)float_to_half_bits(((float)drow[x] * lambda) * 0.001f);
}

// ------------------------------------------------------------------------------------------
// clear — tsdf_volume.cu:11-22: pack_tsdf(0.f, 0) == 0.  Grid-stride 16-byte stores.
__global__ __launch_bounds__(256) void clear_kernel(uint4* __restrict__ vol4, size_t n4, uint32_t* __restrict__ tail,
                                                    int ntail) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
        vol4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0u;
}

// The store pattern of the fused sweep's zero fill (a lane per voxel column, a wave stores one 256-byte x-row segment per
// slice and marches over z): measured faster than the grid-stride 16-byte stores above at 512^3 and 1024^3 (DESIGN.md
// 4.1), so clear() uses it for volumes with whole 64-voxel rows.
__global__ __launch_bounds__(256) void clear_columns_kernel(uint32_t* __restrict__ vol, int X, int Y, int Z, int zchunk) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= X || y >= Y) return;
    const int z0 = blockIdx.z * zchunk, z1 = min(Z, z0 + zchunk);
    const size_t slice = (size_t)X * Y;
    uint32_t* p        = vol + (size_t)z0 * slice + (size_t)y * X + x;
    int z              = z0;
    for (; z + 8 <= z1; z += 8, p += 8 * slice) {
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u * slice] = 0u;
    }
    for (; z < z1; ++z, p += slice) *p = 0u;
}

// ------------------------------------------------------------------------------------------
// integrate — tsdf_volume.cu:43-96.  IntegrateArgs, div_xy_by_z, voxel_tsdf and voxel_update: tsdf_integrate_device.hpp
// (shared with the warped sweep of tsdf_warped.hip)

// One voxel of one slice (tsdf_volume.cu:65-91).  `old` is the packed voxel (0 when the clear
// is fused); returns the packed voxel after the update and sets `changed`.
template <bool FUSED_CLEAR>
__device__ __forceinline__ uint32_t integrate_voxel(const IntegrateArgs& a, f3 vc, uint32_t old, bool& changed) {
    float tsdf;
    if (!voxel_tsdf(a, vc, tsdf)) return old;
    changed = true;
    return voxel_update<FUSED_CLEAR>(a, old, tsdf);
}

// block = (64, 4): a wave spans 64 voxels in x, the block 4 rows in y; grid.z = z chunks.
template <bool FUSED_CLEAR>
__global__ __launch_bounds__(256) void integrate_kernel(const IntegrateArgs a) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.X || y >= a.Y) return;
    const int z0 = blockIdx.z * a.zchunk;
    const int z1 = min(z0 + a.zchunk, a.Z);

    // :58
    const f3 zstep = mk3(a.vol2cam.m[2], a.vol2cam.m[5], a.vol2cam.m[8]) * a.vsz;
    const f3 t     = mk3(a.vol2cam.t[0], a.vol2cam.t[1], a.vol2cam.t[2]);
    const f3 vx    = mk3((float)x * a.vsx, (float)y * a.vsy, 0.f);  // :60
    f3 vc          = mulR(a.vol2cam, vx) + t;                        // :61
    // replay the z0 running additions of :64 so the chunk starts on the reference's value
    for (int i = 0; i < z0; ++i) vc = vc + zstep;

    const size_t slice = (size_t)a.X * a.Y;
    uint32_t* ptr      = a.vol + (size_t)x + (size_t)a.X * y + slice * z0;

    constexpr int U = 4;  // slices in flight per lane
    int z           = z0;
    for (; z + U <= z1; z += U, ptr += slice * U) {
        uint32_t cur[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = FUSED_CLEAR ? 0u : ptr[slice * u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bool changed = FUSED_CLEAR;  // the fused sweep writes every voxel
            cur[u]       = integrate_voxel<FUSED_CLEAR>(a, vc, cur[u], changed);
            vc           = vc + zstep;  // :64, also for skipped voxels
            if (changed) ptr[slice * u] = cur[u];
        }
    }
    for (; z < z1; ++z, ptr += slice) {
        bool changed     = FUSED_CLEAR;
        const uint32_t v = integrate_voxel<FUSED_CLEAR>(a, vc, FUSED_CLEAR ? 0u : *ptr, changed);
        vc               = vc + zstep;
        if (changed) *ptr = v;
    }
}

// ------------------------------------------------------------------------------------------
// Run-classified sweeps (tsdf_classify.hpp).  Same result as integrate_kernel, voxel for voxel; what changes is the
// work: per run of U slices a lane projects ONE point (the far end of the run; the near end is the previous run's
// far end), looks up four min / max tiles of the dists image and knows whether its U voxels are all skipped, all
// updated with tsdf == 1, or need the reference's per-voxel arithmetic.  At C2 (512^3, U = 8) 83 % of the runs are
// skipped, 10 % are in front of the surface, 7 % take the per-voxel path; a wave does when one of its lanes does.
//   * fused clear + integrate: skipped runs store zeros, front runs a constant — the sweep becomes a store stream;
//   * read + write sweep: skipped runs touch no memory at all.
// A wave covers 32 x 2 columns, a block 64 x 4.  Measured (wave shapes and run lengths of earlier trees, fused sweep, 512^3 / 1024^3):
//   per-voxel kernel 0.222 / 1.174 ms; U = 4, WX = 64: 0.157 / 0.883; U = 8, WX = 64: 0.137 / 0.825;
//   U = 8, WX = 32: 0.117 / 0.721 (128-byte row segments, and lanes that agree more often: 14 % instead of 19 % of
//   the wave runs hold a lane on the per-voxel path); U = 8, WX = 16: 0.161 / 1.236 (64-byte segments: half cache
//   lines); the same loop storing zeros only: 0.105 / 0.773.
constexpr int RUN_U = 8;

__device__ __forceinline__ float rcp_approx(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float half_bits_to_float_u(uint32_t b) { return half_bits_to_float(b); }

// min / max tiles of the dists image: one wave per 8 x 8 tile
__global__ __launch_bounds__(256) void dists_tiles_kernel(const uint16_t* __restrict__ dists, int dists_step, int cols,
                                                          int rows, uint32_t* __restrict__ tiles, int tcols, int ntiles) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const int lane = threadIdx.x & 63;
    const int x = (tile % tcols) * 8 + (lane & 7), y = (tile / tcols) * 8 + (lane >> 3);
    uint32_t lo = 0xffffu, hi = 0u;
    if (x < cols && y < rows) {
        const uint16_t* drow = (const uint16_t*)((const char*)dists + (size_t)y * dists_step);
        const uint32_t t = tile_bounds_of_pixel(drow[x]);
        lo = t & 0xffffu, hi = t >> 16;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
    }
    if (lane == 0) tiles[tile] = lo | (hi << 16);
}

template <bool FUSED_CLEAR>
__global__ __launch_bounds__(256) void integrate_runs_kernel(const IntegrateArgs a, const RunConsts rc, const RunConsts rcc,
                                                             const uint32_t front_const) {
    constexpr int WX = 32, U = RUN_U;  // a wave = 32 x 2 voxel columns, runs of RUN_U voxels
    const int lane  = threadIdx.x, wave = threadIdx.y;  // block (64, 4)
    // the block's 64 x 4 columns, WX x (64 / WX) per wave: waves side by side in x, then stacked in y
    constexpr int WAVES_X = 64 / WX, WAVE_ROWS = 64 / WX;
    const int x = blockIdx.x * 64 + (wave % WAVES_X) * WX + (lane % WX);
    const int y = blockIdx.y * 4 + (wave / WAVES_X) * WAVE_ROWS + lane / WX;
    if (x >= a.X || y >= a.Y) return;
    const int z0 = blockIdx.z * a.zchunk;
    const int z1 = min(z0 + a.zchunk, a.Z);

    const f3 zstep = mk3(a.vol2cam.m[2], a.vol2cam.m[5], a.vol2cam.m[8]) * a.vsz;                  // :58
    const f3 vx    = mk3((float)x * a.vsx, (float)y * a.vsy, 0.f);                                   // :60
    f3 vc          = mulR(a.vol2cam, vx) + mk3(a.vol2cam.t[0], a.vol2cam.t[1], a.vol2cam.t[2]);      // :61
    // (all of a chunk's map bytes up front, as a bit mask: a load per run in front of the decision is a memory round trip per run)
    const size_t occ_layer = (size_t)a.ox * a.oy;
    // bit r of (clean_hi : clean): the box of the chunk's r-th run held zeros on entry (fused sweep over a known map); 128 runs
    // are a whole column of a 1024^3 volume, runs beyond are not known to be clean
    unsigned long long clean = 0ull, clean_hi = 0ull;
    const int nruns          = (z1 - z0) / U;
    if (FUSED_CLEAR && a.occ && a.occ_known) {
        const uint8_t* occ_old = a.occ + (size_t)(x / WX) + (size_t)a.ox * ((size_t)(y / WAVE_ROWS) + (size_t)a.oy * (size_t)(z0 / U));
#pragma unroll 8
        for (int r = 0; r < min(nruns, 64); ++r) clean |= (unsigned long long)(occ_old[(size_t)r * occ_layer] == 0) << r;
#pragma unroll 8
        for (int r = 64; r < min(nruns, 128); ++r) clean_hi |= (unsigned long long)(occ_old[(size_t)r * occ_layer] == 0) << (r - 64);
    }
    // The chunk as a whole first (tsdf_classify.hpp, chunk_skipped): when every column of the wave skips every voxel of it —
    // half of a volume lies outside the frustum — there is nothing to classify or replay; the accumulating sweep leaves such
    // voxels alone anyway, the fused sweep may when the map says they are zeros already (and the chunk has no tail).
    auto ones = [](int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1ull; };
    if (!FUSED_CLEAR || (a.occ && a.occ_known && nruns <= 128 && nruns * U == z1 - z0 && clean == ones(nruns) && clean_hi == ones(nruns - 64))) {
        const float zs[3] = {zstep.x, zstep.y, zstep.z};
        const bool skip   = chunk_skipped(vc.x, vc.y, vc.z, zs, z0, z1, rcc, rcp_approx, half_bits_to_float_u);
        if (__ballot(!skip) == 0ull) return;  // (a skipped chunk leaves the map's bytes as they are: nothing gained a weight)
    }
    for (int i = 0; i < z0; ++i) vc = vc + zstep;  // replay :64 up to the chunk's first slice

    const size_t slice = (size_t)a.X * a.Y;
    uint32_t* ptr      = a.vol + (size_t)x + (size_t)a.X * y + slice * z0;
    const f3 stepU     = mk3(rc.stepU[0], rc.stepU[1], rc.stepU[2]);

    int z      = z0;
    RunEnd end = run_end(vc.x, vc.y, vc.z, rc, rcp_approx);
    // occupancy map: a byte per (this wave's WX x (64 / WX) columns) x (run of 8 slices) — the launcher passes it only for
    // chunks that start on a multiple of 8.  Written by the first live lane of the wave.
    uint8_t* occ_cell = nullptr;
    if (a.occ) {
        const unsigned long long live = __ballot(1);
        if (lane == (int)__ffsll((long long)live) - 1)
            occ_cell = a.occ + (size_t)(x / WX) + (size_t)a.ox * ((size_t)(y / WAVE_ROWS) + (size_t)a.oy * (size_t)(z0 / U));
    }
    // The fused sweep over a volume whose map is KNOWN to describe it (dfa_tsdf_clear_integrate_known_occ): a box whose byte
    // is 0 holds 32 x 2 x 8 zeros, and when none of its runs gets a weight now either, storing those zeros again is the
    // 5/6 of the sweep's traffic that changes nothing (`clean`, read above).
    for (; z + U <= z1; z += U, ptr += slice * U) {
        const bool was_clean = (clean & 1ull) != 0ull;
        clean = (clean >> 1) | (clean_hi << 63), clean_hi >>= 1;
        const f3 far     = vc + stepU;
        const RunEnd nxt = run_end(far.x, far.y, far.z, rc, rcp_approx);
        const int cls    = classify_run(end, nxt, rc, half_bits_to_float_u);
        end              = nxt;
        bool untouched = false;  // (wave-uniform) a box of zeros that stays one
        if (a.occ) {  // (uniform) bit 0: a run of the box was not SKIP (SKIP runs are the only ones that leave, or find, no
                      // weight); bit 1: a run was FULL — the only runs that can leave a NEGATIVE distance (FRONT runs write +1)
            const unsigned mark = (__ballot(cls != RUN_SKIP) != 0ull ? 1u : 0u) | (__ballot(cls == RUN_FULL) != 0ull ? 2u : 0u);
            untouched           = FUSED_CLEAR && was_clean && mark == 0u;
            if (occ_cell) {
                if (FUSED_CLEAR) {
                    if (!untouched) *occ_cell = (uint8_t)mark;
                } else if (mark) *occ_cell = (uint8_t)(*occ_cell | mark);  // (one writer per byte and launch)
                occ_cell += occ_layer;
            }
        }
        f3 p[U];  // the run's voxel positions by the reference's running addition (:64)
#pragma unroll
        for (int u = 0; u < U; ++u) p[u] = vc, vc = vc + zstep;
        if (FUSED_CLEAR) {
            if (untouched) continue;
            uint32_t out[U];
            const uint32_t fill = cls == RUN_FRONT ? front_const : 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) out[u] = fill;
            if (cls == RUN_FULL) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bool changed;
                    out[u] = integrate_voxel<true>(a, p[u], 0u, changed);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) ptr[slice * u] = out[u];
        } else if (cls != RUN_SKIP) {
            uint32_t cur[U];
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = ptr[slice * u];
            if (cls == RUN_FRONT) {
#pragma unroll
                for (int u = 0; u < U; ++u) ptr[slice * u] = voxel_update<false>(a, cur[u], 1.0f);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bool changed    = false;
                    const uint32_t v = integrate_voxel<false>(a, p[u], cur[u], changed);
                    if (changed) ptr[slice * u] = v;
                }
            }
        }
    }
    if (occ_cell && z < z1) *occ_cell = 3;  // (the slices of a tail: marked without looking)
    for (; z < z1; ++z, ptr += slice) {  // tail shorter than a run: per voxel
        bool changed     = FUSED_CLEAR;
        const uint32_t v = integrate_voxel<FUSED_CLEAR>(a, vc, FUSED_CLEAR ? 0u : *ptr, changed);
        if (changed) *ptr = v;
        vc = vc + zstep;
    }
}

// ------------------------------------------------------------------------------------------
// raycast — tsdf_volume.cu:128-337: the march, the trilinear samples and the pixel-to-tile map are raycast_device.hpp

template <bool IDX32>
__global__ __launch_bounds__(256) void raycast_points_kernel(const RaycastArgs a, float* __restrict__ points,
                                                             int points_step, float* __restrict__ normals,
                                                             int normals_step) {
    int x, y;
    tile_pixel(x, y);
    if (x >= a.cols || y >= a.rows) return;
    float4* prow = (float4*)((char*)points + (size_t)y * points_step);
    float4* nrow = (float4*)((char*)normals + (size_t)y * normals_step);
    f3 v, n;
    if (cast_ray<false, IDX32>(a, x, y, v, n)) {
        prow[x] = make_float4(v.x, v.y, v.z, 0.f);  // :312-313
        nrow[x] = make_float4(n.x, n.y, n.z, 0.f);
    } else {
        const float q = qnan();
        prow[x] = nrow[x] = make_float4(q, q, q, q);  // :267
    }
}

template <bool IDX32>
__global__ __launch_bounds__(256) void raycast_depth_kernel(const RaycastArgs a, uint16_t* __restrict__ depth,
                                                            int depth_step, float* __restrict__ normals,
                                                            int normals_step) {
    int x, y;
    tile_pixel(x, y);
    if (x >= a.cols || y >= a.rows) return;
    uint16_t* drow = (uint16_t*)((char*)depth + (size_t)y * depth_step);
    float4* nrow   = (float4*)((char*)normals + (size_t)y * normals_step);
    f3 v, n;
    if (cast_ray<false, IDX32>(a, x, y, v, n)) {
        nrow[x]  = make_float4(n.x, n.y, n.z, 0.f);  // :250
        float mm = v.z * 1000.f;                     // :251, saturating truncation
        mm       = mm < 0.f ? 0.f : (mm > 65535.f ? 65535.f : mm);
        drow[x]  = (uint16_t)(int)mm;
    } else {
        const float q = qnan();
        drow[x]       = 0;  // :204-205
        nrow[x]       = make_float4(q, q, q, q);
    }
}

// the same rays with the work counted instead of the images written (measurement only)
__global__ __launch_bounds__(256) void raycast_tally_kernel(const RaycastArgs a, unsigned long long* __restrict__ counts,
                                                            uint32_t* __restrict__ touched) {
    int x, y;
    tile_pixel(x, y);
    RayTally t{counts, touched, 0u, 0u, 0u, 0u};
    if (x < a.cols && y < a.rows) {
        f3 v, n;
        cast_ray<true>(a, x, y, v, n, &t);
    }
    unsigned int part[4] = {t.entered, t.march, t.hits, t.tri};
    for (int c = 0; c < 4; ++c) {
        unsigned int s = part[c];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&counts[c], (unsigned long long)s);
    }
}

// ------------------------------------------------------------------------------------------
// host-side launchers (called by the C ABI, capi_tsdf.cpp)

static inline hipError_t launch_status() { return hipGetLastError(); }

hipError_t launch_compute_dists(const uint16_t* depth, int depth_step, uint16_t* dists, int dists_step, int cols,
                                int rows, float fx, float fy, float cx, float cy, hipStream_t s) {
    dim3 block(64, 4), grid((cols + 63) / 64, (rows + 3) / 4);
    // host wrapper passes finv = 1/f (imgproc.cu:252)
    compute_dists_kernel<<<grid, block, 0, s>>>(depth, depth_step, dists, dists_step, cols, rows, 1.f / fx, 1.f / fy,
                                                cx, cy);
    return launch_status();
}

static int pick_zchunk(int X, int Y, int Z, bool fused_clear);

hipError_t launch_tsdf_clear(uint32_t* vol, int X, int Y, int Z, hipStream_t s) {
    const size_t n = (size_t)X * Y * Z;
    if (X % 64 == 0 && Z >= 32 && (((uintptr_t)vol & 255) == 0)) {
        const int zchunk = pick_zchunk(X, Y, Z, true);
        dim3 block(64, 4), grid(X / 64, (Y + 3) / 4, (Z + zchunk - 1) / zchunk);
        clear_columns_kernel<<<grid, block, 0, s>>>(vol, X, Y, Z, zchunk);
        return launch_status();
    }
    // head/tail so the 16-byte stores are aligned whatever pointer the caller passes
    size_t head = ((16 - ((uintptr_t)vol & 15)) & 15) / 4;
    if (head > n) head = n;
    if (head) {
        hipError_t e = hipMemsetAsync(vol, 0, head * 4, s);
        if (e != hipSuccess) return e;
    }
    uint32_t* body  = vol + head;
    const size_t nb = n - head;
    const size_t n4 = nb / 4;
    const int ntail = (int)(nb - n4 * 4);
    size_t blocks   = (n4 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;  // 16 blocks per CU, grid-stride the rest
    if (blocks == 0) blocks = 1;
    clear_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>((uint4*)body, n4, body + n4 * 4, ntail);
    return launch_status();
}

// Scratch for the tile table of one sweep (19 KiB at VGA): internal, so kept per stream (device_memory.hpp).
namespace {
struct TileScratch {
    DeviceBuffer<uint32_t> tiles;
};
}  // namespace

// z-chunk heuristic: enough workgroups to fill 256 CUs several times over, while keeping the
// replayed-additions prologue (z0 adds per chunk) a small fraction of a chunk's work.
static int pick_zchunk(int X, int Y, int Z, bool fused_clear) {
    const long columns_wg = (long)((X + 63) / 64) * ((Y + 3) / 4);
    int zchunk            = Z;
    // Chunks no shorter than 32 slices.  Measured with one voxel per lane (tools/tsdf_kernels.py): the read+write sweep
    // wants >= 16 workgroups per CU (512^3: 0.265 ms with 4 chunks, 0.386 unsplit); the fused sweep has no loads to hide
    // and is as fast with 4 per CU (512^3 unsplit 0.24 ms, 4 chunks 0.23) — and then half of the chip's wave slots stay
    // free for the kernels of other streams: the per-frame sweep runs beside the solve, whose short full-chip kernels
    // otherwise wait for resident sweep waves to retire (C2 frame 0.969 -> 0.957 ms, C3 4.27 -> 4.10).
    const long want = fused_clear ? 1024 : 4096;
    while (columns_wg * ((Z + zchunk - 1) / zchunk) < want && zchunk > 32) zchunk /= 2;
    zchunk = (zchunk + 3) & ~3;
    if (const char* e = dev_env("DFA_TSDF_ZCHUNK")) {  // (development builds: the tests of the z-chunk independence)
        int v = atoi(e);
        if (v > 0) zchunk = v;
    }
    return zchunk;
}

hipError_t launch_tsdf_integrate(bool fused_clear, const uint16_t* dists, int dists_step, int cols, int rows,
                                 uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                 int max_weight, const float vol2cam[12], float fx, float fy, float cx, float cy,
                                 uint8_t* occ, bool occ_known, hipStream_t s) {
    IntegrateArgs a;
    a.occ_known = occ && occ_known && fused_clear ? 1 : 0;
    a.dists = dists, a.dists_step = dists_step, a.cols = cols, a.rows = rows;
    a.vol = vol, a.X = X, a.Y = Y, a.Z = Z;
    const OccDims od = occ_dims(X, Y, Z);
    a.occ = nullptr, a.ox = od.ox, a.oy = od.oy;
    a.vsx = voxel_size[0], a.vsy = voxel_size[1], a.vsz = voxel_size[2];
    a.trunc      = trunc_dist;
    a.trunc_inv  = 1.f / trunc_dist;  // tsdf_volume.cu:106
    a.max_weight = max_weight;
    for (int i = 0; i < 9; ++i) a.vol2cam.m[i] = vol2cam[i];
    for (int i = 0; i < 3; ++i) a.vol2cam.t[i] = vol2cam[9 + i];
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    // The run-classified sweep.  Development builds (-DDFA_DEV_AB): DFA_TSDF_LEGACY=1 runs the per-voxel sweep (every voxel
    // through the projection; the round-1 kernel) for A/B timings.
    const bool legacy = dev_env("DFA_TSDF_LEGACY") != nullptr;
    if (!legacy) {
        const int tcols = (cols + 7) >> TSDF_TILE_SHIFT, trows = (rows + 7) >> TSDF_TILE_SHIFT;
        DeviceBuffer<uint32_t>& table = stream_scratch<TileScratch>(s).tiles;
        hipError_t e                  = table.reserve((size_t)tcols * trows);
        if (e != hipSuccess) return e;
        uint32_t* tiles = table.data;
        dists_tiles_kernel<<<(tcols * trows + 3) / 4, 256, 0, s>>>(dists, dists_step, cols, rows, tiles, tcols, tcols * trows);
        // bound of |component| over every voxel position in camera space: the 8 corners of the volume
        float extent = 0.f;
        for (int c = 0; c < 8; ++c) {
            const float p[3] = {(c & 1) ? a.vsx * X : 0.f, (c & 2) ? a.vsy * Y : 0.f, (c & 4) ? a.vsz * Z : 0.f};
            for (int r = 0; r < 3; ++r)
                extent = fmaxf(extent, fabsf(vol2cam[3 * r] * p[0] + vol2cam[3 * r + 1] * p[1] + vol2cam[3 * r + 2] * p[2] + vol2cam[9 + r]));
        }
        const float zstep[3] = {vol2cam[2] * a.vsz, vol2cam[5] * a.vsz, vol2cam[8] * a.vsz};
        if (extent == extent && extent < 1e30f) {  // finite poses only; anything else takes the per-voxel sweep
            const RunConsts rc = make_run_consts(tiles, cols, rows, fx, fy, cx, cy, trunc_dist, zstep, RUN_U, extent);
            const uint32_t front_const = 0x3c00u | ((uint32_t)(max_weight < 1 ? max_weight : 1) << 16);  // (1.0h, min(1, max_weight))
            // >= 4 096 workgroups for either sweep: the tile look-ups of a run are dependent loads that only occupancy
            // hides (512^3 fused: 0.147 ms unsplit = 1 024 workgroups, 0.117 ms with z-chunks of 128 slices)
            a.zchunk = pick_zchunk(X, Y, Z, false);
            if (occ) a.zchunk = (a.zchunk + 7) & ~7;  // chunks of whole runs: a byte of the map has one writer
            a.occ = occ;
            dim3 block(64, 4), grid((X + 63) / 64, (Y + 3) / 4, (Z + a.zchunk - 1) / a.zchunk);
            // the chunk-level rule: margins of Z running additions
            const RunConsts rcc = make_run_consts(tiles, cols, rows, fx, fy, cx, cy, trunc_dist, zstep, Z, extent);
            if (fused_clear) integrate_runs_kernel<true><<<grid, block, 0, s>>>(a, rc, rcc, front_const);
            else integrate_runs_kernel<false><<<grid, block, 0, s>>>(a, rc, rcc, front_const);
            return launch_status();
        }
    }
    // One voxel per lane.  Four consecutive voxels per lane (16-byte accesses, the first design) lost everywhere: a lane
    // then walks its four voxels one after the other, each with its own early exits, and a wave waits for its slowest
    // lane four times per slice (fused sweep 0.289 -> 0.229 ms at 512^3, 1.49 -> 1.38 ms at 1024^3, 0.061 -> 0.044 ms
    // at 256^3); a wave's 256-byte stores are wide enough for HBM.
    // This sweep does not keep the occupancy map: it marks everything, so the map stays a superset of the voxels with a weight.
    if (occ) {
        const hipError_t oe = hipMemsetAsync(occ, 3, od.bytes(), s);
        if (oe != hipSuccess) return oe;
    }
    a.zchunk = pick_zchunk(X, Y, Z, fused_clear);
    dim3 block(64, 4), grid((X + 63) / 64, (Y + 3) / 4, (Z + a.zchunk - 1) / a.zchunk);
    if (fused_clear) integrate_kernel<true><<<grid, block, 0, s>>>(a);
    else integrate_kernel<false><<<grid, block, 0, s>>>(a);
    return launch_status();
}

// Normals of surface points (marching-cubes vertices) from the TSDF gradient: the raycaster's own compute_normal
// (tsdf_volume.cu:320-336 — central differences of the trilinear interpolant, `delta_factor` voxels apart) applied
// to points given in the volume's metric frame.  The reference leaves the extracted mesh without normals
// (dyn_fusion.cpp:80-88 "temporary workaround until normals are computed via mc"): this is SURVEY 8f rank 2.
__global__ __launch_bounds__(256) void vertex_normals_kernel(const RaycastArgs a, const float4* __restrict__ points, int n,
                                                             float4* __restrict__ normals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = points[i];
    const f3 nn    = compute_normal(a, mk3(p.x, p.y, p.z));  // NaN where a sample leaves the interpolation range
    normals[i]     = make_float4(nn.x, nn.y, nn.z, 0.f);
}

hipError_t launch_vertex_normals(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float delta_factor,
                                 const float* points, int n, float* normals, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const float id12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, id9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    RaycastArgs a = make_raycast_args(vol, X, Y, Z, voxel_size, 1.f, id12, id9, 1.f, 1.f, 0.f, 0.f, 1.f, delta_factor, 0, 0);
    vertex_normals_kernel<<<(n + 255) / 256, 256, 0, s>>>(a, (const float4*)points, n, (float4*)normals);
    return launch_status();
}

// TsdfVolume::fetchNormals — ExtractNormals (tsdf_volume.cu:602-680): the point is taken back into the volume frame
// (q = Rinv (p - t), :617), its nearest voxel (round-half-even, :609-613) must lie inside [2, dim - 3] on every axis
// (:619-620, otherwise the normal is NaN), and the gradient of the interpolant at q is rotated by R and THEN normalised
// (:662; compute_normal normalises in the volume frame).  The voxel test compares the rounded floats with the bounds:
// the same answer as the reference's __float2int_rn, whose saturation and NaN -> 0 keep such points outside as well.
__global__ __launch_bounds__(256) void extract_normals_kernel(const RaycastArgs a, const Aff3 vol2world,
                                                              const float4* __restrict__ points, int n,
                                                              float4* __restrict__ normals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = points[i];
    const f3 q     = mul(a.Rinv, mk3(p.x, p.y, p.z) - mk3(vol2world.t[0], vol2world.t[1], vol2world.t[2]));
    const float gx = rintf(q.x * a.vix), gy = rintf(q.y * a.viy), gz = rintf(q.z * a.viz);
    f3 nn = mk3(qnan(), qnan(), qnan());
    if (gx > 1.f && gy > 1.f && gz > 1.f && gx < (float)(a.X - 2) && gy < (float)(a.Y - 2) && gz < (float)(a.Z - 2))
        nn = normalized(mulR(vol2world, tsdf_gradient(a, q)));
    normals[i] = make_float4(nn.x, nn.y, nn.z, 0.f);
}

hipError_t launch_extract_normals(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], const float vol2world[12],
                                  const float Rinv[9], float delta_factor, const float* points, int n, float* normals,
                                  hipStream_t s) {
    if (n == 0) return hipSuccess;
    const float id12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    RaycastArgs a = make_raycast_args(vol, X, Y, Z, voxel_size, 1.f, id12, Rinv, 1.f, 1.f, 0.f, 0.f, 1.f, delta_factor, 0, 0);
    Aff3 aff;
    for (int i = 0; i < 9; ++i) aff.m[i] = vol2world[i];
    for (int i = 0; i < 3; ++i) aff.t[i] = vol2world[9 + i];
    extract_normals_kernel<<<(n + 255) / 256, 256, 0, s>>>(a, aff, (const float4*)points, n, (float4*)normals);
    return launch_status();
}

hipError_t launch_raycast_points(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3],
                                 float trunc_dist, const float cam2vol[12], const float Rinv[9], float fx, float fy,
                                 float cx, float cy, float step_factor, float delta_factor, float* points,
                                 int points_step, float* normals, int normals_step, int cols, int rows,
                                 hipStream_t s) {
    RaycastArgs a = make_raycast_args(vol, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy,
                                      step_factor, delta_factor, cols, rows);
    dim3 block(256), grid((cols + 15) / 16, (rows + 15) / 16);
    // (development builds: DFA_RAY_IDX64=1 runs the 64-bit voxel index of volumes beyond 2^32 voxels on any volume — the tests)
    if ((uint64_t)X * Y * Z <= (1ull << 32) && !dev_env("DFA_RAY_IDX64")) raycast_points_kernel<true><<<grid, block, 0, s>>>(a, points, points_step, normals, normals_step);
    else raycast_points_kernel<false><<<grid, block, 0, s>>>(a, points, points_step, normals, normals_step);
    return launch_status();
}

hipError_t launch_raycast_tally(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                                float step_factor, float delta_factor, int cols, int rows, unsigned long long* counts,
                                uint32_t* touched, hipStream_t s) {
    RaycastArgs a = make_raycast_args(vol, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy,
                                      step_factor, delta_factor, cols, rows);
    dim3 block(256), grid((cols + 15) / 16, (rows + 15) / 16);
    raycast_tally_kernel<<<grid, block, 0, s>>>(a, counts, touched);
    return launch_status();
}

hipError_t launch_raycast_depth(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                                float step_factor, float delta_factor, uint16_t* depth, int depth_step,
                                float* normals, int normals_step, int cols, int rows, hipStream_t s) {
    RaycastArgs a = make_raycast_args(vol, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy,
                                      step_factor, delta_factor, cols, rows);
    dim3 block(256), grid((cols + 15) / 16, (rows + 15) / 16);
    if ((uint64_t)X * Y * Z <= (1ull << 32) && !dev_env("DFA_RAY_IDX64")) raycast_depth_kernel<true><<<grid, block, 0, s>>>(a, depth, depth_step, normals, normals_step);
    else raycast_depth_kernel<false><<<grid, block, 0, s>>>(a, depth, depth_step, normals, normals_step);
    return launch_status();
}

}  // namespace dfa
