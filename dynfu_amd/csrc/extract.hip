// extract.hip — point-cloud extraction from the packed TSDF volume for gfx950 (TsdfVolume::fetchCloud).
//
// Reference semantics: src/kfusion/cuda/tsdf_volume.cu FullScan6 (:423-598), driven by device::extractCloud
// (:682-699) and TsdfVolume::fetchCloud (src/kfusion/tsdf_volume.cpp:131-147).  A voxel (x, y, z) with z < Z - 1, a
// non-zero weight and a distance F != 1 emits one point on each of its edges to +x (if x + 1 < X), +y (if y + 1 < Y)
// and +z whose far voxel has a weight, a distance Fn != 1 and the strictly opposite sign: the linear zero crossing
// (V.c |Fn| + (V.c + vs.c) |F|) / (|F| + |Fn|) along that axis, V the voxel centre, mapped by vol2world (:461-536).
// The normals (ExtractNormals :602-680) are in tsdf.hip, beside the raycaster's trilinear interpolate they use.
//
// MI355X design.  The reference runs 32 x 6 thread blocks with 32-lane ballots, appends each warp's points at a
// global atomic counter (the order changes from run to run), keeps that counter in static __device__ variables (two
// calls on two streams corrupt each other) and lets the warp that crosses the end of the buffer store all of its
// points past it.  Here the pipeline is marching cubes' (mc.hip), on the same row segments and the same scan:
//   1. count sweep: HBM-bound streaming read.  A lane owns VX = 4 consecutive x voxels (one 16-byte load per row), a
//      wave a 256-voxel row segment of EX_ROWS rows, a thread marches z keeping slice z's EX_ROWS + 1 rows in
//      registers while it loads slice z + 1; the +x neighbour of a lane's last voxel comes from the next lane by a
//      shuffle.  Output: points per row segment, stored only where non-zero.
//   2. exclusive scan of the segment counts (mc.hip: launch_segment_scan).
//   3. emit: persistent waves find the segments with points, re-read their three rows, and every lane stages its
//      points in LDS in the segment's order; the wave then stores 64 consecutive float4 {x, y, z, 0} per instruction.
// The output order is DEFINED — ascending linear voxel index z*X*Y + y*X + x, within a voxel dx, dy, dz — no
// store lands past max_points, and nothing is shared between calls but the per-stream scratch of the caller.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_math.hpp"
#include "kernels.hpp"
#include "vol_rows.hpp"

namespace dfa {

namespace {

struct ExArgs {
    const uint32_t* vol;
    int X, Y, Z;
    int nseg;    // row segments per row: ceil(X / (64 * VX))
    int zchunk;  // count sweep: slices per workgroup
    float vsx, vsy, vsz;
    Aff3 aff;            // volume -> world (the TsdfVolume's pose)
    const uint8_t* occ;  // occupancy map of the volume (kernels.hpp: OccDims: a byte per 32 x 2 x 8 voxels) or null
    int ox, oy, oz;
};

constexpr int EX_ROWS = 4;        // rows of source voxels per wave: 5 row loads per slice serve 4 rows (+y shared)
constexpr int EMIT_WINDOW = 256;  // points a wave stages in LDS at a time

// :468-469 / :475-476 — the far voxel n of an edge, seen from a source voxel of distance F
__device__ __forceinline__ bool crossing(float F, uint32_t n) {
    const float Fn = unpack_tsdf(n);
    return (n >> 16) != 0u && Fn != 1.f && ((F > 0.f && Fn < 0.f) || (F < 0.f && Fn > 0.f));
}

// bit d (0: +x, 1: +y, 2: +z) — the points voxel c emits (:462-463: W != 0 && F != 1)
__device__ __forceinline__ int voxel_mask(uint32_t c, uint32_t nx, uint32_t ny, uint32_t nz) {
    const float F   = unpack_tsdf(c);
    const bool src  = (c >> 16) != 0u && F != 1.f;
    const int m     = (int)crossing(F, nx) | (int)crossing(F, ny) << 1 | (int)crossing(F, nz) << 2;
    return src ? m : 0;
}

// :470-483 (D = 0), :490-503 (D = 1), :510-523 (D = 2) and `aff * p` (device.hpp: R p + t)
template <int D>
__device__ __forceinline__ float4 crossing_point(const ExArgs& a, int x, int y, int z, uint32_t c, uint32_t n) {
    const float F = unpack_tsdf(c), Fn = unpack_tsdf(n);
    f3 p = mk3(((float)x + 0.5f) * a.vsx, ((float)y + 0.5f) * a.vsy, ((float)z + 0.5f) * a.vsz);
    const float d_inv = 1.f / (fabsf(F) + fabsf(Fn));
    if (D == 0) p.x = (p.x * fabsf(Fn) + (p.x + a.vsx) * fabsf(F)) * d_inv;
    if (D == 1) p.y = (p.y * fabsf(Fn) + (p.y + a.vsy) * fabsf(F)) * d_inv;
    if (D == 2) p.z = (p.z * fabsf(Fn) + (p.z + a.vsz) * fabsf(F)) * d_inv;
    const f3 q = mulR(a.aff, p) + mk3(a.aff.t[0], a.aff.t[1], a.aff.t[2]);
    return make_float4(q.x, q.y, q.z, 0.f);
}

// wave total of per-lane point counts in [0, 15]: four ballots + scalar popcounts
__device__ __forceinline__ int wave_sum_4bit(int n) {
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) s += __popcll(__ballot((n >> b) & 1)) << b;
    return s;
}

// With an occupancy map: may the wave's source voxels in map layer L (slices 8L .. 8L + 7) emit a point at all?  A point
// needs a non-zero weight at its source voxel (bit 0 of the source's box B) and a negative distance at the source or at
// the far voxel of its edge (:468), which lies in B or in B's +x, +y or +z neighbour box (bit 1 of one of the four).
// One lane per source box of the wave's footprint — 2 VX boxes in x, EX_ROWS / 2 in y —, one ballot per layer.
template <int VX>
__device__ __forceinline__ bool layer_may_emit(const ExArgs& a, int seg, int y, int L) {
    constexpr int NBX = 2 * VX;
    const int lane = threadIdx.x & 63, bx = seg * NBX + lane % NBX, by = y / 2 + lane / NBX;
    auto at = [&](int x, int yy, int z) -> unsigned {
        return x < a.ox && yy < a.oy && z < a.oz ? a.occ[((size_t)z * a.oy + yy) * a.ox + x] : 0u;
    };
    bool may = false;
    if (lane < NBX * (EX_ROWS / 2)) {
        const unsigned m = at(bx, by, L);
        may = (m & 1u) && ((m | at(bx + 1, by, L) | at(bx, by + 1, L) | at(bx, by, L + 1)) & 2u);
    }
    return __ballot(may) != 0ull;
}

// ------------------------------------------------------------------------------- 1. count
template <int VX>
__global__ __launch_bounds__(256) void extract_count_kernel(const ExArgs a, int32_t* __restrict__ seg_count) {
    const int seg = blockIdx.x, x0 = (seg * 64 + threadIdx.x) * VX;
    const int y  = (blockIdx.y * 4 + threadIdx.y) * EX_ROWS;
    const int z0 = blockIdx.z * a.zchunk, z1 = min(z0 + a.zchunk, a.Z - 1);  // sources: z < Z - 1 (:459)
    if (y >= a.Y || z0 >= z1) return;                                     // (whole waves: no LDS, no barrier here)
    // with a map the chunks are its layers (zchunk = 8): most waves of a sparse volume end here
    if (a.occ && !layer_may_emit<VX>(a, seg, y, z0 / 8)) return;
    Row<VX> lo[EX_ROWS + 1];
    load_rows<VX, EX_ROWS + 1>(a, x0, y, z0, lo);
    for (int z = z0; z < z1; ++z) {
        Row<VX> hi[EX_ROWS + 1];
        load_rows<VX, EX_ROWS + 1>(a, x0, y, z + 1, hi);
#pragma unroll
        for (int r = 0; r < EX_ROWS; ++r) {
            int n = 0;
#pragma unroll
            for (int i = 0; i < VX; ++i) n += __popc(voxel_mask(lo[r].v[i], lo[r].v[i + 1], lo[r + 1].v[i], hi[r].v[i]));
            n = wave_sum_4bit(n);  // 3 VX <= 12 points per lane
            if (threadIdx.x == 0 && n && y + r < a.Y) seg_count[((size_t)z * a.Y + y + r) * a.nseg + seg] = n;
        }
#pragma unroll
        for (int r = 0; r <= EX_ROWS; ++r) lo[r] = hi[r];
    }
}

// ------------------------------------------------------------------------------- 3. emit
// One segment, the whole wave cooperating (wave-uniform arguments): lanes own voxels to find their points and their
// offsets in the segment (a wave prefix sum), stage them in LDS window by window, and then own consecutive POINTS for
// the stores.  `begin` is the segment's first point in the output; nothing at or past max_points is written.
template <int VX>
__device__ __forceinline__ void emit_segment(const ExArgs& a, float4* st, long s, int begin, int count,
                                             float4* __restrict__ out, int max_points) {
    const int seg = (int)(s % a.nseg);
    const long yz = s / a.nseg;
    const int y = (int)(yz % a.Y), z = (int)(yz / a.Y);
    const int lane = threadIdx.x & 63;
    const int x0   = (seg * 64 + lane) * VX;
    const Row<VX> r0 = load_row<VX>(a, x0, y, z), ry = load_row<VX>(a, x0, y + 1, z), rz = load_row<VX>(a, x0, y, z + 1);
    int mask[VX], mine = 0;
#pragma unroll
    for (int i = 0; i < VX; ++i) {
        mask[i] = voxel_mask(r0.v[i], r0.v[i + 1], ry.v[i], rz.v[i]);
        mine += __popc(mask[i]);
    }
    const int off = wave_inclusive_scan(mine) - mine;
    for (int w0 = 0; w0 < count; w0 += EMIT_WINDOW) {
        int k = off - w0;  // slot of the lane's next point in this window
#pragma unroll
        for (int i = 0; i < VX; ++i) {
            if (mask[i] & 1) {
                if (k >= 0 && k < EMIT_WINDOW) st[k] = crossing_point<0>(a, x0 + i, y, z, r0.v[i], r0.v[i + 1]);
                ++k;
            }
            if (mask[i] & 2) {
                if (k >= 0 && k < EMIT_WINDOW) st[k] = crossing_point<1>(a, x0 + i, y, z, r0.v[i], ry.v[i]);
                ++k;
            }
            if (mask[i] & 4) {
                if (k >= 0 && k < EMIT_WINDOW) st[k] = crossing_point<2>(a, x0 + i, y, z, r0.v[i], rz.v[i]);
                ++k;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int m = min(EMIT_WINDOW, count - w0);
        for (int t = lane; t < m; t += 64) {
            const long g = (long)begin + w0 + t;
            if (g >= 0 && g < max_points) out[g] = st[t];
        }
        __builtin_amdgcn_wave_barrier();  // the next window / segment overwrites the staging area
    }
}

// Persistent waves over the segments, as mc_emit_kernel: wave w looks at w, w + W, w + 2W, ... (W = waves of the grid);
// lane l reads the offsets of segment w + (64 i + l) W, a ballot finds the ones with points and the wave emits them.
template <int VX>
__global__ __launch_bounds__(256) void extract_emit_kernel(const ExArgs a, const int32_t* __restrict__ seg_off,
                                                           float4* __restrict__ out, int max_points, long nsegs_total) {
    __shared__ float4 stage[4][EMIT_WINDOW];
    const long nwaves = (long)gridDim.x * 4;
    const long w      = (long)blockIdx.x * 4 + threadIdx.y;
    const int lane    = threadIdx.x;
    for (long base = w; base < nsegs_total; base += 64 * nwaves) {
        const long s = base + (long)lane * nwaves;
        int begin = 0, end = 0;
        if (s < nsegs_total) begin = seg_off[s], end = seg_off[s + 1];
        unsigned long long todo = __ballot(end > begin && begin < max_points);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int b = __shfl(begin, l, 64);
            emit_segment<VX>(a, stage[threadIdx.y], base + (long)l * nwaves, b, __shfl(end, l, 64) - b, out, max_points);
        }
    }
}

}  // namespace

hipError_t launch_extract_cloud(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], const float vol2world[12],
                                float* out_points, int max_points, int32_t* total_points, int32_t* seg_off, int32_t* chunk_sums,
                                const uint8_t* occ, hipStream_t s) {
    const bool vec4 = (X % 4 == 0) && (((uintptr_t)vol & 15) == 0);
    const int vx    = vec4 ? 4 : 1;
    ExArgs a;
    a.vol = vol, a.X = X, a.Y = Y, a.Z = Z;
    a.nseg = (X + 64 * vx - 1) / (64 * vx);
    a.vsx = voxel_size[0], a.vsy = voxel_size[1], a.vsz = voxel_size[2];
    for (int i = 0; i < 9; ++i) a.aff.m[i] = vol2world[i];
    for (int i = 0; i < 3; ++i) a.aff.t[i] = vol2world[9 + i];
    const OccDims od = occ_dims(X, Y, Z);
    a.occ = occ, a.ox = od.ox, a.oy = od.oy, a.oz = od.oz;
    const long nsegs = mc_segments(X, Y, Z, vec4);  // (the last slice's segments stay 0)
    // z chunks: >= 2048 workgroups when the volume allows, chunks of at least 16 slices; with a map one layer each
    const long columns = (long)a.nseg * ((Y + 4 * EX_ROWS - 1) / (4 * EX_ROWS));
    int zchunk         = Z;
    while (columns * ((Z + zchunk - 1) / zchunk) < 2048 && zchunk > 16) zchunk = (zchunk + 1) / 2;
    if (occ) zchunk = 8;
    a.zchunk = zchunk;
    hipError_t e = hipMemsetAsync(seg_off, 0, sizeof(int32_t) * (size_t)(nsegs + 1), s);
    if (e != hipSuccess) return e;
    dim3 block(64, 4), grid(a.nseg, (Y + 4 * EX_ROWS - 1) / (4 * EX_ROWS), (Z + zchunk - 1) / zchunk);
    if (vec4) extract_count_kernel<4><<<grid, block, 0, s>>>(a, seg_off);
    else extract_count_kernel<1><<<grid, block, 0, s>>>(a, seg_off);
    launch_segment_scan(seg_off, nsegs, chunk_sums, total_points, s);
    if (out_points && max_points > 0) {
        const unsigned eblocks = (unsigned)std::min<long>((nsegs + 3) / 4, 8192);
        if (vec4) extract_emit_kernel<4><<<eblocks, block, 0, s>>>(a, seg_off, (float4*)out_points, max_points, nsegs);
        else extract_emit_kernel<1><<<eblocks, block, 0, s>>>(a, seg_off, (float4*)out_points, max_points, nsegs);
    }
    return hipGetLastError();
}

}  // namespace dfa
