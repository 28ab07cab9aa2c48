// raycast_device.hpp — the raycaster's device functions (kfusion's TsdfRaycaster, tsdf_volume.cu:128-337) and the
// argument block its launchers fill: shared by the kernels that write the point / depth / normal maps (tsdf.hip) and by
// the one that shades the hit straight into a pixel (render.hip).  One statement of the march; the kernels differ only in
// what they store.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"

namespace dfa {

struct RaycastArgs {
    const uint32_t* vol;
    int X, Y, Z;
    float vsx, vsy, vsz;        // voxel size
    float vix, viy, viz;        // 1 / voxel size          (:362)
    float sx, sy, sz;           // volume size = voxel*dims (:359)
    float gdx, gdy, gdz;        // gradient delta           (:361)
    float time_step;            // trunc * step_factor      (:360)
    Aff3 cam2vol;
    Mat3 Rinv;
    float finvx, finvy, cx, cy;  // Reprojector
    int cols, rows;
};

__device__ __forceinline__ float qnan() { return __uint_as_float(0x7fffffffu); }  // temp_utils.hpp:22

// Work counters of one raycast (dfa_tsdf_raycast_tally, a measurement entry point: SURVEY 8(d) prices the raycast by
// rays x steps x 4 B + hits x 64 x 4 B and by the number of distinct voxels touched).  The product kernels are the
// TALLY = false instantiations: no counter exists in them.
struct RayTally {
    unsigned long long* counts;  // [0] rays that enter the box, [1] nearest-voxel fetches of the march, [2] hits,
                                 // [3] voxel fetches of the trilinear samples (8 per sample inside the volume)
    uint32_t* touched;           // one bit per voxel (X*Y*Z / 32 words, zeroed by the caller) or null
    unsigned int entered, march, hits, tri;
    __device__ __forceinline__ void touch(size_t voxel) const {
        if (touched) atomicOr(&touched[voxel >> 5], 1u << (voxel & 31));
    }
};

// :187-193 nearest voxel (round-half-even).  The clamp is memory safety only: rays are kept
// inside [0, size - voxel] by the slab test.
// IDX32: the volume has at most 2^32 voxels (every BASELINE size; 1024^3 = 2^30): the voxel index is formed in 32-bit
// arithmetic and widened once — 4 vector instructions for the address instead of 12.
template <bool IDX32>
__device__ __forceinline__ size_t voxel_index(const RaycastArgs& a, int x, int y, int z) {
    if constexpr (IDX32) return (size_t)((uint32_t)x + (uint32_t)a.X * ((uint32_t)y + (uint32_t)a.Y * (uint32_t)z));
    else return (size_t)x + (size_t)a.X * y + (size_t)a.X * a.Y * z;
}

template <bool TALLY = false, bool IDX32 = false>
__device__ __forceinline__ float fetch_tsdf(const RaycastArgs& a, f3 p, RayTally* tally = nullptr) {
    int x = (int)rintf(p.x * a.vix);
    int y = (int)rintf(p.y * a.viy);
    int z = (int)rintf(p.z * a.viz);
    x     = min(max(x, 0), a.X - 1);
    y     = min(max(y, 0), a.Y - 1);
    z     = min(max(z, 0), a.Z - 1);
    const size_t voxel = voxel_index<IDX32>(a, x, y, z);
    if constexpr (TALLY) {
        tally->march++;
        tally->touch(voxel);
    }
    return unpack_tsdf(a.vol[voxel]);
}

// :146-171 trilinear interpolation, voxel centres at integer coordinates.  The eight fetches are UNCONDITIONAL (from
// voxel 0 when the sample lies outside the interpolation range, the result then replaced by the reference's NaN): no
// branch separates the samples of a hit, so the two samples of the crossing go out as one batch of 16 fetches and the six
// of the normal as one of 48 — two memory round trips per hit where a branch per sample made eight.
template <bool TALLY = false>
__device__ __forceinline__ float interpolate(const RaycastArgs& a, f3 cf, RayTally* tally = nullptr) {
    const bool inside = cf.x >= 0.f && cf.x < (float)(a.X - 1) && cf.y >= 0.f && cf.y < (float)(a.Y - 1) && cf.z >= 0.f &&
                        cf.z < (float)(a.Z - 1);
    const f3 c = inside ? cf : mk3(0.f, 0.f, 0.f);
    const int gx = (int)c.x, gy = (int)c.y, gz = (int)c.z;  // floor of a non-negative value
    const float fa = c.x - (float)gx, fb = c.y - (float)gy, fc = c.z - (float)gz;
    const size_t sy = (size_t)a.X, sz = (size_t)a.X * a.Y;
    const uint32_t* b = a.vol + (size_t)gx + sy * gy + sz * gz;
    if constexpr (TALLY) {
        if (inside) {
            tally->tri += 8;
            const size_t v0 = (size_t)(b - a.vol);
            for (int c8 = 0; c8 < 8; ++c8) tally->touch(v0 + (c8 & 1) + (c8 & 2 ? sy : 0) + (c8 & 4 ? sz : 0));
        }
    }
    const float v000 = unpack_tsdf(b[0]), v001 = unpack_tsdf(b[sz]);
    const float v010 = unpack_tsdf(b[sy]), v011 = unpack_tsdf(b[sy + sz]);
    const float v100 = unpack_tsdf(b[1]), v101 = unpack_tsdf(b[1 + sz]);
    const float v110 = unpack_tsdf(b[1 + sy]), v111 = unpack_tsdf(b[1 + sy + sz]);
    float tsdf = 0.f;
    tsdf = fmaf((v000 * (1.f - fa)) * (1.f - fb), (1.f - fc), tsdf);
    tsdf = fmaf((v001 * (1.f - fa)) * (1.f - fb), fc, tsdf);
    tsdf = fmaf((v010 * (1.f - fa)) * fb, (1.f - fc), tsdf);
    tsdf = fmaf((v011 * (1.f - fa)) * fb, fc, tsdf);
    tsdf = fmaf((v100 * fa) * (1.f - fb), (1.f - fc), tsdf);
    tsdf = fmaf((v101 * fa) * (1.f - fb), fc, tsdf);
    tsdf = fmaf((v110 * fa) * fb, (1.f - fc), tsdf);
    tsdf = fmaf((v111 * fa) * fb, fc, tsdf);
    return inside ? tsdf : qnan();
}

// :320-336 before the normalisation: central differences of the interpolant, each divided by its delta (the raycaster's
// __fdividef as the correctly rounded divide); also ExtractNormals :625-660
template <bool TALLY = false>
__device__ __forceinline__ f3 tsdf_gradient(const RaycastArgs& a, f3 p, RayTally* tally = nullptr) {
    const f3 vi = mk3(a.vix, a.viy, a.viz);
    f3 n;
    const float Fx1 = interpolate<TALLY>(a, mk3(p.x + a.gdx, p.y, p.z) * vi, tally);
    const float Fx2 = interpolate<TALLY>(a, mk3(p.x - a.gdx, p.y, p.z) * vi, tally);
    n.x             = (Fx1 - Fx2) / a.gdx;
    const float Fy1 = interpolate<TALLY>(a, mk3(p.x, p.y + a.gdy, p.z) * vi, tally);
    const float Fy2 = interpolate<TALLY>(a, mk3(p.x, p.y - a.gdy, p.z) * vi, tally);
    n.y             = (Fy1 - Fy2) / a.gdy;
    const float Fz1 = interpolate<TALLY>(a, mk3(p.x, p.y, p.z + a.gdz) * vi, tally);
    const float Fz2 = interpolate<TALLY>(a, mk3(p.x, p.y, p.z - a.gdz) * vi, tally);
    n.z             = (Fz1 - Fz2) / a.gdz;
    return n;
}

// :320-336
template <bool TALLY = false>
__device__ __forceinline__ f3 compute_normal(const RaycastArgs& a, f3 p, RayTally* tally = nullptr) {
    return normalized(tsdf_gradient<TALLY>(a, p, tally));
}

// march steps whose voxels are requested together (measured at 512^3 / VGA and 1024^3 / 720p: 1 step 0.082 / 0.219 ms,
// 2: 0.063 / 0.158, 4: 0.057 / 0.140, 6: 0.060 / 0.143, 8: 0.062 / 0.148 in the first batched form)
constexpr int RAY_BATCH = 4;

// shared body of the two TsdfRaycaster::operator() overloads (:195-318)
template <bool TALLY = false, bool IDX32 = false>
__device__ __forceinline__ bool cast_ray(const RaycastArgs& a, int x, int y, f3& vertex_cam, f3& normal_cam,
                                         RayTally* tally = nullptr) {
    const f3 ray_org = mk3(a.cam2vol.t[0], a.cam2vol.t[1], a.cam2vol.t[2]);
    const f3 pix     = mk3((1.f * ((float)x - a.cx)) * a.finvx, (1.f * ((float)y - a.cy)) * a.finvy, 1.f);
    const f3 ray_dir = normalized(mulR(a.cam2vol, pix));
    const f3 box_max = mk3(a.sx - a.vsx, a.sy - a.vsy, a.sz - a.vsz);  // :213
    // intersect (:128-144), including the reference's asymmetric max/min
    const f3 invR = mk3(1.f / ray_dir.x, 1.f / ray_dir.y, 1.f / ray_dir.z);
    const f3 tbot = invR * (mk3(0.f, 0.f, 0.f) - ray_org);
    const f3 ttop = invR * (box_max - ray_org);
    const f3 tmn  = mk3(fminf(ttop.x, tbot.x), fminf(ttop.y, tbot.y), fminf(ttop.z, tbot.z));
    const f3 tmx  = mk3(fmaxf(ttop.x, tbot.x), fmaxf(ttop.y, tbot.y), fmaxf(ttop.z, tbot.z));
    float tmin    = fmaxf(fmaxf(tmn.x, tmn.y), fmaxf(tmn.x, tmn.z));
    float tmax    = fminf(fminf(tmx.x, tmx.y), fminf(tmx.x, tmx.z));
    tmin          = fmaxf(0.f, tmin);  // :219
    if (!(tmin < tmax)) return false;  // :220
    if constexpr (TALLY) tally->entered++;
    tmax -= a.time_step;
    const f3 vstep  = ray_dir * a.time_step;
    f3 next         = ray_org + ray_dir * tmin;
    float tsdf_next = fetch_tsdf<TALLY, IDX32>(a, next, tally);
    const f3 vi     = mk3(a.vix, a.viy, a.viz);
    // The march (:222-256) in batches of RAY_BATCH steps: the positions of the next RAY_BATCH samples — the same running
    // `next += vstep` additions — are computed and their voxels requested TOGETHER (a memory round trip per batch instead
    // of per step), as are the running `tcurr += time_step` sums.  Whether ANY of the batch's steps ends the march — the
    // reference's two sign tests (:234, :237) or its loop condition — takes a few compares; only a batch that holds an
    // event is then walked step by step, in the reference's order, to find the first one.  The fetches behind the exit
    // are speculative (clamped addresses, at most RAY_BATCH - 1 per ray) and their values unused.
    bool hit = false;
    f3 hit_curr = next, hit_next = next;
    float hit_t = 0.f;
    if (!(tmin < tmax)) return false;  // the loop condition before the first step
    for (float tcurr = tmin;;) {
        f3 pos[RAY_BATCH];
        float val[RAY_BATCH], tc[RAY_BATCH + 1];
        pos[0] = next + vstep;
        tc[0]  = tcurr;
#pragma unroll
        for (int j = 1; j < RAY_BATCH; ++j) pos[j] = pos[j - 1] + vstep;
#pragma unroll
        for (int j = 0; j < RAY_BATCH; ++j) tc[j + 1] = tc[j] + a.time_step;
#pragma unroll
        for (int j = 0; j < RAY_BATCH; ++j) val[j] = fetch_tsdf<false, IDX32>(a, pos[j]);  // (tallied below, per step taken)
        bool event = false;
#pragma unroll
        for (int j = 0; j < RAY_BATCH; ++j) {
            const float c = j ? val[j - 1] : tsdf_next, n = val[j];
            event |= (c < 0.f && n > 0.f) || (c > 0.f && n < 0.f) || !(tc[j + 1] < tmax);
        }
        if (event) {
#pragma unroll
            for (int j = 0; j < RAY_BATCH; ++j) {
                const float c = j ? val[j - 1] : tsdf_next, n = val[j];
                if constexpr (TALLY) (void)fetch_tsdf<true, IDX32>(a, pos[j], tally);
                if (c < 0.f && n > 0.f) break;  // :234
                if (c > 0.f && n < 0.f) {       // :237
                    hit      = true;
                    hit_curr = j ? pos[j - 1] : next, hit_next = pos[j], hit_t = tc[j];
                    break;
                }
                if (!(tc[j + 1] < tmax)) break;  // the loop condition
            }
            break;
        }
        if constexpr (TALLY)
            for (int j = 0; j < RAY_BATCH; ++j) (void)fetch_tsdf<true, IDX32>(a, pos[j], tally);
        next = pos[RAY_BATCH - 1], tsdf_next = val[RAY_BATCH - 1], tcurr = tc[RAY_BATCH];
    }
    if (hit) {
        const float Ft   = interpolate<TALLY>(a, hit_curr * vi, tally);
        const float Ftdt = interpolate<TALLY>(a, hit_next * vi, tally);
        const float Ts   = hit_t - (a.time_step * Ft) / (Ftdt - Ft);  // :241
        const f3 vertex  = ray_org + ray_dir * Ts;
        const f3 normal  = compute_normal<TALLY>(a, vertex, tally);
        const float prod = normal.x * normal.y * normal.z;
        if (prod == prod) {  // :246 !isnan
            if constexpr (TALLY) tally->hits++;
            normal_cam = mul(a.Rinv, normal);
            vertex_cam = mul(a.Rinv, vertex - ray_org);
            return true;
        }
    }
    return false;
}

// A wave covers an 8x8 pixel tile (rays of a tile walk neighbouring voxels -> shared cache lines); a 256-thread block
// covers 16x16 pixels.  Workgroups are dealt round-robin to the 8 XCDs, each with an L2 of its own: within every round of
// 64 tiles XCD i takes 8 CONSECUTIVE tiles — neighbours along x share their 64-byte voxel lines (16 voxels = ~32 pixels
// at 1.5 m and 512^3), so the line is fetched into one L2 instead of two to eight (HBM fetch 107 -> 69 MB per VGA launch
// at 512^3, L2 hit rate 21 -> 48 %, 0.051 -> 0.042 ms; contiguous bands per XCD fetch even less — 50 MB — but leave the XCDs
// with unequal work: slower).  The last, partial round keeps the identity order.
constexpr int RAY_XCD_GROUP = 8;
__device__ __forceinline__ void tile_pixel(int& x, int& y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = gridDim.x * gridDim.y, b = blockIdx.y * gridDim.x + blockIdx.x;
    const int full = nb / (8 * RAY_XCD_GROUP) * (8 * RAY_XCD_GROUP);
    int t = b;
    if (b < full) {
        const int round = b / (8 * RAY_XCD_GROUP), r = b % (8 * RAY_XCD_GROUP);
        t = round * 8 * RAY_XCD_GROUP + (r & 7) * RAY_XCD_GROUP + (r >> 3);
    }
    const int bx = t % gridDim.x, by = t / gridDim.x;
    x = bx * 16 + (wave & 1) * 8 + (lane & 7);
    y = by * 16 + (wave >> 1) * 8 + (lane >> 3);
}

// the launchers' argument block (host)
inline RaycastArgs make_raycast_args(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3],
                                     float trunc_dist, const float cam2vol[12], const float Rinv[9], float fx,
                                     float fy, float cx, float cy, float step_factor, float delta_factor, int cols,
                                     int rows) {
    RaycastArgs a;
    a.vol = vol, a.X = X, a.Y = Y, a.Z = Z;
    a.vsx = voxel_size[0], a.vsy = voxel_size[1], a.vsz = voxel_size[2];
    // tsdf_volume.cu:359-362 (host, plain float arithmetic)
    a.sx = voxel_size[0] * (float)X, a.sy = voxel_size[1] * (float)Y, a.sz = voxel_size[2] * (float)Z;
    a.time_step = trunc_dist * step_factor;
    a.gdx = voxel_size[0] * delta_factor, a.gdy = voxel_size[1] * delta_factor, a.gdz = voxel_size[2] * delta_factor;
    a.vix = 1.f / voxel_size[0], a.viy = 1.f / voxel_size[1], a.viz = 1.f / voxel_size[2];
    for (int i = 0; i < 9; ++i) a.cam2vol.m[i] = cam2vol[i], a.Rinv.m[i] = Rinv[i];
    for (int i = 0; i < 3; ++i) a.cam2vol.t[i] = cam2vol[9 + i];
    a.finvx = 1.f / fx, a.finvy = 1.f / fy, a.cx = cx, a.cy = cy;
    a.cols = cols, a.rows = rows;
    return a;
}

}  // namespace dfa
