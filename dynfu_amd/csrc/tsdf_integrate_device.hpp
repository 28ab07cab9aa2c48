// tsdf_integrate_device.hpp — the per-voxel TSDF update of tsdf_volume.cu:65-91, shared by the sweeps of tsdf.hip (voxel
// positions by the reference's running addition) and the warped sweeps of tsdf_warped.hip (warped_sweep_device.hpp: voxel positions through the
// warp field): the argument block, the projector's divisions, the distance of one voxel and its running average.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"

namespace dfa {

// integrate — tsdf_volume.cu:43-96
struct IntegrateArgs {
    const uint16_t* dists;
    int dists_step, cols, rows;
    uint32_t* vol;
    int X, Y, Z;
    float vsx, vsy, vsz;
    float trunc, trunc_inv;
    int max_weight;
    Aff3 vol2cam;
    float fx, fy, cx, cy;
    int zchunk;
    uint8_t* occ;  // occupancy map (kernels.hpp: OccDims) or null
    int ox, oy;
    int occ_known;  // fused sweep: the map describes the volume as it is NOW — a box without weights that gets none is not written
};

// x / z and y / z, correctly rounded.  hipcc expands an fp32 division into
//   s0 = div_scale(den), s1 = div_scale(num), r = rcp(s0), e = fma(-s0, r, 1), r1 = fma(e, r, r), q = s1 * r1,
//   e2 = fma(-s0, q, s1), q1 = fma(e2, r1, q), e3 = fma(-s0, q1, s1), div_fixup(div_fmas(e3, r1, q1))
// (11 instructions; div_scale / div_fmas / div_fixup only act on operands near the ends of the exponent range).  For
// operands well inside the range the two quotients share everything that depends on z alone — the same instructions
// on the same values, hence the same bits, in 13 instead of 22; anything else takes the plain divisions.
__device__ __forceinline__ void div_xy_by_z(float x, float y, float z, float& qx, float& qy) {
    const float big = fmaxf(fmaxf(fabsf(x), fabsf(y)), z);
    if (big <= 1048576.f && z >= 9.5367431640625e-07f) {  // 2^20, 2^-20 (z > 0 here)
        const float r  = __builtin_amdgcn_rcpf(z);
        const float r1 = fmaf(fmaf(-z, r, 1.0f), r, r);
        float q        = x * r1;
        q              = fmaf(fmaf(-z, q, x), r1, q);
        qx             = fmaf(fmaf(-z, q, x), r1, q);
        q              = y * r1;
        q              = fmaf(fmaf(-z, q, y), r1, q);
        qy             = fmaf(fmaf(-z, q, y), r1, q);
    } else {
        qx = x / z, qy = y / z;
    }
}

// One voxel of one slice, first half (tsdf_volume.cu:65-80): false when the reference leaves the voxel alone, else the
// truncated signed distance of this frame.
__device__ __forceinline__ bool voxel_tsdf(const IntegrateArgs& a, f3 vc, float& tsdf) {
    // :74 `vc.z <= 0` is tested first here: the reference tests it after the (side-effect
    // free) projection and texture fetch, the outcome is the same and NaN/inf never form.
    if (!(vc.z > 0.f)) return false;
    // Projector (device.hpp:40-45): correctly rounded divisions stand in for __fdividef
    float qx, qy;
    div_xy_by_z(vc.x, vc.y, vc.z, qx, qy);
    const float coox = fmaf(a.fx, qx, a.cx);
    const float cooy = fmaf(a.fy, qy, a.cy);
    if (!(coox >= 0.f && cooy >= 0.f && coox < (float)a.cols && cooy < (float)a.rows)) return false;  // :70
    // :73 point-sampled, un-normalised texture fetch == texel (floor x, floor y); coordinates
    // are non-negative here so the truncating convert is the floor
    const int px         = (int)coox;
    const int py         = (int)cooy;
    const uint16_t* drow = (const uint16_t*)((const char*)a.dists + (size_t)py * a.dists_step);
    const float Dp       = half_bits_to_float(drow[px]);
    if (Dp == 0.f) return false;                    // :74
    // Voxels far behind the surface (a third of the volume) leave before the correctly rounded square root: when
    // |vc|^2 exceeds (Dp + trunc)^2 by more than 1e-5 relative, sqrt exceeds Dp + trunc by 5e-6 relative — two orders
    // above the rounding of the three operations below, so the test of :79 fails for certain.
    const float d2  = dot(vc, vc);
    const float lim = Dp + a.trunc;
    if (d2 > lim * lim * 1.00001f) return false;
    const float sdf = Dp - sqrtf(d2);               // :77
    if (!(sdf >= -a.trunc)) return false;           // :79
    tsdf = fminf(1.f, sdf * a.trunc_inv);           // :80
    return true;
}

// second half (:82-90): running average with the voxel's previous state (`old` packed; 0 when the clear is fused)
template <bool FUSED_CLEAR>
__device__ __forceinline__ uint32_t voxel_update(const IntegrateArgs& a, uint32_t old, float tsdf) {
    int weight_prev;
    float tsdf_prev;
    if (FUSED_CLEAR) {
        weight_prev = 0;
        tsdf_prev   = 0.f;
    } else {
        weight_prev = (int)(old >> 16);
        tsdf_prev   = unpack_tsdf(old);
    }
    const float tsdf_new = fmaf(tsdf_prev, (float)weight_prev, tsdf) / (float)(weight_prev + 1);  // :86
    const int weight_new = min(weight_prev + 1, a.max_weight);                                   // :87
    return pack_tsdf(tsdf_new, weight_new);
}

}  // namespace dfa
