// render.hip — gfx950 kernels that turn the model maps into an image one can look at: the Phong view of a point or
// depth map, the normal colours, and the raycast fused with either.
//
// What they compute is kfusion's src/kfusion/cuda/imgproc.cu:363-514 (cited per kernel).  The output pixel is the
// reference's RGB (types.hpp): four bytes b, g, r, 0 — one dword store per pixel.
//
// Arithmetic (device_math.hpp: -ffp-contract=off, an fma only inside dot()).  The result is reproducible byte for byte
// from tests/render_statement.py, so the three CUDA intrinsics of the reference are fixed IEEE sequences here:
//   * __powf(x, 20.f)             -> five multiplications: x2 = x x, x4 = x2 x2, x5 = x4 x, x10 = x5 x5, x20 = x10 x10;
//   * normalized                  -> device_math.hpp's v * (1 / sqrt(dot(v, v)));
//   * uchar(__saturatef(c) * 255) -> NaN -> 0, clamp to [0, 1], multiply, truncate;
//   * the normal colours' uchar((5 - n k) * 25.5) has no clamp in the reference and is undefined in C++ for NaN (every
//     missed pixel of a raycast normal map) and outside [0, 256): here NaN -> 0, else clamp to [0, 255], truncate — what
//     the CUDA conversion yields for NaN, and unit normals stay inside 38 ... 216 anyway;
//   * fmax(0, d) is `d > 0 ? d : 0`: 0 for NaN, as fmax gives.
//
// Layout: a wave covers a 64-pixel row segment (block 64 x 4), so its two float4 loads are 1 KiB contiguous each and its
// pixel store 256 B contiguous; no LDS, no atomics.  The shade kernels are pure streaming (32 or 18 B in, 4 B out per
// pixel).  The fused kernel keeps the raycaster's 8 x 8 tile per wave (raycast_device.hpp): its time is the march's.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"
#include "raycast_device.hpp"

namespace dfa {

__device__ __forceinline__ float max0(float v) { return v > 0.f ? v : 0.f; }  // fmax(0.f, v): 0 for NaN

// uchar(__saturatef(c) * 255.f)
__device__ __forceinline__ uint32_t unit_to_byte(float c) {
    const float s = c > 0.f ? (c < 1.f ? c : 1.f) : 0.f;  // NaN -> 0
    return (uint32_t)(int)(s * 255.f);
}

// uchar(v) of the normal colours: NaN -> 0, clamp to [0, 255], truncate
__device__ __forceinline__ uint32_t clamp_to_byte(float v) {
    const float s = v > 0.f ? (v < 255.f ? v : 255.f) : 0.f;
    return (uint32_t)(int)s;
}

__device__ __forceinline__ uint32_t pack_bgr(uint32_t b, uint32_t g, uint32_t r) { return b | (g << 8) | (r << 16); }

// imgproc.cu:376-380 / :426-430 — the background of a pixel without a surface: bgr1 (1 - w) + bgr2 w down the image
__device__ __forceinline__ uint32_t background_pixel(int y, int rows) {
    const float w  = (float)y / (float)rows;
    const float w1 = 1.f - w;
    const float b  = (4.f / 255.f) * w1 + (236.f / 255.f) * w;
    const float g  = (2.f / 255.f) * w1 + (120.f / 255.f) * w;
    return pack_bgr(unit_to_byte(b), unit_to_byte(g), unit_to_byte(g));  // (bgr1.y == bgr1.z, bgr2.y == bgr2.z)
}

// imgproc.cu:385-402 / :435-452 — Ix = Ka + Kd max(0, N.L) + Ks max(0, R.V)^20, every colour 1; the camera sits at the origin
__device__ __forceinline__ uint32_t phong_pixel(f3 P, f3 N, f3 light) {
    const f3 L      = normalized(light - P);
    const f3 V      = normalized(mk3(0.f, 0.f, 0.f) - P);
    const float nl  = dot(N, L);
    const f3 R      = normalized((N * 2.f) * nl - L);
    const float x   = max0(dot(R, V));
    const float x2  = x * x;
    const float x4  = x2 * x2;
    const float x5  = x4 * x;
    const float x10 = x5 * x5;
    const float x20 = x10 * x10;
    const float Ix  = (0.3f + 0.5f * max0(nl)) + 0.2f * x20;
    const uint32_t c = unit_to_byte(Ix);
    return pack_bgr(c, c, c);
}

// imgproc.cu:499-503 (the `#else` branch): colours(y, x) = (b, g, r, 0)
__device__ __forceinline__ uint32_t tangent_pixel(float nx, float ny, float nz) {
    const uint32_t r = clamp_to_byte((5.f - nx * 3.5f) * 25.5f);
    const uint32_t g = clamp_to_byte((5.f - ny * 2.5f) * 25.5f);
    const uint32_t b = clamp_to_byte((5.f - nz * 3.5f) * 25.5f);
    return pack_bgr(b, g, r);
}

__device__ __forceinline__ const float4* row4(const float* img, int step, int y) {
    return (const float4*)((const char*)img + (size_t)y * step);
}
__device__ __forceinline__ uint32_t* pixel_row(uint8_t* img, int step, int y) { return (uint32_t*)(img + (size_t)y * step); }

// ------------------------------------------------------------------------------------------
// Phong view of a point map — render_image_kernel(PtrStep<Point>, ...), imgproc.cu:413-461.  block (64, 4)
__global__ __launch_bounds__(256) void render_points_kernel(const float* __restrict__ points, int points_step,
                                                            const float* __restrict__ normals, int normals_step, int cols,
                                                            int rows, f3 light, uint8_t* __restrict__ image, int image_step) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const float4 p = row4(points, points_step, y)[x];
    const float4 n = row4(normals, normals_step, y)[x];
    pixel_row(image, image_step, y)[x] =
        p.x != p.x ? background_pixel(y, rows) : phong_pixel(mk3(p.x, p.y, p.z), mk3(n.x, n.y, n.z), light);
}

// Phong view of a depth map — render_image_kernel(PtrStep<ushort>, ...), imgproc.cu:363-411
__global__ __launch_bounds__(256) void render_depth_kernel(const uint16_t* __restrict__ depth, int depth_step,
                                                           const float* __restrict__ normals, int normals_step, int cols,
                                                           int rows, float finvx, float finvy, float cx, float cy, f3 light,
                                                           uint8_t* __restrict__ image, int image_step) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const int d    = ((const uint16_t*)((const char*)depth + (size_t)y * depth_step))[x];
    const float4 n = row4(normals, normals_step, y)[x];
    uint32_t px;
    if (d == 0) px = background_pixel(y, rows);
    else {
        const float z = (float)d * 0.001f;  // Reprojector (device.hpp:50-54)
        const f3 P    = mk3((z * ((float)x - cx)) * finvx, (z * ((float)y - cy)) * finvy, z);
        px            = phong_pixel(P, mk3(n.x, n.y, n.z), light);
    }
    pixel_row(image, image_step, y)[x] = px;
}

// normal colours — tangent_colors_kernel, imgproc.cu:485-504
__global__ __launch_bounds__(256) void tangent_colors_kernel(const float* __restrict__ normals, int normals_step, int cols,
                                                             int rows, uint8_t* __restrict__ image, int image_step) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const float4 n = row4(normals, normals_step, y)[x];
    pixel_row(image, image_step, y)[x] = tangent_pixel(n.x, n.y, n.z);
}

// ------------------------------------------------------------------------------------------
// raycast + shade: the rays of raycast_points_kernel (tsdf.hip), pixel for pixel and bit for bit — the same cast_ray, the
// same 8 x 8 tile per wave and the same order of the tiles over the XCDs — with the hit shaded in registers instead of
// stored as two float4 (KinFu::renderImage(image, pose, flag), kinfu.cpp:289-316, raycasts into maps it then throws away).
// MODE as dfa_render_mode: 0 Phong, 1 normal colours, 2 both, the normal colours `cols` pixels to the right.
template <bool IDX32>
__global__ __launch_bounds__(256) void raycast_render_kernel(const RaycastArgs a, f3 light, int mode,
                                                             uint8_t* __restrict__ image, int image_step) {
    int x, y;
    tile_pixel(x, y);
    if (x >= a.cols || y >= a.rows) return;
    f3 v, n;
    const bool hit = cast_ray<false, IDX32>(a, x, y, v, n);
    uint32_t* row  = pixel_row(image, image_step, y);
    if (mode != 1) row[x] = hit ? phong_pixel(v, n, light) : background_pixel(y, a.rows);
    if (mode != 0) row[mode == 2 ? x + a.cols : x] = hit ? tangent_pixel(n.x, n.y, n.z) : 0u;  // (a miss is a NaN normal)
}

// ------------------------------------------------------------------------------------------
static inline dim3 row_grid(int cols, int rows) { return dim3((cols + 63) / 64, (rows + 3) / 4); }

hipError_t launch_render_points(const float* points, int points_step, const float* normals, int normals_step, int cols,
                                int rows, const float light[3], uint8_t* image, int image_step, hipStream_t s) {
    render_points_kernel<<<row_grid(cols, rows), dim3(64, 4), 0, s>>>(points, points_step, normals, normals_step, cols, rows,
                                                                      f3{light[0], light[1], light[2]}, image, image_step);
    return hipGetLastError();
}

hipError_t launch_render_depth(const uint16_t* depth, int depth_step, const float* normals, int normals_step, int cols,
                               int rows, float fx, float fy, float cx, float cy, const float light[3], uint8_t* image,
                               int image_step, hipStream_t s) {
    render_depth_kernel<<<row_grid(cols, rows), dim3(64, 4), 0, s>>>(depth, depth_step, normals, normals_step, cols, rows,
                                                                     1.f / fx, 1.f / fy, cx, cy,
                                                                     f3{light[0], light[1], light[2]}, image, image_step);
    return hipGetLastError();
}

hipError_t launch_tangent_colors(const float* normals, int normals_step, int cols, int rows, uint8_t* image, int image_step,
                                 hipStream_t s) {
    tangent_colors_kernel<<<row_grid(cols, rows), dim3(64, 4), 0, s>>>(normals, normals_step, cols, rows, image, image_step);
    return hipGetLastError();
}

hipError_t launch_raycast_render(const uint32_t* vol, int X, int Y, int Z, const float voxel_size[3], float trunc_dist,
                                 const float cam2vol[12], const float Rinv[9], float fx, float fy, float cx, float cy,
                                 float step_factor, float delta_factor, int cols, int rows, const float light[3], int mode,
                                 uint8_t* image, int image_step, hipStream_t s) {
    RaycastArgs a = make_raycast_args(vol, X, Y, Z, voxel_size, trunc_dist, cam2vol, Rinv, fx, fy, cx, cy, step_factor,
                                      delta_factor, cols, rows);
    const f3 l = f3{light[0], light[1], light[2]};
    dim3 block(256), grid((cols + 15) / 16, (rows + 15) / 16);
    if ((uint64_t)X * Y * Z <= (1ull << 32)) raycast_render_kernel<true><<<grid, block, 0, s>>>(a, l, mode, image, image_step);
    else raycast_render_kernel<false><<<grid, block, 0, s>>>(a, l, mode, image, image_step);
    return hipGetLastError();
}

}  // namespace dfa
