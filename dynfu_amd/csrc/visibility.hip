// visibility.hip — which vertices of a cloud the camera can see, against a point map of the model's visible surface
// (dfa_visible_vertices; the map is dfa_mesh_rasterize's or dfa_tsdf_raycast_points': float4 pixels in the camera frame,
// quiet NaN where nothing is seen).  No reference counterpart: DynamicFusion's data term sums over the visible points of
// the warped model, the reference's solve takes every canonical vertex.
//
// One lane per vertex (x, y, z) in the camera frame, float32, in this order (tests/visibility_statement.py states the same):
//   1. x, y or z not finite, or z <= 0:                      flag 0
//   2. qx = x / z, qy = y / z                                 correctly rounded divisions (div_xy_by_z)
//   3. u = fmaf(fx, qx, cx), v = fmaf(fy, qy, cy)
//   4. ru = rintf(u), rv = rintf(v) (ties to even); unless 0 <= ru <= cols - 1 and 0 <= rv <= rows - 1, compared as
//      floats (a NaN fails):                                  flag 0
//   5. M = model_points[rv][ru]; M.x is NaN:                  flag 1   (nothing of the model covers the pixel)
//   6. otherwise                                              flag = z <= M.z + z_tol   (one addition, one comparison)
// The count of set flags: every workgroup leaves its own, a second launch of one workgroup adds them (integers: the same
// number in every run).
#include "kernels.hpp"
#include "tsdf_integrate_device.hpp"  // div_xy_by_z

namespace dfa {

namespace {

__global__ void __launch_bounds__(256) visible_vertices_kernel(const float* __restrict__ vertices, int stride, int n,
                                                               const float* __restrict__ model_points, int points_step,
                                                               int cols, int rows, float fx, float fy, float cx, float cy,
                                                               float z_tol, uint8_t* __restrict__ flags,
                                                               int32_t* __restrict__ partial /* per workgroup, or null */) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool vis       = false;
    if (i < (size_t)n) {
        float x, y, z;
        if (stride == 4 && (reinterpret_cast<uintptr_t>(vertices) & 15) == 0) {  // (uniform) one 16-byte load
            const float4 p = reinterpret_cast<const float4*>(vertices)[i];
            x = p.x, y = p.y, z = p.z;
        } else {
            const float* p = vertices + i * (size_t)stride;
            x = p[0], y = p[1], z = p[2];
        }
        if (isfinite(x) && isfinite(y) && isfinite(z) && z > 0.f) {  // 1.
            float qx, qy;
            div_xy_by_z(x, y, z, qx, qy);                              // 2.
            const float u = fmaf(fx, qx, cx), v = fmaf(fy, qy, cy);   // 3.
            const float ru = rintf(u), rv = rintf(v);                 // 4.
            if (ru >= 0.f && ru <= (float)(cols - 1) && rv >= 0.f && rv <= (float)(rows - 1)) {
                const float* M = reinterpret_cast<const float*>(reinterpret_cast<const char*>(model_points) +
                                                                (size_t)(int)rv * (size_t)points_step) + 4 * (size_t)(int)ru;
                const float mx = M[0], mz = M[2];
                vis = mx != mx || z <= mz + z_tol;                    // 5., 6.
            }
        }
        flags[i] = vis ? 1 : 0;
    }
    if (!partial) return;  // (uniform)
    __shared__ int wave_count[4];
    const int c = __popcll(__ballot(vis));
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

// one workgroup: the workgroups' counts added up
__global__ void __launch_bounds__(256) visible_count_kernel(const int32_t* __restrict__ partial, int blocks, int32_t* __restrict__ count) {
    __shared__ int wave_sum[4];
    int c = 0;
    for (int b = threadIdx.x; b < blocks; b += 256) c += partial[b];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) *count = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

}  // namespace

int visible_blocks(int n) { return (int)(((long)n + 255) / 256); }

hipError_t launch_visible_vertices(const float* vertices, int stride, int n, const float* model_points, int points_step, int cols,
                                   int rows, float fx, float fy, float cx, float cy, float z_tol, uint8_t* flags, int32_t* count,
                                   int32_t* partial, hipStream_t s) {
    if (n <= 0) return count ? hipMemsetAsync(count, 0, sizeof(int32_t), s) : hipSuccess;
    const int blocks = visible_blocks(n);
    visible_vertices_kernel<<<blocks, 256, 0, s>>>(vertices, stride, n, model_points, points_step, cols, rows, fx, fy, cx, cy, z_tol,
                                                  flags, count ? partial : nullptr);
    if (count) visible_count_kernel<<<1, 256, 0, s>>>(partial, blocks, count);
    return hipGetLastError();
}

}  // namespace dfa
