// icp.hip — one linearisation of the reference's rigid projective ICP for gfx950:
// ComputeIcpHelper::find_coresp + the row [s x n, n | n.(d - s)] + its 27 products summed over the image
// (src/kfusion/cuda/proj_icp.cu:41-103 depth / points variants, :326-375; textures point-sampled :377-379).
// The 6x6 solve and the pose update stay on the host as in the reference (src/kfusion/projective_icp.cpp:118-150).
//
// One lane per pixel of the current frame; the 27 products are reduced per wave with DPP adds and per
// workgroup through LDS (the reference tree-reduces 27 times through shared memory with 5 barriers each), one
// partial per workgroup and product; a second launch adds the partials in index order in double precision.
//
// rigid_rows_cloud_kernel (dfa_rigid_sums_cloud; no reference counterpart) is the same linearisation over a CLOUD against
// the live maps: one lane per vertex, the pixel rule and the gates of the north-star solve's data term
// (solve6_linearise.hip), the same reduction and the same closing launch.
//
// rigid_loop_rows_kernel / rigid_loop_step_kernel (dfa_rigid_align_cloud) run that linearisation's whole Gauss-Newton loop
// without the host: the same row over every step-th vertex at a pose kept on the device, then one workgroup that adds the
// 27 sums in the closing launch's order and runs the 6x6 step and the loop's rules (rigid_step.hpp) in one lane.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/dynfu_amd.h"
#include "device_math.hpp"
#include "kernels.hpp"
#include "rigid_step.hpp"

namespace dfa {

namespace {

struct IcpArgs {
    const void* curr;   // u16 depth or float4 vertex map of the current frame
    const float* ncurr;
    const void* prev;
    const float* nprev;
    int curr_step, ncurr_step, prev_step, nprev_step, cols, rows;
    Aff3 aff;
    float fx, fy, cx, cy, finvx, finvy, min_cosine, dist2_thres;
};

template <class T>
__device__ __forceinline__ const T& at(const void* base, int step, int y, int x) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (size_t)y * step + sizeof(T) * (size_t)x);
}

template <bool DEPTH>
__device__ __forceinline__ bool find_coresp(const IcpArgs& a, int x, int y, f3& n, f3& d, f3& s) {
    f3 p;
    if (DEPTH) {
        const int src_z = at<uint16_t>(a.curr, a.curr_step, y, x);
        if (src_z == 0) return false;  // :44-46
        const float z = src_z * 0.001f;
        p = mk3(z * ((float)x - a.cx) * a.finvx, z * ((float)y - a.cy) * a.finvy, z);  // reproj :35-39
    } else {
        const float4 v = at<float4>(a.curr, a.curr_step, y, x);
        if (v.x != v.x) return false;  // :75-77
        p = mk3(v.x, v.y, v.z);
    }
    s = mulR(a.aff, p) + mk3(a.aff.t[0], a.aff.t[1], a.aff.t[2]);
    const float u = fmaf(a.fx, s.x / s.z, a.cx), w = fmaf(a.fy, s.y / s.z, a.cy);  // proj :28-33
    if (s.z <= 0.f || u < 0.f || w < 0.f || u >= (float)a.cols || w >= (float)a.rows) return false;
    const int iu = (int)floorf(u), iw = (int)floorf(w);  // point-sampled texture fetch
    if (DEPTH) {
        const int dst_z = at<uint16_t>(a.prev, a.prev_step, iw, iu);
        if (dst_z == 0) return false;
        const float z = dst_z * 0.001f;
        d = mk3(z * (u - a.cx) * a.finvx, z * (w - a.cy) * a.finvy, z);  // :57: reproj at the float coordinates
    } else {
        const float4 v = at<float4>(a.prev, a.prev_step, iw, iu);
        if (v.x != v.x) return false;
        d = mk3(v.x, v.y, v.z);
    }
    const f3 sd = s - d;
    if (dot(sd, sd) > a.dist2_thres) return false;  // :59-61
    const float4 nc = at<float4>(a.ncurr, a.ncurr_step, y, x);
    const f3 ns     = mulR(a.aff, mk3(nc.x, nc.y, nc.z));
    const float4 np = at<float4>(a.nprev, a.nprev_step, iw, iu);
    n               = mk3(np.x, np.y, np.z);
    return !(fabsf(dot(ns, n)) < a.min_cosine);  // :66-68
}

template <bool DEPTH>
__global__ __launch_bounds__(256) void icp_rows_kernel(const IcpArgs a, float* __restrict__ partial, int nblocks,
                                                       unsigned int* __restrict__ matched) {
    __shared__ float sh[4][28];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    float row[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f3 n, d, s;
    const bool ok = x < a.cols && y < a.rows && find_coresp<DEPTH>(a, x, y, n, d, s);
    if (ok) {  // :333-337
        row[0] = s.y * n.z - s.z * n.y, row[1] = s.z * n.x - s.x * n.z, row[2] = s.x * n.y - s.y * n.x;
        row[3] = n.x, row[4] = n.y, row[5] = n.z;
        row[6] = dot(n, d - s);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 7; ++j) {
            const float t = wave_total(row[i] * row[j]);
            if (lane == 0) sh[wave][q] = t;
            ++q;
        }
    const float cnt = wave_total(ok ? 1.f : 0.f);
    if (lane == 0) sh[wave][27] = cnt;
    __syncthreads();
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x < 27) partial[(size_t)threadIdx.x * nblocks + b] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
    if (threadIdx.x == 27 && matched) {
        const float c = (sh[0][27] + sh[1][27]) + (sh[2][27] + sh[3][27]);
        if (c > 0.f) atomicAdd(matched, (unsigned int)c);
    }
}

__global__ __launch_bounds__(64) void icp_final_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ out) {
    double acc = 0.0;
    const float* p = partial + (size_t)blockIdx.x * nblocks;
    for (int i = threadIdx.x; i < nblocks; i += 64) acc += (double)p[i];
    acc = wave_sum_all(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)acc;
}

struct RigidCloudArgs {
    const float* vertices;
    const float* normals;  // or null: no cosine gate
    int stride, n;
    Aff3 aff;
    const float* vmap;
    const float* nmap;
    int vstep, nstep, cols, rows;
    float fx, fy, cx, cy, dist_thresh, cos_thresh;
};

struct __attribute__((packed, aligned(4))) Packed3 {  // one 12-byte load
    float x, y, z;
};

// One lane per vertex c (normal n0), float32 (tests/rigid_align_statement.py states the same):
//   s = R c + t; no row if c.x is NaN or s.z > 0 fails
//   u = rintf(fx * (s.x / s.z) + cx), w likewise (ties to even); no row outside [0, cols) x [0, rows) (compared as floats: a
//   NaN or an overflowed quotient is outside)
//   L, Ln the float4 pixels of the two maps; no row if L.x or Ln.x is NaN
//   gates: sqrtf(|s - L|^2) <= dist_thresh, and with normals dot(R n0, Ln) >= cos_thresh (signed)
//   row (s x Ln, Ln | Ln . (L - s))
// (row and ok are out-parameters the caller has zeroed: in this form the compiler makes of rigid_rows_cloud_kernel what it made
// of it with the row written out in its body)
__device__ __forceinline__ void rigid_cloud_row(const RigidCloudArgs& a, const Aff3& aff, size_t i, bool in_range, float (&row)[7],
                                                bool& ok) {
    if (in_range) {
        const Packed3 c = *reinterpret_cast<const Packed3*>(a.vertices + i * (size_t)a.stride);
        Packed3 n0{0.f, 0.f, 0.f};
        if (a.normals) n0 = *reinterpret_cast<const Packed3*>(a.normals + i * (size_t)a.stride);  // (uniform)
        const f3 s = mulR(aff, mk3(c.x, c.y, c.z)) + mk3(aff.t[0], aff.t[1], aff.t[2]);
        if (c.x == c.x && s.z > 0.f) {
            const float u = rintf(a.fx * (s.x / s.z) + a.cx), w = rintf(a.fy * (s.y / s.z) + a.cy);
            if (u >= 0.f && w >= 0.f && u < (float)a.cols && w < (float)a.rows) {
                const size_t px = 16 * (size_t)(int)u;
                // two gathers: both in flight before either is looked at
                const float4 L  = *reinterpret_cast<const float4*>((const char*)a.vmap + (size_t)(int)w * a.vstep + px);
                const float4 Ln = *reinterpret_cast<const float4*>((const char*)a.nmap + (size_t)(int)w * a.nstep + px);
                if (L.x == L.x && Ln.x == Ln.x) {
                    const f3 l = mk3(L.x, L.y, L.z), n = mk3(Ln.x, Ln.y, Ln.z);
                    const f3 sl = s - l;
                    ok = sqrtf(dot(sl, sl)) <= a.dist_thresh;
                    if (ok && a.normals) ok = dot(mulR(aff, mk3(n0.x, n0.y, n0.z)), n) >= a.cos_thresh;
                    if (ok) {
                        row[0] = s.y * n.z - s.z * n.y, row[1] = s.z * n.x - s.x * n.z, row[2] = s.x * n.y - s.y * n.x;
                        row[3] = n.x, row[4] = n.y, row[5] = n.z;
                        row[6] = dot(n, l - s);
                    }
                }
            }
        }
    }
}

// the 27 products of a workgroup's rows and its matched count: per wave with DPP adds, per workgroup through LDS, one
// partial per product at partial[q * nblocks + blockIdx.x]; the count is added to *matched (may be null)
__device__ __forceinline__ void rigid_cloud_reduce(const float row[7], bool ok, float (&sh)[4][27], unsigned int (&sh_count)[4],
                                                   float* __restrict__ partial, int nblocks, unsigned int* __restrict__ matched) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int j = r; j < 7; ++j) {
            const float t = wave_total(row[r] * row[j]);
            if (lane == 0) sh[wave][q] = t;
            ++q;
        }
    const unsigned int cnt = (unsigned int)__popcll(__ballot(ok));  // integers: the count is exact
    if (lane == 0) sh_count[wave] = cnt;
    __syncthreads();
    if (threadIdx.x < 27)
        partial[(size_t)threadIdx.x * nblocks + blockIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
    if (threadIdx.x == 27 && matched) {
        const unsigned int c = (sh_count[0] + sh_count[1]) + (sh_count[2] + sh_count[3]);
        if (c) atomicAdd(matched, c);
    }
}

__global__ __launch_bounds__(256) void rigid_rows_cloud_kernel(const RigidCloudArgs a, float* __restrict__ partial, int nblocks,
                                                               unsigned int* __restrict__ matched) {
    __shared__ float sh[4][27];
    __shared__ unsigned int sh_count[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    float row[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool ok = false;
    rigid_cloud_row(a, a.aff, i, i < (size_t)a.n, row, ok);
    rigid_cloud_reduce(row, ok, sh, sh_count, partial, nblocks, matched);
}

// The row kernel of dfa_rigid_align_cloud: rigid_rows_cloud_kernel, but the pose comes from the device-resident state of the
// call (a.aff is the call's aff0, the pose until an update was accepted), a launch whose level is finished or whose call met
// a singular system returns at entry, and the launch visits every `step`-th vertex: vertex j of the level is vertex j * step
// of the cloud, workgroup b takes vertices 256 b ... 256 b + 255 of the level's n_level = ceil(a.n / step).  The matched
// count goes into the iteration's own slot of the state.
__global__ __launch_bounds__(256) void rigid_loop_rows_kernel(const RigidCloudArgs a, RigidLoopState* __restrict__ state, int level,
                                                              int iter, int step, int n_level, float* __restrict__ partial,
                                                              int nblocks) {
    __shared__ float sh[4][27];
    __shared__ unsigned int sh_count[4];
    if (!rigid_loop_active(*state, level)) return;
    Aff3 aff = a.aff;
    if (state->have_pose) {
#pragma unroll
        for (int k = 0; k < 9; ++k) aff.m[k] = state->aff[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) aff.t[k] = state->aff[9 + k];
    }
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    float row[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool ok = false;
    rigid_cloud_row(a, aff, j * (size_t)step, j < (size_t)n_level, row, ok);
    rigid_cloud_reduce(row, ok, sh, sh_count, partial, nblocks, &state->matched[iter]);
}

// The step kernel of dfa_rigid_align_cloud, ONE workgroup of 16 waves.  Each of the 27 sums is added by one wave in double in
// icp_final_kernel's order (lane-strided by 64, then the wave sum) and rounded to float: the bits dfa_rigid_sums_cloud returns
// for that pose and that subsampled cloud.  Lane 0 then runs rigid_loop_advance (rigid_step.hpp: the 6x6 step and the rules
// of the loop) and writes the iteration's trace row.  The last launch of a call (report != null) fills the report whether
// or not its iteration still ran; iter < 0 is a call without iterations: the report only.
__global__ __launch_bounds__(1024) void rigid_loop_step_kernel(RigidLoopState* __restrict__ state, const Aff3 aff0,
                                                               const float* __restrict__ partial, int nblocks, int level, int iter,
                                                               float stop_rot, float stop_trans, float* __restrict__ trace,
                                                               dfa_rigid_align_report* __restrict__ report) {
    __shared__ float sums[27];
    const bool active = iter >= 0 && rigid_loop_active(*state, level);  // (uniform)
    if (!active && !report) return;
    float a0[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) a0[k] = k < 9 ? aff0.m[k] : aff0.t[k - 9];
    if (active) {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        // a wave adds sums `wave` and `wave + 16` side by side, eight partials of each in flight: the ADDS of a sum stay in
        // icp_final_kernel's order, the loads do not wait for one another (one workgroup has this to itself: at a million
        // vertices a lane would otherwise make 2 x 66 round trips to the L2, one behind the other)
        const bool two  = wave + 16 < 27;
        const float* p0 = partial + (size_t)wave * nblocks;
        const float* p1 = partial + (size_t)(two ? wave + 16 : wave) * nblocks;
        double acc0 = 0.0, acc1 = 0.0;
        int i = lane;
        for (; i + 7 * 64 < nblocks; i += 8 * 64) {
            float x0[8], x1[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x0[k] = p0[i + 64 * k], x1[k] = p1[i + 64 * k];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc0 += (double)x0[k], acc1 += (double)x1[k];
        }
        for (; i < nblocks; i += 64) acc0 += (double)p0[i], acc1 += (double)p1[i];
        acc0 = wave_sum_all(acc0), acc1 = wave_sum_all(acc1);
        if (lane == 0) {
            sums[wave] = (float)acc0;
            if (two) sums[wave + 16] = (float)acc1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (trace) {
                float* row = trace + 40 * (size_t)iter;
                float at[12];
                rigid_loop_pose(*state, a0, at);
                for (int q = 0; q < 27; ++q) row[q] = sums[q];
                row[27] = __uint_as_float(state->matched[iter]);
                for (int k = 0; k < 12; ++k) row[28 + k] = at[k];
            }
            rigid_loop_advance(*state, a0, level, iter, sums, stop_rot, stop_trans);
        }
    }
    if (report && threadIdx.x == 0) {
        const bool good = state->status == 0;
        for (int k = 0; k < 12; ++k) report->aff[k] = good && state->have_pose ? state->aff[k] : a0[k];
        report->status = state->status;
        for (int l = 0; l < RIGID_MAX_LEVELS; ++l) report->iters_run[l] = state->iters_run[l];
        report->matched_first = iter >= 0 ? state->matched[0] : 0u;
        report->matched_last  = iter >= 0 ? state->matched[state->last_iter] : 0u;
        report->last_rot      = state->last_rot;
        report->last_trans    = state->last_trans;
    }
}

}  // namespace

size_t icp_partial_floats(int cols, int rows) { return (size_t)27 * ((cols + 31) / 32) * ((rows + 7) / 8); }

hipError_t launch_icp_sums(bool depth_variant, const void* curr, int curr_step, const float* ncurr, int ncurr_step,
                           const void* prev, int prev_step, const float* nprev, int nprev_step, int cols, int rows,
                           const float aff[12], float fx, float fy, float cx, float cy, float dist_thres, float angle_thres,
                           float* partial, float* sums27, unsigned int* matched, hipStream_t s) {
    IcpArgs a;
    a.curr = curr, a.ncurr = ncurr, a.prev = prev, a.nprev = nprev;
    a.curr_step = curr_step, a.ncurr_step = ncurr_step, a.prev_step = prev_step, a.nprev_step = nprev_step;
    a.cols = cols, a.rows = rows;
    for (int i = 0; i < 9; ++i) a.aff.m[i] = aff[i];
    for (int i = 0; i < 3; ++i) a.aff.t[i] = aff[9 + i];
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy, a.finvx = 1.f / fx, a.finvy = 1.f / fy;  // setLevelIntr, projective_icp.cpp:15-20
    a.min_cosine  = cosf(angle_thres);                                                     // :10-13
    a.dist2_thres = dist_thres * dist_thres;
    dim3 grid((cols + 31) / 32, (rows + 7) / 8);
    const int nblocks = (int)(grid.x * grid.y);
    if (matched) {
        hipError_t e = hipMemsetAsync(matched, 0, sizeof(unsigned int), s);
        if (e != hipSuccess) return e;
    }
    if (depth_variant) icp_rows_kernel<true><<<grid, 256, 0, s>>>(a, partial, nblocks, matched);
    else icp_rows_kernel<false><<<grid, 256, 0, s>>>(a, partial, nblocks, matched);
    icp_final_kernel<<<27, 64, 0, s>>>(partial, nblocks, sums27);
    return hipGetLastError();
}

size_t rigid_cloud_partial_floats(int n) { return (size_t)27 * (size_t)(((long)n + 255) / 256); }

hipError_t launch_rigid_sums_cloud(const float* vertices, const float* normals, int stride, int n, const float aff[12],
                                   const float* vmap, int vstep, const float* nmap, int nstep, int cols, int rows, float fx,
                                   float fy, float cx, float cy, float dist_thresh, float cos_thresh, float* partial,
                                   float* sums27, unsigned int* matched, hipStream_t s) {
    if (matched) {
        hipError_t e = hipMemsetAsync(matched, 0, sizeof(unsigned int), s);
        if (e != hipSuccess) return e;
    }
    if (n <= 0) return hipMemsetAsync(sums27, 0, 27 * sizeof(float), s);
    RigidCloudArgs a;
    a.vertices = vertices, a.normals = normals, a.stride = stride, a.n = n;
    a.aff  = aff3_from(aff);
    a.vmap = vmap, a.nmap = nmap, a.vstep = vstep, a.nstep = nstep, a.cols = cols, a.rows = rows;
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy, a.dist_thresh = dist_thresh, a.cos_thresh = cos_thresh;
    const int nblocks = (int)(((long)n + 255) / 256);
    rigid_rows_cloud_kernel<<<nblocks, 256, 0, s>>>(a, partial, nblocks, matched);
    icp_final_kernel<<<27, 64, 0, s>>>(partial, nblocks, sums27);
    return hipGetLastError();
}

static int rigid_level_vertices(int n, int step) { return (int)(((long)n + step - 1) / step); }

size_t rigid_align_scratch_floats(int n, const int* level_step, int levels) {
    int most = 0;
    for (int l = 0; l < levels; ++l) most = std::max(most, rigid_level_vertices(n, level_step[l]));
    return RIGID_STATE_FLOATS + rigid_cloud_partial_floats(std::max(most, 1));
}

hipError_t launch_rigid_align_cloud(const float* vertices, const float* normals, int stride, int n, const float aff0[12],
                                    const float* vmap, int vstep, const float* nmap, int nstep, int cols, int rows, float fx,
                                    float fy, float cx, float cy, float dist_thresh, float cos_thresh, const int* level_step,
                                    const int* level_iters, int levels, float stop_rot, float stop_trans,
                                    dfa_rigid_align_report* report, float* trace, float* scratch, hipStream_t s) {
    static_assert(sizeof(RigidLoopState) <= RIGID_STATE_FLOATS * sizeof(float), "the state's room in the scratch");
    RigidLoopState* state = reinterpret_cast<RigidLoopState*>(scratch);
    float* partial        = scratch + RIGID_STATE_FLOATS;
    int total             = 0;
    for (int l = 0; l < levels; ++l) total += level_iters[l];
    hipError_t e = hipMemsetAsync(state, 0, sizeof(RigidLoopState), s);  // once per call: every iteration has its own slots
    if (e != hipSuccess) return e;
    if (trace && total > 0 && (e = hipMemsetAsync(trace, 0xff, sizeof(float) * 40 * (size_t)total, s)) != hipSuccess) return e;
    RigidCloudArgs a;
    a.vertices = vertices, a.normals = normals, a.stride = stride, a.n = n;
    a.aff  = aff3_from(aff0);
    a.vmap = vmap, a.nmap = nmap, a.vstep = vstep, a.nstep = nstep, a.cols = cols, a.rows = rows;
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy, a.dist_thresh = dist_thresh, a.cos_thresh = cos_thresh;
    if (total == 0) {
        rigid_loop_step_kernel<<<1, 1024, 0, s>>>(state, a.aff, partial, 0, 0, -1, stop_rot, stop_trans, nullptr, report);
        return hipGetLastError();
    }
    int iter = 0;
    for (int l = 0; l < levels; ++l) {
        const int n_level = rigid_level_vertices(n, level_step[l]);
        const int nblocks = std::max((n_level + 255) / 256, 1);  // an empty cloud: one workgroup of zeros, a singular system
        for (int it = 0; it < level_iters[l]; ++it, ++iter) {
            rigid_loop_rows_kernel<<<nblocks, 256, 0, s>>>(a, state, l, iter, level_step[l], n_level, partial, nblocks);
            rigid_loop_step_kernel<<<1, 1024, 0, s>>>(state, a.aff, partial, nblocks, l, iter, stop_rot, stop_trans, trace,
                                                      iter == total - 1 ? report : nullptr);
        }
    }
    return hipGetLastError();
}

}  // namespace dfa
