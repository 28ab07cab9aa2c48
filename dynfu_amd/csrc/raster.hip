// raster.hip — gfx950 mesh rasteriser: triangles in, per-pixel point and normal maps out, nearest surface wins.  The
// consumer of the indexed marching-cubes mesh (mc.hip) after it has been carried through the warp field (warp.hip): a
// warped surface cannot be raycast.  No reference counterpart.  Three steps on one stream: fill the z-buffer with
// "miss", draw (64-bit atomicMin per covered pixel), resolve (one thread per pixel).  tests/raster_statement.py states
// the same contract in numpy; the maps are reproducible from it byte for byte.
//
// Contract.  float32 throughout under -ffp-contract=off; an fma only inside dot() (device_math.hpp).
//   vertex     P = R p + t as dfa_transform_points orders it: ((R0 x + R1 y) + R2 z) + t, per row of world2cam.
//              iz = 1 / P.z, u = (P.x fx) iz + cx, v = (P.y fy) iz + cy.  Pixel (i, j) has its centre at u = i, v = j.
//              Snapped to 1/256 pixel: sx = (int) floorf(u 256 + 0.5f), sy likewise.
//   skipped    whole triangles, nothing is clipped: an index outside [0, N); a vertex with a non-finite P or P.z < z_near;
//              |floorf(u 256 + 0.5f)| or the same of v not below 2^22 (a guard band of 16384 pixels: every edge function
//              fits in int64); zero doubled area.
//   coverage   orient(a, b, c) = (b.x - a.x)(c.y - a.y) - (b.y - a.y)(c.x - a.x) in int64 on the snapped coordinates, the
//              pixel centre c = (256 i, 256 j).  area2 = orient(v0, v1, v2); when negative v1 and v2 change places (iz and
//              normals with them) and area2 changes sign, so both windings are drawn.  E0 = orient(v1, v2, c),
//              E1 = orient(v2, v0, c), E2 = orient(v0, v1, c).  Covered: every E > 0, or E == 0 on a top or left edge —
//              the edge a -> b with d = b - a is one when d.y < 0 (left: y grows downwards and the inside is to its right)
//              or d.y == 0 and d.x > 0 (top).  Two triangles that share an edge run through it in opposite directions, so
//              a centre on it belongs to exactly one of them: coverage is exact and watertight.
//   depth      perspective-correct: w_i = (float) E_i, q = (w0 iz0 + w1 iz1) + w2 iz2, z = (float) area2 / q.
//   visibility key = (bits(z) << 32) | triangle, merged with a 64-bit atomicMin; a miss is all ones.  z > 0, so its bits
//              order as z does: the nearest depth wins, the lower triangle number on equal bits, and the z-buffer does not
//              depend on the order the atomics land in.  (Device-scope atomics, executed at the memory side: coherent over
//              the XCDs; the resolve is a later launch.)
//   resolve    miss: quiet NaN (0x7fffffff) in all four components of both maps, as dfa_tsdf_raycast_points writes it.
//              hit: point = (((i - cx) z) / fx, ((j - cy) z) / fy, z, 0).  Normal: the winner's E_i again, b_i = w_i iz_i,
//              n = (b0 N0 + b1 N1) + b2 N2 per component with N_i = (R0 x + R1 y) + R2 z of vertex normal i; without
//              vertex normals n = (P1 - P0) x (P2 - P0) of the camera-frame triangle (after the change of places), each
//              component a y b z - a z b y, negated when dot(n, P0) > 0 so that it faces the camera.  Written as
//              n (1 / sqrtf(dot(n, n))), 0; all four components quiet NaN unless 0 < dot(n, n) < inf.  The point stays.
//              Bytes of a pitched row beyond its last pixel are not touched.
//
// Shape of the draw.  Marching-cubes triangles at 512^3 under a VGA camera cover about a pixel each: one lane per
// triangle walks its clipped bounding box with incremental edge functions.  A triangle whose box holds more than
// RASTER_WIDE_BOX pixel centres would hold its wave for as long as one lane needs; those are left for a second phase inside
// the wave: a loop over the ballot of their lanes, every lane sets the same triangle up again (a broadcast load of three
// vertices) and the 64 lanes cover the box as 8 x 8 tiles.  No work list, no scratch but the caller's z-buffer.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"

namespace dfa {

// Pixel centres in a box above which the whole wave draws the triangle.  Measured at 16, 64 and 1024
// (tools/mesh_view_timing.py; DESIGN_NOTES.md "Mesh rasteriser"): no difference where triangles cover about a pixel; from a
// camera four times nearer, where boxes hold tens to hundreds of centres, 1024 draws in 0.035 ms what 64 draws in 0.138 ms —
// a wave that takes its wide triangles one after the other pays 64 set-ups and half-empty 8 x 8 tiles for work its lanes do
// side by side in a few hundred steps each.  The wave form is for the triangle that would hold one lane for thousands of
// steps; at 1024 a lane's walk is bounded by what a 32 x 32 box costs.
#ifndef DFA_RASTER_WIDE_BOX
#define DFA_RASTER_WIDE_BOX 1024
#endif
constexpr int RASTER_WIDE_BOX = DFA_RASTER_WIDE_BOX;

constexpr unsigned long long RASTER_MISS = ~0ull;

struct RasterCam {
    float r[9], t[3];
    float fx, fy, cx, cy, z_near;
    int cols, rows;
};

struct RasterTri {
    int x[3], y[3];  // snapped, 1/256 pixel
    float iz[3];
    long long area2;         // > 0
    int vertex[3];           // after the change of places
    f3 P[3];                 // camera frame
    int i0, i1, j0, j1;      // pixel centres inside the bounding box and the image, inclusive; empty when i0 > i1 or j0 > j1
};

__device__ __forceinline__ f3 rotate(const RasterCam& c, float x, float y, float z) {
    return mk3((c.r[0] * x + c.r[1] * y) + c.r[2] * z, (c.r[3] * x + c.r[4] * y) + c.r[5] * z, (c.r[6] * x + c.r[7] * y) + c.r[8] * z);
}

__device__ __forceinline__ bool finite3(f3 p) { return __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z); }

__device__ __forceinline__ bool snap_vertex(const RasterCam& c, f3 P, int& sx, int& sy, float& iz) {
    if (!finite3(P) || P.z < c.z_near) return false;
    iz             = 1.f / P.z;
    const float u  = (P.x * c.fx) * iz + c.cx;
    const float v  = (P.y * c.fy) * iz + c.cy;
    const float fu = floorf(u * 256.f + 0.5f), fv = floorf(v * 256.f + 0.5f);
    if (!(fabsf(fu) < 4194304.f && fabsf(fv) < 4194304.f)) return false;  // (NaN fails too)
    sx = (int)fu, sy = (int)fv;
    return true;
}

template <class T>
__device__ __forceinline__ void exchange(T& a, T& b) {
    const T t = a;
    a = b, b = t;
}

// false: the triangle is skipped
__device__ __forceinline__ bool setup_triangle(const RasterCam& c, const float* __restrict__ vertices,
                                               const int32_t* __restrict__ indices, int N, int t, RasterTri& tri) {
#pragma unroll
    for (int k = 0; k < 3; ++k) tri.vertex[k] = indices[3 * (size_t)t + k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if ((unsigned)tri.vertex[k] >= (unsigned)N) return false;
    float4 p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = reinterpret_cast<const float4*>(vertices)[tri.vertex[k]];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const f3 r = rotate(c, p[k].x, p[k].y, p[k].z);
        tri.P[k]   = mk3(r.x + c.t[0], r.y + c.t[1], r.z + c.t[2]);
        ok         = snap_vertex(c, tri.P[k], tri.x[k], tri.y[k], tri.iz[k]) && ok;
    }
    if (!ok) return false;
    tri.area2 = (long long)(tri.x[1] - tri.x[0]) * (tri.y[2] - tri.y[0]) - (long long)(tri.y[1] - tri.y[0]) * (tri.x[2] - tri.x[0]);
    if (tri.area2 == 0) return false;
    if (tri.area2 < 0) {
        exchange(tri.x[1], tri.x[2]), exchange(tri.y[1], tri.y[2]), exchange(tri.iz[1], tri.iz[2]);
        exchange(tri.vertex[1], tri.vertex[2]), exchange(tri.P[1], tri.P[2]);
        tri.area2 = -tri.area2;
    }
    const int xmin = min(tri.x[0], min(tri.x[1], tri.x[2])), xmax = max(tri.x[0], max(tri.x[1], tri.x[2]));
    const int ymin = min(tri.y[0], min(tri.y[1], tri.y[2])), ymax = max(tri.y[0], max(tri.y[1], tri.y[2]));
    tri.i0 = max(0, (xmin + 255) >> 8), tri.i1 = min(c.cols - 1, xmax >> 8);  // ceil / floor of x / 256 (arithmetic shift)
    tri.j0 = max(0, (ymin + 255) >> 8), tri.j1 = min(c.rows - 1, ymax >> 8);
    return true;
}

// the three edge functions of pixel centre (i, j)
__device__ __forceinline__ void edge_functions(const RasterTri& t, int i, int j, long long E[3]) {
    const int px = i << 8, py = j << 8;
    E[0] = (long long)(t.x[2] - t.x[1]) * (py - t.y[1]) - (long long)(t.y[2] - t.y[1]) * (px - t.x[1]);
    E[1] = (long long)(t.x[0] - t.x[2]) * (py - t.y[2]) - (long long)(t.y[0] - t.y[2]) * (px - t.x[2]);
    E[2] = (long long)(t.x[1] - t.x[0]) * (py - t.y[0]) - (long long)(t.y[1] - t.y[0]) * (px - t.x[0]);
}

// 0 for a top or left edge a -> b (a zero of its edge function is inside), else 1 (it is not)
__device__ __forceinline__ int edge_bias(int ax, int ay, int bx, int by) {
    const int dx = bx - ax, dy = by - ay;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}
__device__ __forceinline__ void edge_biases(const RasterTri& t, int bias[3]) {
    bias[0] = edge_bias(t.x[1], t.y[1], t.x[2], t.y[2]);
    bias[1] = edge_bias(t.x[2], t.y[2], t.x[0], t.y[0]);
    bias[2] = edge_bias(t.x[0], t.y[0], t.x[1], t.y[1]);
}

__device__ __forceinline__ float fragment_depth(const RasterTri& t, const long long E[3]) {
    const float q = ((float)E[0] * t.iz[0] + (float)E[1] * t.iz[1]) + (float)E[2] * t.iz[2];
    return (float)t.area2 / q;
}

__device__ __forceinline__ void merge_fragment(const RasterTri& t, int id, const long long E[3], const int bias[3],
                                               unsigned long long* __restrict__ pixel) {
    if (E[0] < bias[0] || E[1] < bias[1] || E[2] < bias[2]) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(fragment_depth(t, E)) << 32) | (uint32_t)id;
    atomicMin(pixel, key);
}

__global__ __launch_bounds__(256) void raster_draw_kernel(const RasterCam c, const float* __restrict__ vertices,
                                                          const int32_t* __restrict__ indices, int N, int T,
                                                          unsigned long long* __restrict__ zbuffer) {
    const int t    = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    RasterTri tri;
    const bool live = t < T && setup_triangle(c, vertices, indices, N, t, tri) && tri.i0 <= tri.i1 && tri.j0 <= tri.j1;
    const bool wide = live && (tri.i1 - tri.i0 + 1) * (tri.j1 - tri.j0 + 1) > RASTER_WIDE_BOX;  // (at most 8192^2 centres)
    if (live && !wide) {
        int bias[3];
        edge_biases(tri, bias);
        long long row[3];
        edge_functions(tri, tri.i0, tri.j0, row);
        // one pixel to the right: px grows by 256, E = dx (py - ay) - dy (px - ax) by -256 dy; one row down by 256 dx
        const long long sx[3] = {-256ll * (tri.y[2] - tri.y[1]), -256ll * (tri.y[0] - tri.y[2]), -256ll * (tri.y[1] - tri.y[0])};
        const long long sy[3] = {256ll * (tri.x[2] - tri.x[1]), 256ll * (tri.x[0] - tri.x[2]), 256ll * (tri.x[1] - tri.x[0])};
        for (int j = tri.j0; j <= tri.j1; ++j) {
            long long E[3] = {row[0], row[1], row[2]};
            for (int i = tri.i0; i <= tri.i1; ++i) {
                merge_fragment(tri, t, E, bias, zbuffer + (size_t)j * c.cols + i);
                E[0] += sx[0], E[1] += sx[1], E[2] += sx[2];
            }
            row[0] += sy[0], row[1] += sy[1], row[2] += sy[2];
        }
    }
    // the wide triangles of this wave, one after the other, by all of its lanes
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int id = __shfl(t, src, 64);
        RasterTri b;
        if (!setup_triangle(c, vertices, indices, N, id, b)) continue;  // (wave-uniform; it was drawable in lane src)
        int bias[3];
        edge_biases(b, bias);
        const int lx = lane & 7, ly = lane >> 3;
        for (int tj = b.j0; tj <= b.j1; tj += 8)
            for (int ti = b.i0; ti <= b.i1; ti += 8) {
                const int i = ti + lx, j = tj + ly;
                if (i > b.i1 || j > b.j1) continue;
                long long E[3];
                edge_functions(b, i, j, E);
                merge_fragment(b, id, E, bias, zbuffer + (size_t)j * c.cols + i);
            }
    }
}

// block (64, 4): a wave reads 512 contiguous bytes of the z-buffer and writes 1 KiB of each map
__global__ __launch_bounds__(256) void raster_resolve_kernel(const RasterCam c, const float* __restrict__ vertices,
                                                             const float* __restrict__ normals,
                                                             const int32_t* __restrict__ indices, int N, int T,
                                                             const unsigned long long* __restrict__ zbuffer,
                                                             float* __restrict__ points, int points_step,
                                                             float* __restrict__ out_normals, int normals_step) {
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (i >= c.cols || j >= c.rows) return;
    const float nan = __uint_as_float(0x7fffffffu);
    float4 p = make_float4(nan, nan, nan, nan), n = p;
    const unsigned long long key = zbuffer[(size_t)j * c.cols + i];
    const uint32_t id            = (uint32_t)key;
    RasterTri tri;
    if (key != RASTER_MISS && id < (uint32_t)T && setup_triangle(c, vertices, indices, N, (int)id, tri)) {
        const float z = __uint_as_float((uint32_t)(key >> 32));
        p             = make_float4((((float)i - c.cx) * z) / c.fx, (((float)j - c.cy) * z) / c.fy, z, 0.f);
        f3 s;
        if (normals) {
            long long E[3];
            edge_functions(tri, i, j, E);
            float b[3];
            f3 nv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                b[k]            = (float)E[k] * tri.iz[k];
                const float4 nk = reinterpret_cast<const float4*>(normals)[tri.vertex[k]];
                nv[k]           = rotate(c, nk.x, nk.y, nk.z);
            }
            s = mk3((b[0] * nv[0].x + b[1] * nv[1].x) + b[2] * nv[2].x, (b[0] * nv[0].y + b[1] * nv[1].y) + b[2] * nv[2].y,
                    (b[0] * nv[0].z + b[1] * nv[1].z) + b[2] * nv[2].z);
        } else {
            const f3 a = tri.P[1] - tri.P[0], d = tri.P[2] - tri.P[0];
            s          = mk3(a.y * d.z - a.z * d.y, a.z * d.x - a.x * d.z, a.x * d.y - a.y * d.x);
            if (dot(s, tri.P[0]) > 0.f) s = mk3(-s.x, -s.y, -s.z);
        }
        const float len2 = dot(s, s);
        if (len2 > 0.f && len2 < __builtin_inff()) {
            const f3 u = s * (1.0f / sqrtf(len2));
            n          = make_float4(u.x, u.y, u.z, 0.f);
        }
    }
    if (points) reinterpret_cast<float4*>((char*)points + (size_t)j * points_step)[i] = p;
    if (out_normals) reinterpret_cast<float4*>((char*)out_normals + (size_t)j * normals_step)[i] = n;
}

hipError_t launch_mesh_rasterize(const float* vertices, const float* normals, int N, const int32_t* indices, int T,
                                 const float world2cam[12], float fx, float fy, float cx, float cy, float z_near, int cols,
                                 int rows, uint64_t* zbuffer, float* points, int points_step, float* out_normals,
                                 int normals_step, hipStream_t s) {
    RasterCam c;
    const float identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    const float* m           = world2cam ? world2cam : identity;
    for (int k = 0; k < 9; ++k) c.r[k] = m[k];
    for (int k = 0; k < 3; ++k) c.t[k] = m[9 + k];
    c.fx = fx, c.fy = fy, c.cx = cx, c.cy = cy, c.z_near = z_near, c.cols = cols, c.rows = rows;
    hipError_t e = hipMemsetAsync(zbuffer, 0xff, (size_t)rows * cols * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    unsigned long long* zb = reinterpret_cast<unsigned long long*>(zbuffer);
    if (T > 0) raster_draw_kernel<<<(T + 255) / 256, 256, 0, s>>>(c, vertices, indices, N, T, zb);
    if (points || out_normals)
        raster_resolve_kernel<<<dim3((cols + 63) / 64, (rows + 3) / 4), dim3(64, 4), 0, s>>>(
            c, vertices, normals, indices, N, T, zb, points, points_step, out_normals, normals_step);
    return hipGetLastError();
}

}  // namespace dfa
