// solve6_internal.hpp — what the units of the north-star solve (solve6_graph / _pattern / _linearise / _assemble / _pcg /
// _update .hip) have in common and nobody else uses.  Most entries are called from two or three units: the point
// transform, the energy's total, the LDS sort of the two per-node lists, the k dispatch, the work units of a node, the
// phase clocks of the DFA_S6_TIMING build, the pattern's launcher.  A few have one calling unit and stand here as one
// stage's side of what another stage relies on: s6_node_now (what the linearisation and the assembly read), the
// workgroup's share of the energy and the bookkeeping after its total, the plan's capacity, dot3.  Internal to those six
// files; the launchers the C ABI calls are in solve6.hpp.  Every device helper is __device__ __forceinline__
// (s6_linearise_blocks: __host__ __device__ inline) in an anonymous namespace: the library is built without relocatable
// device code, no unit exports or imports device symbols.
// Beside each entry, in brackets: the units that use it (_x = solve6_x.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "blend6_device.hpp"
#include "dq_device.hpp"
#include "kernels.hpp"
#include "solve6.hpp"

namespace dfa {

namespace {

// (qconj, qdot, pureq, qvec: blend6_device.hpp)
// [called by: _linearise]
__device__ __forceinline__ float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// e_c^ (x) q for the basis vectors e_x, e_y, e_z  [called by: s6_node_now below]
__device__ __forceinline__ Quat basis_mul(int c, Quat q) {
    return c == 0 ? Quat{-q.x, q.w, -q.z, q.y} : c == 1 ? Quat{-q.y, q.z, q.w, -q.x} : Quat{-q.z, -q.y, q.x, q.w};
}
// rotation + translation of a unit dual quaternion  [called by: s6_node_now below, _linearise (s6_reg_edge)]
__device__ __forceinline__ f3 dq_point(DQ q, f3 c) {
    const f3 rc = qvec(qmul(qmul(q.r, pureq(c)), qconj(q.r)));
    const f3 t  = qvec(qmul(q.d, qconj(q.r)));
    return mk3(rc.x + 2.f * t.x, rc.y + 2.f * t.y, rc.z + 2.f * t.z);
}

// g^_n = T_n(g_n) and M_n of node n at transform q (part of the launch that produced q: s6_begin / s6_update)
// [called by: _update (s6_begin_kernel, s6_update_kernel); what it writes is read by _linearise (ghat) and _assemble (mnode)]
__device__ __forceinline__ void s6_node_now(const Solve6View& s, int n, DQ q) {
    const f3 g = dq_point(q, mk3(s.node_pos[3 * n], s.node_pos[3 * n + 1], s.node_pos[3 * n + 2]));
    s.ghat[3 * n] = g.x, s.ghat[3 * n + 1] = g.y, s.ghat[3 * n + 2] = g.z;
    // M_n (6 x 8): the twist components of node n as dual-quaternion increments (W, Wd).  A data row's
    // 6-vector for a neighbour n is f_vn * M_n l_v with the per-vertex functional l_v = (lW, lD) of
    // s6_linearise — the assembly accumulates 8 x 8 moments of l and applies M afterwards.
    float* M = s.mnode + 48 * (size_t)n;
#pragma unroll
    for (int col = 0; col < 3; ++col) {
        const f3 e    = mk3(col == 0 ? 1.f : 0.f, col == 1 ? 1.f : 0.f, col == 2 ? 1.f : 0.f);
        const Quat W  = basis_mul(col, q.r);                                         // omega = e_col
        const Quat Wd = qadd(basis_mul(col, q.d), qmul(pureq(cross(g, e)), q.r));    // rotation about g^: v0 = g^ x e
        float* r0 = M + 8 * col;
        r0[0] = W.w, r0[1] = W.x, r0[2] = W.y, r0[3] = W.z, r0[4] = Wd.w, r0[5] = Wd.x, r0[6] = Wd.y, r0[7] = Wd.z;
        float* r1 = M + 8 * (3 + col);                                               // translation e_col: (0, e^ r)
        r1[0] = 0.f, r1[1] = 0.f, r1[2] = 0.f, r1[3] = 0.f, r1[4] = W.w, r1[5] = W.x, r1[6] = W.y, r1[7] = W.z;
    }
}

// The energy of a linearisation: every workgroup leaves ITS sum (and count of valid rows) in cost_part / valid_part, the
// first workgroup of the assembly that follows adds them up in a fixed order (s6_cost_total).  Two atomicAdds per workgroup
// on the state block's two words — 4 000 same-address fp64 atomics per launch at C3 — cost 15-25 us of the launch
// (C2 0.033 -> 0.017 ms, C3 0.061 -> 0.041), and their order decided the last bits of the sum.
// [called by: _linearise]
__device__ __forceinline__ void block_add_cost(double cost, unsigned int nvalid, const Solve6View& s, bool through = false) {
    __shared__ double sc[8];
    __shared__ unsigned int sn[8];
    cost   = wave_sum_all(cost);
    nvalid = (unsigned int)wave_sum_all((double)nvalid);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) sc[wave] = cost, sn[wave] = nvalid;
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0;
        unsigned int n = 0;
        for (int w = 0; w < nw; ++w) c += sc[w], n += sn[w];
        if (through) {  // read by ANOTHER workgroup of this launch (its last one): written through, past this XCD's L2
            __hip_atomic_store(&s.cost_part[blockIdx.x], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&s.valid_part[blockIdx.x], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            s.cost_part[blockIdx.x] = c, s.valid_part[blockIdx.x] = n;
        }
    }
}
__host__ __device__ inline int s6_linearise_blocks(int N, int D, int k) { return (N + 255) / 256 + (D * k + 255) / 256; }
// by all 256 threads of one workgroup: the partial sums of the last linearisation, in a fixed order, into the state block
// [called by: _linearise (gn_tol > 0: the launch's last workgroup), _assemble (gn_tol <= 0: its extra workgroup)]
__device__ __forceinline__ void s6_cost_total(const Solve6View& s, Solve6State* st, bool through = false) {
    __shared__ double tc[4];
    __shared__ unsigned long long tn[4];
    const int n = s6_linearise_blocks(s.N, s.D, s.k), tid = threadIdx.x;
    double c = 0.0;
    unsigned long long v = 0ull;
    if (through) {
        // partials of the launch in flight: loads that do not stop at this XCD's L2 — each a round trip of ~2 us, and this is
        // the one workgroup the whole launch waits for: eight of them in flight per thread (clamped addresses, masked sums;
        // a loop of load-wait-add was five dependent round trips at C2: 9 us per linearisation)
        constexpr int Q = 8;
        for (int base = tid; base < n; base += 256 * Q) {
            double cq[Q];
            unsigned int vq[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int i = min(base + 256 * q, n - 1);
                cq[q] = __hip_atomic_load(&s.cost_part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                vq[q] = __hip_atomic_load(&s.valid_part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int q = 0; q < Q; ++q)
                if (base + 256 * q < n) c += cq[q], v += vq[q];
        }
    } else
    for (int i = tid; i < n; i += 256) c += s.cost_part[i], v += s.valid_part[i];
    c = wave_sum_all(c);
    v = (unsigned long long)wave_sum_all((double)v);  // (counts below 2^53: exact)
    if ((tid & 63) == 0) tc[tid >> 6] = c, tn[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) st->cost = (tc[0] + tc[1]) + (tc[2] + tc[3]), st->valid = (tn[0] + tn[1]) + (tn[2] + tn[3]);
}

// bookkeeping of the linearisation that just finished (one thread of the assembly launch): costs, the slot of this
// Gauss-Newton iteration in the per-iteration history, the stop test of the PCG that follows
// [called by: _assemble (gn_tol <= 0); s6_decide of _linearise is what runs instead when gn_tol > 0]
__device__ __forceinline__ void s6_bookkeeping(Solve6State* st, const S6Forcing f) {
    if (!st->have_first) st->initial_cost = st->cost, st->valid_first = st->valid, st->have_first = 1;
    st->final_cost = st->cost, st->valid_last = st->valid;
    const int h = st->gn_iters;
    if (h < S6_HIST) {
        st->cost_hist[h] = st->cost, st->pcg_it_hist[h] = 0, st->pcg_rel_hist[h] = 1.f, st->pcg_tol_hist[h] = sqrtf(f.tol2);
        st->valid_hist[h] = (unsigned int)st->valid, st->stop_hist[h] = 0, st->hist_n = h + 1;
    }
    st->gn_iters = h + 1, st->gn_solves = h + 1, st->cur = h;
    st->tol2 = f.tol2, st->pcg_last_it = 0, st->pcg_done = 0;
    st->ew_gamma = f.ew_gamma, st->ew_min2 = f.ew_min2, st->ew_max2 = f.ew_max2, st->ew_slot = f.ew_slot;
}

constexpr int S6_SORT_MAX = 4096;  // [used by: _graph, _pattern — the buffers s6_sort_lds sorts]

// bitonic sort of n <= S6_SORT_MAX keys in LDS by one 256-thread workgroup (buf holds the next power of two, padded with
// 0xffffffff)
// Stages with a stride of at most 64 keep a wave inside its own 128-key blocks (compare-exchange i = tid + 256 m touches the
// 2-stride-aligned block of key 2 i): the wave's LDS operations are ordered among themselves, no workgroup barrier is needed
// between such stages — 10 barriers instead of 66 for 2 048 keys.
// [called by: _graph (s6_permute_kernel: a node's vertices), _pattern (s6_pattern_kernel: a node's rows)]
__device__ __forceinline__ void s6_sort_lds(uint32_t* buf, int n2, int tid) {
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2 / 2; i += 256) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t x = buf[lo], y = buf[hi];
                if ((x > y) == up) buf[lo] = y, buf[hi] = x;
            }
            // the next stage leaves the wave's blocks (or there is none): everybody waits; else only the compiler does
            const int next = stride > 1 ? stride >> 1 : size;  // (after stride 1 comes size 2 x size with stride = size)
            if (stride > 64 || next > 64 || (stride == 1 && size == n2)) __syncthreads();
            else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"), __builtin_amdgcn_wave_barrier(), __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
}

// the plan's shape, which the pattern writes and the assembly walks  [used by: _pattern (S6_UNITS), _assemble (both)]
constexpr int S6_MAXSLOT = S6_ROW_BLOCKS;  // plan capacity of a block row
constexpr int S6_UNITS = 256;           // work units of a node's assembly = threads of its workgroup

}  // namespace

// a kernel template by the smaller K in {4, 8} that holds the plan's k  [used by: _graph, _update; _linearise, whose kernel has a second template argument, spells the same choice out]
#define K6DISPATCH(kernel, k, ...)            \
    do {                                      \
        if ((k) <= 4) kernel<4> __VA_ARGS__;  \
        else kernel<8> __VA_ARGS__;           \
    } while (0)

// DFA_S6_TIMING (development builds only): per-workgroup phase clocks of the pattern (tools/ns_pattern_phases.py) and of
// the assembly (tools/ns_assemble_phases.py)  [used by: _pattern, _assemble].  A device buffer cannot be shared between
// units, so each of the two has its own, S6_TIMING_BUFFER(reader), with its own exported reader — 16 clocks per workgroup.
#ifdef DFA_S6_TIMING
#define S6_TICK(var) const unsigned long long var = clock64()
#define S6_TIMING_BUFFER(reader)                                                                                    \
    __device__ unsigned long long s6_tbuf[16384 * 16];                                                              \
    extern "C" __attribute__((visibility("default"))) int reader(unsigned long long* out, int n) {                  \
        return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(s6_tbuf), sizeof(unsigned long long) * 16 * (size_t)n);     \
    }
#else
#define S6_TICK(var)
#define S6_TIMING_BUFFER(reader)
#endif

#pragma GCC visibility push(hidden)  // internal to the library: nothing here joins its exported symbols
// solve6_pattern.hip: s6_pattern_kernel and s6_rslot_kernel, the end of s6_build_graph (solve6_graph.hip)
hipError_t s6_launch_pattern(const Solve6View& s, Solve6State* state, hipStream_t st);
#pragma GCC visibility pop

}  // namespace dfa
