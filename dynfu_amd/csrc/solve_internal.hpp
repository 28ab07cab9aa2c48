// solve_internal.hpp — what more than one unit of the reference-mode solve uses (solve_graph / _linearise / _assemble /
// _pcg / _pcg_launched / _pcg_team .hip) and nobody else: the k dispatch of the row kernels, the workgroup sums and the
// phase marks of the PCG forms, the opt-in to a CU's whole LDS, and the launchers that route_pcg (solve_pcg.hip) chooses
// between.  Internal to those six files; the launchers the C ABI calls are in solve.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"
#include "solve.hpp"

namespace dfa {

// Workgroup total: DPP wave totals (float) -> one LDS slot per wave -> ONE barrier -> every
// thread adds the NWAVES partials in double.  `red` must alternate between two buffers on
// successive calls so that no second barrier is needed to protect the slots.
template <int NWAVES>
__device__ __forceinline__ double block_sum(float v, float* red) {
    const float w = wave_total(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < NWAVES; ++i) tot += (double)red[i];
    return tot;
}

// DFA_PCG_PROFILE builds accumulate shader cycles per PCG phase (thread 0) into SolveState::prof
#ifdef DFA_PCG_PROFILE
#define PROF_MARK(i)                      \
    do {                                  \
        const long long now_ = clock64(); \
        pc_[i] += now_ - last_;           \
        last_ = now_;                     \
    } while (0)
#else
#define PROF_MARK(i)
#endif

// float flavour (fewer registers; used by the register-resident kernel)
template <int NWAVES>
__device__ __forceinline__ float block_sum_f(float v, float* red) {
    const float w = wave_total(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < NWAVES; ++i) tot += red[i];
    return tot;
}

// a row kernel by the smallest template K in {4, 8, 16} that holds the plan's k
#define KDISPATCH(kernel, k, ...)                      \
    do {                                               \
        if ((k) <= 4) kernel<4> __VA_ARGS__;           \
        else if ((k) <= 8) kernel<8> __VA_ARGS__;      \
        else kernel<16> __VA_ARGS__;                   \
    } while (0)

// ------------------------------------------------------------------------------------------
// The linearisation's cost: one partial per workgroup in cost_partials[0, nb), for re-weighting launches one maximum per
// workgroup in cost_partials[LIN_MAX_BLOCKS, LIN_MAX_BLOCKS + nb) (linearise_kernel, solve_linearise.hip), summed in index
// order and booked into SolveState by ONE 256-thread workgroup: the linearisation's own last workgroup, or the extra
// workgroup of the assembly launch behind it (solve_assemble.hip) — the code below either way, hence the same bits.
// Where the launch hands its tail to the assembly, the same maxima stand once more as floats behind the two arrays
// (lin_max_floats): every assembly workgroup reads all of them, one 16-byte load per thread.
constexpr int LIN_SHARDS     = 32;    // ticket counters: one device-scope atomic costs ~11 ns when
constexpr int LIN_MAX_BLOCKS = 1024;  // serialised on one word, so arrivals are sharded 2-level
constexpr size_t LIN_PARTIALS_LEN = 2 * LIN_MAX_BLOCKS + LIN_MAX_BLOCKS / 2;  // doubles: costs, maxima, maxima as floats
__host__ __device__ inline float* lin_max_floats(double* cost_partials) { return reinterpret_cast<float*>(cost_partials + 2 * LIN_MAX_BLOCKS); }
__host__ __device__ inline const float* lin_max_floats(const double* cost_partials) {
    return reinterpret_cast<const float*>(cost_partials + 2 * LIN_MAX_BLOCKS);
}
// workgroups of a linearisation: one per 256 rows, capped (a larger plan's threads take several rows)
__host__ __device__ inline int lin_blocks(int N, int D, int k) {
    const size_t R  = (size_t)N + (size_t)D * k;
    const size_t nb = (R + 255) / 256;
    return (int)(nb < (size_t)LIN_MAX_BLOCKS ? nb : (size_t)LIN_MAX_BLOCKS);
}

// SAME_LAUNCH: the partials were published by other workgroups of the launch that reads them, so the loads go past the
// L2 (~2 us each); behind a launch boundary they are plain loads.  Either way this is one workgroup that others wait for:
// all of a thread's partials in flight together (LIN_MAX_BLOCKS / 256 = 4 per array; a load-wait-add loop was four
// dependent round trips), clamped addresses, masked sums in index order.  Cost in sm[0], maximum in smx[0] on return.
template <bool SAME_LAUNCH>
__device__ __forceinline__ void lin_sum_partials(const double* cost_partials, unsigned int nb, bool with_max, double* sm /*[256]*/,
                                                 double* smx /*[256]*/) {
    double acc = 0.0, mx = 0.0;
    constexpr int Q = LIN_MAX_BLOCKS / 256;
    double cq[Q], mq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const unsigned int i = min(threadIdx.x + 256u * q, nb - 1);
        if constexpr (SAME_LAUNCH) {
            cq[q] = __hip_atomic_load(&cost_partials[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mq[q] = with_max ? __hip_atomic_load(&cost_partials[LIN_MAX_BLOCKS + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        } else {
            cq[q] = cost_partials[i];
            mq[q] = with_max ? cost_partials[LIN_MAX_BLOCKS + i] : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (threadIdx.x + 256u * q < nb) acc += cq[q], mx = fmax(mx, mq[q]);
    sm[threadIdx.x] = acc, smx[threadIdx.x] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o], smx[threadIdx.x] = fmax(smx[threadIdx.x], smx[threadIdx.x + o]);
        __syncthreads();
    }
}

// ... and the Gauss-Newton control that goes with the cost (one thread).  mode: 0 first linearisation of an outer
// iteration, 1 later Gauss-Newton iteration, 2 the closing evaluation.  clear_outer: this launch also ends a
// `converged == 2` (a new outer iteration) — not for the assembly's booking workgroup, whose launch reads the flag at entry.
__device__ __forceinline__ void lin_book_cost(SolveState* st, double cost, double amax, int update_weights, int mode, float gn_tol,
                                              bool clear_outer) {
    if (update_weights) st->amax = (float)amax;
    if (!st->have_initial) st->initial_cost = cost, st->have_initial = 1;
    if (mode == 0) st->done = 0;
    // Gauss-Newton early-out: relative cost decrease of the previous step below gn_tol
    if (mode == 1 && !st->done && gn_tol > 0.f && (st->cost - cost) <= (double)gn_tol * st->cost) st->done = 1;
    st->cost       = cost;
    st->final_cost = cost;
    st->cost_stale = 0;
    // robust weights evaluated at THIS t: a gradient at the floor now means the whole solve has converged (with
    // stale weights it only ends the current outer iteration: the next one re-weights at the moved t)
    if (mode != 2) st->weights_fresh = update_weights;
    if (clear_outer && mode != 2 && update_weights && st->converged == 2) st->converged = 0;  // a new outer iteration
}

// the persistent PCG kernels ask for (nearly) a CU's whole LDS
template <class Kernel>
static hipError_t allow_big_lds(Kernel* k) {
    return allow_dynamic_lds((const void*)k, 160 * 1024 - 1024);  // once per (device, kernel)
}

#pragma GCC visibility push(hidden)  // internal to the library: nothing here joins its exported symbols
// solve_pcg_launched.hip: one launch per iteration across many workgroups, chunks replayed as HIP graphs
hipError_t launch_mb_pcg(const SolveView& s, SolveState* state, int max_iter, float pcg_tol, int* host_flag,
                         MbGraphCache* gc, hipStream_t st);
// solve_pcg_team.hip: three teams of persistent workgroups and their guard launch
hipError_t launch_team_pcg(const SolveView& s, SolveState* state, int max_iter, float pcg_tol, TeamPcg* tp, hipStream_t st);
#pragma GCC visibility pop

}  // namespace dfa
