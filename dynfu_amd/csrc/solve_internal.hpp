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
