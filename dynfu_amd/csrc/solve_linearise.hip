// solve_linearise.hip — the linearisation of the reference-mode solve (formulation: solve.hpp): robust weights (Tukey for
// the data rows; Huber for interface parity), residuals into the tails of the row records (solve_rows.hpp), the cost
// and the Gauss-Newton control in ONE launch per Gauss-Newton iteration; and the regradient that replaces a linearisation
// and an assembly while the robust weights are frozen.
#include <hip/hip_runtime.h>

#include "dev_switch.hpp"
#include "dq_device.hpp"
#include "solve.hpp"
#include "solve_internal.hpp"
#include "solve_rows.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------
// linearisation, one launch per Gauss-Newton iteration:
//   [outer-iteration start only] robust weights: Tukey biweight of the current warp error for
//       the data rows (opt_solver.cpp:204-231; warp(c) = calcDQB(c)(c) with node transforms
//       DQ(t_i) * dg_se3_i, :270-285 + node.cpp:19-23), w_reg^2 for the regularisation rows (:30);
//   residual  e_r = b_r - sum_j w_rj t_{n_rj}  -> tail (e, tau) of the row's packed record;
//   cost      sum tau |e|^2: one partial per workgroup, added in index order (deterministic) by ONE workgroup that also
//       runs the Gauss-Newton control logic — no separate control launch.  Which workgroup:
//       * the launch's own LAST workgroup to arrive (agent-scope release/acquire around a ticket counter): the closing
//         evaluation, launches with gn_tol > 0 (their control sets `done`, which the assembly reads at entry) and
//         launches that keep the stored weights;
//       * the HAND-OFF (LineariseArgs::handoff; solve_lin_handoff, solve.hpp): a re-weighting linearisation with
//         gn_tol == 0 ends with its rows — thread 0 of each workgroup stores the workgroup's partial cost and partial
//         maximum (as a double for the booking, as a float for the assembly's workgroups) with plain stores and the
//         kernel ends: no wait for publication, no tickets, no last workgroup.  The
//         assembly launch behind it (solve_assemble.hip) forms amax in every workgroup from the per-workgroup maxima and
//         books the cost in one extra workgroup, with the code the last workgroup runs here (lin_sum_partials,
//         lin_book_cost: solve_internal.hpp), so cost and amax keep their bits.  The launch boundary orders what the
//         tail ordered by hand (measured: profiles/r12_linearise_tail.md).  What that form had to settle:
//           - a launch that returns at entry (converged == 1) has written no partials: SolveState::lin_pending is set by
//             block 0 of a launch that really runs and consumed by the booking workgroup, which books nothing without it;
//           - `converged == 2` is cleared for the new outer iteration by block 0 AT ENTRY, not by the booking workgroup:
//             the assembly's workgroups read `converged` at entry, and no workgroup of a re-weighting launch here
//             branches on the value 2 (they test `== 1`), so the early clear races with nothing;
//           - the state block is complete behind the assembly, which is where the statistics are read; the assembly's
//             timing bracket contains the booking.

// (the row's own data — graph slots n, w, canonical point c, live point l — is the caller's: already in registers)
// a row's sum_j w_j t_{n_j} and largest |w_j|, one present slot after the other in slot order
struct RowSums {
    float sx = 0.f, sy = 0.f, sz = 0.f, wm = 0.f;
    __device__ __forceinline__ void add(float w, float tx, float ty, float tz) {
        sx += w * tx, sy += w * ty, sz += w * tz, wm = fmaxf(wm, fabsf(w));
    }
};

// Also forms the row's residual e = b - sum_j w_j t_{n_j} and its largest |w_j| from the translations it gathers: the
// residual needs the same numbers, and behind the store of the weight the compiler would have to gather them again.  The
// residual is complete with the last gather, ahead of the arithmetic: e takes the registers of b, and nothing of the
// 3 k translations stays live.  B_AHEAD = false (the caller has not loaded b yet): e returns the sum, the caller subtracts.
template <int K, bool B_AHEAD>
__device__ __forceinline__ float tukey_weight_of(const SolveView& s, const int (&n)[K], const float (&w)[K], f3 c, f3 l, float tukey_offset,
                                                 float psi_data, f3 b, f3& e, float& wm) {
    RowSums rs;
    DQ sum = dq_identity();
    // the neighbours' translations and transforms four at a time, by unconditional loads (an absent neighbour reads node 0
    // and is skipped): loads inside the `if` were k dependent round trips
#pragma unroll
    for (int h = 0; h < K; h += 4) {
        float tx[4], ty[4], tz[4];
        DQ q[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int nn = n[h + jj] >= 0 ? n[h + jj] : 0;
            tx[jj] = s.t[3 * nn], ty[jj] = s.t[3 * nn + 1], tz[jj] = s.t[3 * nn + 2];
            q[jj]  = dq_load(s.node_dq + 8 * (size_t)nn);
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            if (n[h + jj] >= 0) rs.add(w[h + jj], tx[jj], ty[jj], tz[jj]);
        if (h + 4 >= K) e = B_AHEAD ? mk3(b.x - rs.sx, b.y - rs.sy, b.z - rs.sz) : mk3(rs.sx, rs.sy, rs.sz), wm = rs.wm;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            if (n[h + jj] >= 0) {
                const DQ cur = dq_mul(dq_from_translation(tx[jj], ty[jj], tz[jj]), q[jj]);
                sum          = dq_mul(sum, dq_scale(cur, w[h + jj]));
            }
        }
    }
    const f3 warped = dq_transform(dq_normalize(sum), c);
    const float ex = l.x - warped.x, ey = l.y - warped.y, ez = l.z - warped.z;
    // calcTukeyBiweight (:204-212)
    const float d = sqrtf(ex * ex + ey * ey + ez * ez) / tukey_offset;
    if (d < psi_data) {
        const double q = 1.0 - ((double)d * (double)d) / ((double)psi_data * (double)psi_data);
        return (float)(q * q);
    }
    return 0.f;
}
// Huber weights (opt_solver.cpp:233-268): computed for interface parity, energy.t:70 never uses them
__device__ __forceinline__ void huber_node(const SolveView& s, int i, float psi_reg) {
    const DQ dq_i = dq_mul(dq_from_translation(s.t[3 * i], s.t[3 * i + 1], s.t[3 * i + 2]),
                           dq_load(s.node_dq + 8 * (size_t)i));
    float h = 0.f;
    for (int j = 0; j < s.k; ++j) {
        const int m = s.reg_idx[(size_t)i * s.k + j];
        if (m < 0) break;
        const f3 pm   = mk3(s.node_pos[3 * m], s.node_pos[3 * m + 1], s.node_pos[3 * m + 2]);
        const DQ dq_m = dq_mul(dq_from_translation(s.t[3 * m], s.t[3 * m + 1], s.t[3 * m + 2]),
                               dq_load(s.node_dq + 8 * (size_t)m));
        const f3 pa = dq_transform(dq_i, pm), pb = dq_transform(dq_m, pm);
        const float ex = pa.x - pb.x, ey = pa.y - pb.y, ez = pa.z - pb.z;
        const float err = sqrtf(ex * ex + ey * ey + ez * ez);
        h               = fabsf(err) <= psi_reg ? 1.f : psi_reg / fabsf(err);  // last neighbour wins (:263)
    }
    s.huber[i] = h;
}
__global__ __launch_bounds__(256) void huber_kernel(SolveView s, float psi_reg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < s.D) huber_node(s, i, psi_reg);
}

struct LineariseArgs {
    int update_weights;  // first linearisation of an outer iteration
    int mode;            // 0 first of outer, 1 later GN iteration, 2 final cost only
    float gn_tol, tukey_offset, psi_data, w_reg_sq;
    long long* iters_total;  // mode 2, optional (device): += the solve's PCG iterations
    int handoff;      // the launch ends with its rows: the assembly launch behind it books the cost (header comment)
    float huber_psi;  // > 0: also evaluate the nodes' Huber weights at the current t (the last outer iteration's
                      // preNonlinearSolve, opt_solver.cpp:135-140; a launch of its own before)
};

#ifdef DFA_PCG_PROFILE  // development builds: a workgroup's life in the linearisation (tools/ref_linearise_phases.py)
// per workgroup, 100 MHz ticks: start | rows finished | partial published, ticket taken | exit; the last workgroup also:
// start of the partial loads | end of the tree | end of the state update; [7] = 1 marks the last workgroup
__device__ unsigned long long lin_tbuf[1024 * 8];
extern "C" __attribute__((visibility("default"))) int dfa_dev_lin_timing(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(lin_tbuf), sizeof(unsigned long long) * 8 * (size_t)n);
}
#define LIN_MARK(i) (lw_[i] = wall_clock64())
#define LIN_MARKS_OUT(last)                                                          \
    do {                                                                             \
        if (threadIdx.x == 0 && a.mode != 2) {                                       \
            lw_[3 + 3 * (last)] = wall_clock64(), lw_[7] = (last);                   \
            if (last) lw_[3] = lw_[6];                                               \
            for (int i_ = 0; i_ < 8; ++i_) lin_tbuf[8 * blockIdx.x + i_] = lw_[i_];  \
        }                                                                            \
    } while (0)
#else
#define LIN_MARK(i)
#define LIN_MARKS_OUT(last)
#endif

// What a row's arithmetic reads of the row itself — graph slots, right-hand side, and for its robust weight the canonical
// and the live point (data rows of a re-weighting linearisation) or the stored weight — asked for together, ahead of the
// gathers (translations, transforms) that depend on the slots.
template <int K>
struct LinRow {
    int n[K];
    float w[K];
    float bx, by, bz, tau;
    f3 c, l;
};
// WITH_B = false leaves out the right-hand side (lin_row_finish<K, false> asks for it beside its gathers and needs it only
// behind the weight's arithmetic): three registers fewer held across the row in front.
template <int K, bool WITH_B>
__device__ __forceinline__ void lin_row_load(const SolveView& s, size_t r, int update_weights, LinRow<K>& q) {
    load_row_graph<K>(s, r, q.n, q.w);
    q.bx = q.by = q.bz = 0.f;
    if (WITH_B) q.bx = s.rb[3 * r], q.by = s.rb[3 * r + 1], q.bz = s.rb[3 * r + 2];
    q.tau = 0.f, q.c = q.l = mk3(0.f, 0.f, 0.f);
    if (!update_weights) q.tau = s.rtau[r];
    else if (r < (size_t)s.N) {
        q.c = mk3(s.canon[3 * r], s.canon[3 * r + 1], s.canon[3 * r + 2]);
        q.l = mk3(s.live[3 * r], s.live[3 * r + 1], s.live[3 * r + 2]);
    }
}
// ... and the row's arithmetic: weight, residual into the record's tail, the row's share of the cost added to c, its
// largest matrix addend into amax.  The k translations by unconditional loads (an absent neighbour reads node 0 and is
// skipped; with the loads inside `if (n >= 0)` it was k dependent round trips), ONCE per row: a data row of a re-weighting
// linearisation has its sums from its Tukey weight's gather.
template <int K, bool B_AHEAD>
__device__ __forceinline__ void lin_row_sums(const SolveView& s, const int (&n)[K], const float (&w)[K], f3 b, f3& e, float& wm) {
    float tx[K], ty[K], tz[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int nn = n[j] >= 0 ? n[j] : 0;
        tx[j] = s.t[3 * nn], ty[j] = s.t[3 * nn + 1], tz[j] = s.t[3 * nn + 2];
    }
    RowSums rs;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (n[j] >= 0) rs.add(w[j], tx[j], ty[j], tz[j]);
    e = B_AHEAD ? mk3(b.x - rs.sx, b.y - rs.sy, b.z - rs.sz) : mk3(rs.sx, rs.sy, rs.sz), wm = rs.wm;
}
__device__ __forceinline__ void lin_row_store(const SolveView& s, size_t r, f3 e, float tau, float wm, double& c, float& amax) {
    amax = fmaxf(amax, tau * wm * wm);
    // tail of the packed row record (head = k ids + k weights, written once per frame)
    *(float4*)(s.re + r * (size_t)solve_rec_words(s.k) + solve_rec_tail(s.k)) = make_float4(e.x, e.y, e.z, tau);
    c += (double)tau * ((double)e.x * e.x + (double)e.y * e.y + (double)e.z * e.z);
}
template <int K, bool WITH_B>
__device__ __forceinline__ void lin_row_finish(const SolveView& s, size_t r, const LineariseArgs& a, const LinRow<K>& q, double& c, float& amax) {
    float tau = q.tau, wm;
    f3 e;
    const f3 b = WITH_B ? mk3(q.bx, q.by, q.bz) : mk3(s.rb[3 * r], s.rb[3 * r + 1], s.rb[3 * r + 2]);
    if (a.update_weights && r < (size_t)s.N) tau = tukey_weight_of<K, WITH_B>(s, q.n, q.w, q.c, q.l, a.tukey_offset, a.psi_data, b, e, wm);
    else {
        lin_row_sums<K, WITH_B>(s, q.n, q.w, b, e, wm);
        if (a.update_weights) tau = a.w_reg_sq;
    }
    if (a.update_weights) s.rtau[r] = tau;
    if (!WITH_B) e = mk3(b.x - e.x, b.y - e.y, b.z - e.z);
    lin_row_store(s, r, e, tau, wm, c, amax);
}
// The same for a row on its own (the plain loop): nothing asked for ahead, so nothing held across the arithmetic either —
// the graph slots first, the points or the stored weight behind them, the right-hand side last.
template <int K>
__device__ __forceinline__ void lin_row_plain(const SolveView& s, size_t r, const LineariseArgs& a, double& c, float& amax) {
    int n[K];
    float w[K];
    load_row_graph<K>(s, r, n, w);
    float tau, wm;
    f3 e;
    if (a.update_weights && r < (size_t)s.N) {
        const f3 cp = mk3(s.canon[3 * r], s.canon[3 * r + 1], s.canon[3 * r + 2]);
        const f3 l  = mk3(s.live[3 * r], s.live[3 * r + 1], s.live[3 * r + 2]);
        tau         = tukey_weight_of<K, false>(s, n, w, cp, l, a.tukey_offset, a.psi_data, mk3(0.f, 0.f, 0.f), e, wm);
    } else {
        tau = a.update_weights ? a.w_reg_sq : s.rtau[r];
        lin_row_sums<K, false>(s, n, w, mk3(0.f, 0.f, 0.f), e, wm);
    }
    if (a.update_weights) s.rtau[r] = tau;
    e = mk3(s.rb[3 * r] - e.x, s.rb[3 * r + 1] - e.y, s.rb[3 * r + 2] - e.z);
    lin_row_store(s, r, e, tau, wm, c, amax);
}

// TWO: a thread's first two rows with the second row's own loads (lin_row_load) ahead of the first row's arithmetic.  The
// grid is capped at LIN_MAX_BLOCKS x 256 threads — raising the cap would regroup the cost's partial sums — so a plan of
// more rows than that (C2: 262 144 data rows fill it, the 8 192 regularisation rows are a second trip of blocks 0-31) took
// that trip's loads only when the first row was finished: a dependent round trip in front of the last workgroup's serial
// tail, which the assembly behind this launch waits for.  Same row -> thread mapping, same order of a thread's adds into
// c and amax: the same bits (tests/test_gpu_linearise_two_rows.py).  Third and later trips: the plain loop.
template <int K, bool TWO>
__global__ __launch_bounds__(256) void linearise_kernel(SolveView s, SolveState* __restrict__ st,
                                                        double* __restrict__ cost_partials,
                                                        unsigned int* __restrict__ ticket /*[LIN_SHARDS+1]*/,
                                                        LineariseArgs a) {
    __shared__ double wsum[4];
    __shared__ int is_last;
    if (a.huber_psi > 0.f)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.D; i += gridDim.x * blockDim.x) huber_node(s, i, a.huber_psi);
    if (a.mode == 2) {
        // the closing evaluation also composes the result: dg_se3_i <- DQ(0,0,0,t_i) * dg_se3_i (opt_solver.cpp:270-285,
        // node.cpp:19-23) — t is final here; a launch of its own before
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < s.D; i += gridDim.x * blockDim.x) {
            const DQ out = dq_mul(dq_from_translation(s.t[3 * i], s.t[3 * i + 1], s.t[3 * i + 2]),
                                  dq_load(s.node_dq + 8 * (size_t)i));
            dq_store(s.node_dq_out + 8 * (size_t)i, out);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.iters_total) *a.iters_total += st->pcg_iters;
    }
    // after convergence t no longer changes: weights, residual records and cost of this linearisation exist already.
    // That includes the solve's closing evaluation (mode 2) when an iteration ran: the flag is set by a PCG that found
    // its gradient at the floor and left t where the linearisation before it had evaluated the cost.
    if (st->converged == 1 || (st->converged && !a.update_weights)) {
        if (a.mode != 2 || (st->have_initial && !st->cost_stale)) return;
    }
    if (a.handoff && blockIdx.x == 0 && threadIdx.x == 0) {  // (header comment: what the hand-off had to settle)
        if (st->converged == 2) st->converged = 0;  // a new outer iteration
        st->lin_pending = 1;
    }
#ifdef DFA_PCG_PROFILE
    unsigned long long lw_[8] = {};
    LIN_MARK(0);
#endif
    const size_t R = (size_t)s.N + (size_t)s.D * s.k;
    double c       = 0.0;
    float amax     = 0.f;  // re-weighting linearisations: the largest addend tau w_a w_b any row brings to the normal matrix
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t r_first      = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (TWO) {
        if (r_first < R) {
            const size_t r1 = r_first + stride;
            LinRow<K> q0, q1;
            lin_row_load<K, true>(s, r_first, a.update_weights, q0);
            if (r1 < R) lin_row_load<K, false>(s, r1, a.update_weights, q1);
            lin_row_finish<K, true>(s, r_first, a, q0, c, amax);
            if (r1 < R) lin_row_finish<K, false>(s, r1, a, q1, c, amax);
            r_first = r1 + stride;  // (past R if there was no second row)
        }
    }
    for (size_t r = r_first; r < R; r += stride) {
        lin_row_plain<K>(s, r, a, c, amax);
    }
    c = wave_sum_all(c);
    __shared__ float wmax[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c, wmax[threadIdx.x >> 6] = amax;
    __syncthreads();
    LIN_MARK(1);
    if (a.handoff) {  // the launch ends here; the assembly launch behind it takes the rest
        if (threadIdx.x == 0) {
            cost_partials[blockIdx.x]                  = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
            const float mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
            cost_partials[LIN_MAX_BLOCKS + blockIdx.x] = (double)mx;
            lin_max_floats(cost_partials)[blockIdx.x]  = mx;
        }
        LIN_MARK(2);
        LIN_MARKS_OUT(0);
        return;
    }
    if (threadIdx.x == 0) {
        // publish the partial write-through (sc1) — no release fence, which would write back the
        // whole L2's dirty record tails — then arrive: shard counter first, top counter for the
        // last arriver of each shard
        __hip_atomic_store(&cost_partials[blockIdx.x], (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        if (a.update_weights)  // (the second half of the array: one maximum per workgroup)
            __hip_atomic_store(&cost_partials[LIN_MAX_BLOCKS + blockIdx.x], (double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int shard   = blockIdx.x % LIN_SHARDS;
        const unsigned int members = (gridDim.x - shard + LIN_SHARDS - 1) / LIN_SHARDS;
        const unsigned int nshards = min((unsigned int)LIN_SHARDS, gridDim.x);
        int last                   = 0;
        if (__hip_atomic_fetch_add(&ticket[shard], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1) {
            __hip_atomic_store(&ticket[shard], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
            if (__hip_atomic_fetch_add(&ticket[LIN_SHARDS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                nshards - 1) {
                __hip_atomic_store(&ticket[LIN_SHARDS], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = 1;
            }
        }
        is_last = last;
    }
    __syncthreads();
    LIN_MARK(2);
    if (!is_last) {
        LIN_MARKS_OUT(0);
        return;
    }
    LIN_MARK(4);

    // last workgroup: ordered sum of the partials + Gauss-Newton control
    __shared__ double sm[256];
    __shared__ double smx[256];
    lin_sum_partials<true>(cost_partials, gridDim.x, a.update_weights != 0, sm, smx);
    LIN_MARK(5);
    if (threadIdx.x == 0) lin_book_cost(st, sm[0], smx[0], a.update_weights, a.mode, a.gn_tol, true);
    LIN_MARKS_OUT(1);
}

// ------------------------------------------------------------------------------------------
// launchers

int solve_residual_blocks(const SolveView& s) { return lin_blocks(s.N, s.D, s.k); }
size_t solve_cost_partials_len() { return LIN_PARTIALS_LEN; }

// which template K takes the two-row form: where its second row's registers leave the kernel's waves per SIMD as they are
constexpr bool lin_two_rows(int K) { return K == 4; }

template <int K>
static void launch_linearise(const SolveView& s, SolveState* state, double* cost_partials, unsigned int* ticket, const LineariseArgs& a,
                             int nb, hipStream_t st) {
#ifdef DFA_DEV_AB  // DFA_LIN_TWO_ROWS=0 / 1 (development builds): either form for every k (A/B, tests)
    if (dev_env_int("DFA_LIN_TWO_ROWS", lin_two_rows(K)) != 0) linearise_kernel<K, true><<<nb, 256, 0, st>>>(s, state, cost_partials, ticket, a);
    else linearise_kernel<K, false><<<nb, 256, 0, st>>>(s, state, cost_partials, ticket, a);
#else
    linearise_kernel<K, lin_two_rows(K)><<<nb, 256, 0, st>>>(s, state, cost_partials, ticket, a);
#endif
}

hipError_t solve_linearise(const SolveView& s, SolveState* state, double* cost_partials, unsigned int* ticket,
                           int update_weights, int mode, float gn_tol, float tukey_offset, float psi_data,
                           float w_reg_sq, float huber_psi, long long* iters_total, bool handoff, hipStream_t st) {
    const int nb = solve_residual_blocks(s);
    if (handoff && !solve_lin_handoff(update_weights, mode, gn_tol)) return hipErrorInvalidValue;
    LineariseArgs a{update_weights, mode, gn_tol, tukey_offset, psi_data, w_reg_sq, iters_total, handoff ? 1 : 0, huber_psi};
    if (s.k <= 4) launch_linearise<4>(s, state, cost_partials, ticket, a, nb, st);
    else if (s.k <= 8) launch_linearise<8>(s, state, cost_partials, ticket, a, nb, st);
    else launch_linearise<16>(s, state, cost_partials, ticket, a, nb, st);
    return hipGetLastError();
}

hipError_t solve_huber(const SolveView& s, float psi_reg, hipStream_t st) {
    huber_kernel<<<(s.D + 255) / 256, 256, 0, st>>>(s, psi_reg);
    return hipGetLastError();
}

// g = g_base - A (t - t_base): a thread per row over the slot-major ELL (entry q of row a at [q * D + a]: coalesced)
__global__ __launch_bounds__(256) void regradient_kernel(SolveView s, SolveState* __restrict__ st) {
    if (st->done || st->converged) return;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a == 0) st->cost_stale = 1, st->weights_fresh = 0;  // (a floor hit now ends this outer iteration only)
    if (a >= s.D) return;
    const int cnt = s.ell_cnt[a];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int q = 0; q < cnt; ++q) {
        const float2 e = s.ell[(size_t)q * s.D + a];
        const int col  = __float_as_int(e.y);
        sx = fmaf(e.x, s.t[3 * col] - s.t_base[3 * col], sx);
        sy = fmaf(e.x, s.t[3 * col + 1] - s.t_base[3 * col + 1], sy);
        sz = fmaf(e.x, s.t[3 * col + 2] - s.t_base[3 * col + 2], sz);
    }
    s.g[3 * a] = s.g_base[3 * a] - sx, s.g[3 * a + 1] = s.g_base[3 * a + 1] - sy, s.g[3 * a + 2] = s.g_base[3 * a + 2] - sz;
}

hipError_t solve_regradient(const SolveView& s, SolveState* state, hipStream_t st) {
    regradient_kernel<<<(s.D + 255) / 256, 256, 0, st>>>(s, state);
    return hipGetLastError();
}

}  // namespace dfa
