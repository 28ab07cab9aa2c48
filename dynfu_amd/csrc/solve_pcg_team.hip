// solve_pcg_team.hip — the block-Jacobi PCG of the reference-mode solve by three teams of persistent workgroups, one
// coordinate per team and one XCD per team, with the guard launch behind every team launch and the per-device turn-taking
// of team launches from different streams.  route_pcg (solve_pcg.hip) sends plans of 2 049 .. 19 584 nodes here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "dev_switch.hpp"
#include "device_math.hpp"
#include "pcg_rules.hpp"
#include "solve.hpp"
#include "solve_internal.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------
// PCG by three TEAMS of persistent workgroups, one coordinate per team, every team confined to ONE XCD
// (plans of 2 049 nodes up to the bound of solve_team_pcg_fits, 19 584 nodes: C3, C4, the adaptor's frames; rows longer
// than J x TEAM_E entries make the first launch give up and the plan fall back to the launched form).
//
// The launched form (solve_pcg_launched.hip) pays a kernel boundary per iteration: ~5.8 us for an iteration whose arithmetic takes a fraction of
// a microsecond, and the host has to guess how many launches to enqueue (192 launches for 105 iterations per C3 frame).
// A grid barrier across the chip costs more than the boundary (L2 write-back + invalidate between XCDs: ~15 us); a barrier
// among workgroups that share ONE L2 does not (tools/microbench_xcd_barrier.hip).  J^T J = A (x) I_3 is three independent
// scalar systems with the same matrix (as the register-resident kernel, solve_pcg.hip, solves them): coordinate c is solved by the
// TEAM_W workgroups that the dispatcher placed on XCD c, one per CU (the launch asks for more than half a CU's LDS) — every
// workgroup reads its XCC_ID, takes a rank in its team by an atomic counter and leaves if the team is full or the XCD is
// not 0..2: the placement is counted, never assumed.
//
// One synchronisation per iteration (Chronopoulos-Gear form, the recurrences of pcg_mb_step_kernel), one gathered vector
// pair: a member owns R = ceil(D / TEAM_W) rows; J = TEAM_NT / R threads share a row and keep their entries' values,
// columns and the REPLICA of u at the entry's column in registers for the whole solve:
//   wait(round i)            gamma_i, delta_i = sums of the members' partials (carried by the flag words themselves)
//   beta_i, alpha_i          the same bits in every member (same words, same summation order)
//   LDS <- (m_i, t_(i-1))    the pair every row owner published before it raised its flag: D x 8 bytes, coalesced, from L2
//   per entry                t_i[col] = m_i[col] + beta_i t_(i-1)[col];  u_(i+1)[col] = u_i[col] - alpha_i t_i[col]  (replica: the
//                            owner of row col does the same arithmetic on the same numbers);  w_(i+1)[a] += val u_(i+1)[col]
//   row owner                p, s, x, r, t, u as in pcg_mb_step_kernel;  m_(i+1) = M^-1 w_(i+1);  partial (r, u), (w, u)
//   publish                  (m_(i+1), t_i) of the own rows, s_waitcnt vmcnt(0), workgroup barrier, then the member's flag
//                            words {round i + 1, partial}
// Where the longest row of the matrix fits TEAM_E_TREG slots per thread, t's replica at the entry's column lives in a register
// as well and m ALONE is exchanged (half the copy, 4-byte gathers): team_member<16, true>; longer rows: team_member<20, false>.
//
// How the exchange stays inside the XCD's L2.  Agent-scope atomics (sc1) are the textbook tool and were the first version:
// every such load is a trip over the fabric (1.2-1.5 us measured here; 2 MB of them per team and iteration for the vector
// copy) and an iteration cost 6.7 us — no better than a launch.  An agent-scope acquire fence + plain loads: buffer_inv sc1
// from 1 500 waves, 30 us per iteration.  `buffer_inv sc0` + plain loads: leaves the vector L1 alone outside threadgroup-split
// mode — the pollers never saw a flag, the teams timed out and the guard launch took over (which is how that was found).
// What works: PLAIN stores and PLAIN loads, with NO ADDRESS READ TWICE by a CU inside a launch.  A plain store is in the
// XCD's L2 once acknowledged (the vector L1 writes through and does not allocate on stores); a plain load of an address this CU
// has not read since the kernel began (the L1 starts a kernel empty; one workgroup per CU: nobody else fills it) misses the
// L1 and is served by that same L2.  So every barrier round of a launch has an exchange area of its own, and a flag word
// is stored TEAM_K times: poll attempt k reads copy k, a fresh line, and only a wait that outlasts TEAM_K attempts goes on
// with agent-scope loads.  Flag words are self-validating ({round, value} in one 64-bit store; rounds grow from launch to
// launch, and only where they would wrap are the words cleared), and the vectors are complete when the flag is stored because every wave has waited for
// its stores' acknowledgements (vmcnt(0): stores count in vmcnt on gfx9) before the workgroup barrier in front of it.
// What makes this enough is that writer and reader share the L2 — which the XCC_ID census guarantees and nothing else does.
// The team kernel writes only its exchange areas, flag words, staging x (the plan's mb_x, component c) and TeamCtl; t and
// SolveState change only in the guard launch behind it (pcg_team_guard_kernel: one workgroup per coordinate), which runs
// once the whole team launch has ended.  It commits a coordinate whose TEAM_W members all finished and none gave up, and
// solves every other one by itself — a team that gave up, a team no workgroup ever joined.  Every spin is bounded by the
// wall clock (s_memrealtime): a team that cannot assemble (placement, starvation by other kernels), a row that does not fit
// the register slots, or a member whose wait times out gives up; the host sees the count in pinned memory at its next call
// and goes back to the launched form.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "pcg_team_kernel orders its stores with s_waitcnt vmcnt(0): gfx9 only (gfx10+ count stores in vscnt)"
#endif
constexpr int TEAM_W = 32;        // members per team: ONE 1024-thread workgroup per CU of a 32-CU XCD
constexpr int TEAM_NT = 1024;
constexpr int TEAM_E = 20;        // register slots per thread (rows of up to J x 20 entries) ...
constexpr int TEAM_E_TREG = 16;   // ... and of the form that keeps t's replica in registers (rows of up to J x 16)
constexpr int TEAM_K = 4;         // copies of a flag word = poll attempts served by plain loads
constexpr int TEAM_ROUNDS = 257;  // exchange areas per launch: barrier rounds 0 .. 256 (the reference's linearIter, dyn_fusion.cpp:186)
constexpr size_t TEAM_MIN_LDS = 82 * 1024;  // more than half a CU's LDS: one member per CU, nobody else fills its L1
constexpr long long TEAM_TICKS_FIRST = 2000000, TEAM_TICKS = 500000;  // 20 ms / 5 ms of the 100 MHz wall clock
// flag words of one team: [round][copy][kind: (gamma | delta), joint][2 x TEAM_W]
__host__ __device__ constexpr size_t team_words_per_round() { return (size_t)TEAM_K * 2 * 2 * TEAM_W; }
size_t solve_team_pcg_words() { return 3 * (size_t)TEAM_ROUNDS * team_words_per_round(); }

__device__ __forceinline__ unsigned xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xf; }  // HW_REG_XCC_ID[3:0]

__device__ __forceinline__ void team_give_up(TeamCtl* ctl, int c, int* host_abort) {
    if (atomicExch(&ctl->abort[c], 1u) == 0u && host_abort) atomicAdd_system(host_abort, 1);
}

// The first wave of a member polls the words of `round`: lane l reads member l & 31's gamma (l < 32) or delta word; with
// JOINT the lanes below 32 also read the joint (r0, z0) word.  Sums in lane order by the same butterfly in every member; the
// workgroup meets at a barrier behind it.  Called by every thread; false = timed out / the team has given up.  The wall clock
// (s_memrealtime: a microsecond by itself) is only consulted once a wait has lasted 64 polls.
template <bool JOINT>
__device__ __forceinline__ bool team_wait(const unsigned long long* __restrict__ wr /* this round's words */, unsigned round,
                                          float (&sum)[3], const unsigned* abort_flag, long long ticks, float* bc /* LDS [4] */,
                                          long long* prof = nullptr, int rank = 0) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        long long t0 = 0;
        unsigned long long w0 = 0, w1 = 0;
        bool good = true;
#ifdef DFA_PCG_PROFILE
        const long long c0_ = clock64();
        bool own_seen = false;
#endif
        for (unsigned spins = 0;; ++spins) {
            // attempt k < TEAM_K: copy k by a plain load (a line this CU has never read: from the L2); later: copy 0, agent scope
            const unsigned long long* p = wr + (size_t)(spins < (unsigned)TEAM_K ? spins : 0u) * (4 * TEAM_W) + lane;
            if (spins < (unsigned)TEAM_K) {
                // (wavefront scope = no cache-policy bits on the load; `volatile` would make it a system-scope one)
                w0 = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                if (JOINT) w1 = __hip_atomic_load(p + 2 * TEAM_W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            } else {
                w0 = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (JOINT) w1 = __hip_atomic_load(p + 2 * TEAM_W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const bool ok = (unsigned)(w0 >> 32) == round && (!JOINT || lane >= TEAM_W || (unsigned)(w1 >> 32) == round);
#ifdef DFA_PCG_PROFILE
            if (prof) {  // how long until this member's OWN words come back (store -> L2 -> load: no skew in it), and the polls
                const bool mine_ok = __builtin_amdgcn_readlane((int)ok, rank);
                if (mine_ok && !own_seen) own_seen = true, prof[0] += clock64() - c0_;
                prof[1] += 1;
            }
#endif
            if (__all((int)ok)) break;
            if (spins >= 64u && (spins & 63u) == 0u) {
                const long long now = wall_clock64();
                if (t0 == 0) t0 = now;
                if (now - t0 > ticks || __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    good = false;
                    break;
                }
            }
            if (spins >= (unsigned)TEAM_K) __builtin_amdgcn_s_sleep(1);
        }
        float v0 = __uint_as_float((unsigned)w0), v1 = JOINT && lane < TEAM_W ? __uint_as_float((unsigned)w1) : 0.f;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v0 += __shfl_xor(v0, o, 64), v1 += __shfl_xor(v1, o, 64);  // sums of each half of the wave
        if (lane == 0) bc[0] = v0, bc[2] = v1, bc[3] = good ? 1.f : 0.f;
        if (lane == TEAM_W) bc[1] = v0;
    }
    __syncthreads();
    sum[0] = bc[0], sum[1] = bc[1], sum[2] = bc[2];
    return bc[3] != 0.f;
}

// a member's solve: E register slots per thread; TREG: the replica of t at the entry's column lives in a register too, and the
// exchange carries m alone (4 bytes per row instead of the (m, t) pair: half the copy, 4-byte LDS gathers) — the form for
// plans whose longest row fits 16 slots per thread
template <int E, bool TREG>
__device__ __forceinline__ void team_member(const SolveView& s, SolveState* __restrict__ st, TeamCtl* ctl, char* smem, float (&red)[3][TEAM_NT / 64],
                                            float* bc, int c, int rank, unsigned epoch0, int max_iter, float pcg_tol, int* host_abort,
                                            bool late_give_up) {
    const int tid = threadIdx.x, D = s.D;
    float2* mt_s = (float2*)smem;                                      // Dpad x (m, t) ...
    float* m_s   = (float*)smem;                                       // ... TREG: Dpad x m
    float* part  = (float*)(smem + sizeof(float2) * (size_t)s.Dpad);  // TEAM_NT partial row sums
    const int R = (D + TEAM_W - 1) / TEAM_W, J = TEAM_NT / R;          // rows per member, threads per row
    const int r0 = rank * R, nrows = max(0, min(R, D - r0));
    const int a_loc = tid % R, j = tid / R;
    const bool active = j < J && a_loc < nrows, owner = active && j == 0;
    const int a = active ? r0 + a_loc : 0;  // (a valid row for the unconditional loads of the others)

    // ---- this thread's entries -> registers: slot e holds entry q = j + e J of row a
    const int cnt  = active ? min(s.ell_cnt[a], s.ell_cap) : 0;
    const int mine = cnt > j ? (cnt - j + J - 1) / J : 0;
    if (__syncthreads_or(mine > E)) {  // a row that does not fit: before anything has been published
        if (tid == 0) team_give_up(ctl, c, host_abort);
        return;
    }
    int emax = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) emax = max(emax, __shfl_xor(emax, o, 64));
    emax = __builtin_amdgcn_readfirstlane(emax);  // wave-uniform slot bound
    // (batches of unconditional loads, masked after: a load under a per-slot condition makes hipcc wait for each one by
    // itself — 48 dependent round trips, 35 us, in the first version of this prologue; in two halves: the unpacked columns of
    // all E slots at once cost registers the loop needs)
    float val[E], ucol[E], tcol[TREG ? E : 1];
    uint32_t colp[E / 2];
#pragma unroll
    for (int e = 0; e < (TREG ? E : 1); ++e) tcol[e] = 0.f;
#pragma unroll
    for (int h0 = 0; h0 < E; h0 += E / 2) {
        int col[E / 2];
#pragma unroll
        for (int i = 0; i < E / 2; ++i) {
            const int e     = h0 + i;
            const float2 en = s.ell[(size_t)min(j + e * J, s.ell_cap - 1) * D + a];
            const bool live = e < mine;
            val[e] = live ? en.x : 0.f;
            col[i] = live ? __float_as_int(en.y) : a;
        }
        float gcol[E / 2];
#pragma unroll
        for (int i = 0; i < E / 2; ++i) ucol[h0 + i] = s.diag[col[i]], gcol[i] = s.g[3 * col[i] + c];  // (both in one round trip)
#pragma unroll
        for (int i = 0; i < E / 2; ++i) ucol[h0 + i] = jacobi_inv(ucol[h0 + i]) * gcol[i];
#pragma unroll
        for (int i = 0; i < E / 2; i += 2) colp[(h0 + i) / 2] = (uint32_t)col[i] | ((uint32_t)col[i + 1] << 16);
        __builtin_amdgcn_sched_barrier(0);
    }
    // ---- row owners: r = g, u = M^-1 g, x = p = s = t = 0; (r0, z0) of the JOINT system scales the stopping rules
    float minv = 0.f, r = 0.f, u = 0.f, x = 0.f, pv = 0.f, sv = 0.f, tv = 0.f, w = 0.f, m = 0.f, joint_loc = 0.f;
    if (owner) {
        minv = jacobi_inv(s.diag[a]);
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            const float g = s.g[3 * a + cc];
            joint_loc     = fmaf(g, minv * g, joint_loc);
            if (cc == c) r = g;
        }
        u = minv * r;
    }
    // exchange area / flag words of barrier round r of THIS launch (r = 0 .. max_iter): never read twice by a CU
    auto mt_at = [&](int rr) __attribute__((always_inline)) { return s.team_mt + ((size_t)rr * 3 + c) * s.team_stride; };
    auto words_at = [&](int rr) __attribute__((always_inline)) {
        return s.team_words + ((size_t)c * TEAM_ROUNDS + rr) * team_words_per_round();
    };

    // w = A u over the replicas; the row's J partial sums meet in LDS (threads of a row are R apart: any R, any J)
    auto row_product = [&]() __attribute__((always_inline)) {
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
        for (int e = 0; e < E; e += 2)
            if (e < emax) acc0 = fmaf(val[e], ucol[e], acc0), acc1 = fmaf(val[e + 1], ucol[e + 1], acc1);  // (empty slots hold val = 0)
        part[tid] = acc0 + acc1;
        __syncthreads();
        float tot = 0.f;
        if (owner) {
            for (int j0 = 0; j0 < J; j0 += 8) {  // eight LDS reads in flight
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = part[a_loc + min(j0 + q, J - 1) * R];
#pragma unroll
                for (int q = 0; q < 8; ++q) tot += j0 + q < J ? v[q] : 0.f;
            }
        }
        return tot;
    };
    // (m, t) of the own rows and the member's partial sums for barrier round rr (tag `round`)
    auto publish = [&](int rr, unsigned round, float gp, float dp, float jp, bool with_joint) __attribute__((always_inline)) {
        // (a plain store: in the XCD's L2 once acknowledged)
        if (owner) {
            if (TREG) ((float*)mt_at(rr))[a] = m;
            else mt_at(rr)[a] = make_float2(m, tv);
        }
        const float gw = wave_total(gp), dw = wave_total(dp), jw = with_joint ? wave_total(jp) : 0.f;
        if ((tid & 63) == 0) red[0][tid >> 6] = gw, red[1][tid >> 6] = dw, red[2][tid >> 6] = jw;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores have been acknowledged by the L2
        __syncthreads();
        // thread (copy k, kind q): q = 0 gamma, 1 delta, 2 joint — 64-bit stores, one per copy
        if (tid < 3 * TEAM_K) {
            const int q = tid % 3, kk = tid / 3;
            if (q < 2 || with_joint) {
                float tot = 0.f;
#pragma unroll
                for (int i = 0; i < TEAM_NT / 64; ++i) tot += red[q][i];
                unsigned long long* dst = words_at(rr) + (size_t)kk * (4 * TEAM_W) + (q == 2 ? 2 * TEAM_W : q * TEAM_W) + rank;
                __hip_atomic_store(dst, ((unsigned long long)round << 32) | __float_as_uint(tot), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WAVEFRONT);  // (one 64-bit store, no cache-policy bits)
            }
        }
    };

#ifdef DFA_PCG_PROFILE
    long long pc_[6] = {0, 0, 0, 0, 0, 0}, pw_[2] = {0, 0};
    long long last_  = clock64();
#endif
    w = row_product();
    m = minv * w;
    publish(0, epoch0, r * u, w * u, joint_loc, true);
    PROF_MARK(5);  // (prologue's product + first publication)

    float target = 0.f, gamma_old = 1.f, alpha_old = 1.f;
    int it = 0;
    bool gave_up = false;
    while (it < max_iter) {
        float sm[3];
        const unsigned round = epoch0 + (unsigned)it;
        if (it == 0) {
            if (!team_wait<true>(words_at(0), round, sm, &ctl->abort[c], TEAM_TICKS_FIRST, bc)) { gave_up = true; break; }
            const float rz0    = sm[2];
            const bool at_floor = pcg_at_floor(st, rz0);  // the same in every team
            if (tid == 0 && rank == 0) ctl->rz0[c] = rz0, ctl->at_floor[c] = at_floor;
            if (at_floor) break;  // (x = 0: nothing to solve)
            target = pcg_joint_target(st, pcg_tol, rz0) * (1.0f / 3.0f);  // this coordinate's share of the joint target
        } else {
#ifdef DFA_PCG_PROFILE
            if (!team_wait<false>(words_at(it), round, sm, &ctl->abort[c], TEAM_TICKS, bc, tid == 0 && c == 0 && rank == 0 ? pw_ : nullptr, rank)) { gave_up = true; break; }
#else
            if (!team_wait<false>(words_at(it), round, sm, &ctl->abort[c], TEAM_TICKS, bc)) { gave_up = true; break; }
#endif
        }
        const float gamma = sm[0], delta = sm[1];
        PROF_MARK(0);  // wait
        if (!(gamma > target)) {  // converged: (r, M^-1 r) of the iterate in x
            gave_up = late_give_up;  // (development builds: a member that gives up behind the last barrier its team passed)
            break;
        }
        const float beta  = cg_beta(it == 0, gamma, gamma_old);
        const float denom = cg_denom(it == 0, gamma, delta, beta, alpha_old);
        if (!(denom > 0.f)) break;
        const float alpha = gamma / denom;
        {   // the published (m_i, t_(i-1)) of every row -> LDS by plain wide loads (first and only read of round i's area by
            // this CU: from the L2)
            const float4* src = (const float4*)mt_at(it);
            float4* dst       = (float4*)mt_s;
            const int n4      = TREG ? s.Dpad / 4 : s.Dpad / 2;
            for (int i0 = tid; i0 < n4; i0 += 4 * TEAM_NT) {  // four loads in flight per thread
                float4 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = src[min(i0 + q * TEAM_NT, n4 - 1)];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (i0 + q * TEAM_NT < n4) dst[i0 + q * TEAM_NT] = v[q];
            }
        }
        __syncthreads();
        PROF_MARK(1);  // copy
        // four gathers in flight per step (a step under its own wave-uniform branch would wait for each gather by itself)
#pragma unroll
        for (int e0 = 0; e0 < E; e0 += 4)
            if (e0 < emax) {
                uint32_t c01 = colp[e0 / 2], c23 = colp[e0 / 2 + 1];
                asm volatile("" : "+v"(c01), "+v"(c23));
                if (TREG) {  // t's replica in a register: the same fmaf on the same numbers as the row's owner
                    const float g0 = m_s[c01 & 0xffffu], g1 = m_s[c01 >> 16], g2 = m_s[c23 & 0xffffu], g3 = m_s[c23 >> 16];
                    const int t0 = TREG ? e0 : 0;  // (tcol has one element in the other form: never indexed there)
                    tcol[t0]                  = fmaf(beta, tcol[t0], g0);
                    tcol[TREG ? e0 + 1 : 0]   = fmaf(beta, tcol[TREG ? e0 + 1 : 0], g1);
                    tcol[TREG ? e0 + 2 : 0]   = fmaf(beta, tcol[TREG ? e0 + 2 : 0], g2);
                    tcol[TREG ? e0 + 3 : 0]   = fmaf(beta, tcol[TREG ? e0 + 3 : 0], g3);
                    ucol[e0]     = fmaf(-alpha, tcol[t0], ucol[e0]);
                    ucol[e0 + 1] = fmaf(-alpha, tcol[TREG ? e0 + 1 : 0], ucol[e0 + 1]);
                    ucol[e0 + 2] = fmaf(-alpha, tcol[TREG ? e0 + 2 : 0], ucol[e0 + 2]);
                    ucol[e0 + 3] = fmaf(-alpha, tcol[TREG ? e0 + 3 : 0], ucol[e0 + 3]);
                } else {
                    const float2 g0 = mt_s[c01 & 0xffffu], g1 = mt_s[c01 >> 16], g2 = mt_s[c23 & 0xffffu], g3 = mt_s[c23 >> 16];
                    ucol[e0]     = fmaf(-alpha, fmaf(beta, g0.y, g0.x), ucol[e0]);
                    ucol[e0 + 1] = fmaf(-alpha, fmaf(beta, g1.y, g1.x), ucol[e0 + 1]);
                    ucol[e0 + 2] = fmaf(-alpha, fmaf(beta, g2.y, g2.x), ucol[e0 + 2]);
                    ucol[e0 + 3] = fmaf(-alpha, fmaf(beta, g3.y, g3.x), ucol[e0 + 3]);
                }
            }
        if (owner) cg_update_row(alpha, beta, u, w, pv, sv, x, r), cg_update_u(alpha, beta, m, tv, u);
        PROF_MARK(2);  // replicas
        w = row_product();  // (its barrier also orders this iteration's reads of mt_s before the next copy)
        m = minv * w;
        ++it;
        gamma_old = gamma, alpha_old = alpha;
        PROF_MARK(3);  // row product
        publish(it, epoch0 + (unsigned)it, r * u, w * u, 0.f, false);
        PROF_MARK(4);  // publish
    }
#ifdef DFA_PCG_PROFILE
    if (tid == 0 && c == 0 && rank == 0) {
        for (int i = 0; i < 6; ++i) st->prof[i] += pc_[i];
        st->prof[6] += pw_[0], st->prof[7] += pw_[1];
    }
#endif
    if (gave_up) {  // the guard launch solves this coordinate (t is untouched: members only stage x)
        if ((tid & 63) == 0) team_give_up(ctl, c, host_abort);
        return;
    }
    // staged for the guard launch, which commits it only if every member of the team gets here and none gives up
    if (owner) ((float*)s.mb_x)[4 * a + c] = x;
    if (tid == 0) {
        atomicAdd(&ctl->finished[c], 1u);
        if (rank == 0) ctl->iters[c] = it;
    }
}

__global__ __launch_bounds__(TEAM_NT) void pcg_team_kernel(SolveView s, SolveState* __restrict__ st, unsigned epoch0, int max_iter,
                                                           float pcg_tol, int* host_abort, int force_abort) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int rank_sh;
    __shared__ float red[3][TEAM_NT / 64];
    __shared__ float bc[4];
    if (st->done || st->converged) return;  // (converged: a no-op iteration, see SolveState::converged; the guard books it)
    const unsigned xcc = xcc_id();
    if (xcc >= 3u) return;
    const int c = (int)xcc, tid = threadIdx.x, D = s.D;
    TeamCtl* ctl = s.team_ctl;
    if (tid == 0) rank_sh = (int)atomicAdd(&ctl->count[c], 1u);
    __syncthreads();
    const int rank = rank_sh;
    if (rank >= TEAM_W) return;  // the team is complete without this workgroup
    // (development builds, the guard launch's tests: the teams of the masked coordinates give up at entry; 8 + mask: they
    // leave without a word, as a team that never existed; 32 + mask: their member TEAM_W - 1 gives up behind the barrier of
    // the converging round while the others finish)
    const bool masked = (force_abort >> c) & 1;
    if (masked && !(force_abort & 32)) {
        if (tid == 0 && !(force_abort & 8)) team_give_up(ctl, c, host_abort);
        return;
    }
    const bool late_give_up = masked && rank == TEAM_W - 1;
    // which form: the longest row of the matrix (SolveState::max_row_nnz, raised by the assembly in front of this launch: the
    // same value in every workgroup) against the 16 slots per thread of the form that keeps t's replica in registers
    const int rows_ = (D + TEAM_W - 1) / TEAM_W, j_ = TEAM_NT / rows_;
    const bool treg = st->max_row_nnz <= j_ * TEAM_E_TREG && !(force_abort & 16);  // (development builds: 16 = the (m, t) form always)
    if (treg) team_member<TEAM_E_TREG, true>(s, st, ctl, smem, red, bc, c, rank, epoch0, max_iter, pcg_tol, host_abort, late_give_up);
    else team_member<TEAM_E, false>(s, st, ctl, smem, red, bc, c, rank, epoch0, max_iter, pcg_tol, host_abort, late_give_up);
}

// The guard behind every team launch, and for the team form the only writer of t and SolveState: it runs once the whole
// team launch has ended.  Workgroup c commits team c's result if all TEAM_W members finished and none gave up (t += the
// staged x; nothing but the at-floor mark if the team found the gradient at the floor); otherwise it solves coordinate c
// by itself, which is safe because the team has not touched t — the same recurrence and stopping rules in one
// 1024-thread workgroup, u in LDS, the matrix streamed from the ELL as assembled, the rows' vectors in the plan's mb_*
// buffers (component c).  Slow (tens of microseconds per iteration) and rare by construction.  It resets team c's words
// of the control block for the next launch.
__global__ __launch_bounds__(1024) void pcg_team_guard_kernel(SolveView s, SolveState* __restrict__ st, int max_iter, float pcg_tol,
                                                              int* host_abort) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red0[16], red1[16];
    __shared__ int todo_sh, it_sh, floor_sh;  // todo: 0 nothing, 1 commit the team's result, 2 solve here
    __shared__ float rz0_sh;
    const int c = blockIdx.x, tid = threadIdx.x, D = s.D;
    TeamCtl* ctl = s.team_ctl;
    if (tid == 0) {
        // (st->done and st->converged are read here by every workgroup and written, if at all, by the last one to arrive
        // at the ticket below: the three agree)
        const bool gave_up = ctl->abort[c] != 0u, complete = ctl->finished[c] == (unsigned)TEAM_W && !gave_up;
        todo_sh = 0;
        if (!st->done && st->converged) {  // the team launch returned at entry: a no-op iteration, booked once
            if (c == 0) st->gn_iters += 1, st->gn_noop += 1;
        } else if (!st->done) {
            todo_sh = complete ? 1 : 2;
            // a team that gave up has counted itself; a team nobody joined is counted here: the plan goes back to the
            // launched form
            if (!complete && !gave_up && host_abort) atomicAdd_system(host_abort, 1);
            it_sh = ctl->iters[c], rz0_sh = ctl->rz0[c], floor_sh = (int)ctl->at_floor[c];
        }
        ctl->count[c] = 0u, ctl->abort[c] = 0u, ctl->finished[c] = 0u, ctl->at_floor[c] = 0u, ctl->iters[c] = 0, ctl->rz0[c] = 0.f;
    }
    __syncthreads();
    if (todo_sh == 0) return;
    int it = it_sh;
    float rz0 = rz0_sh;
    bool at_floor = floor_sh != 0;
    float* xs = (float*)s.mb_x + c;  // [4 a]
    if (todo_sh == 2) {
        float* u_s = (float*)smem;  // Dpad
        float *rs = (float*)s.mb_r + c, *ps = (float*)s.mb_p + c, *ss = (float*)s.mb_s + c;
        float joint_loc = 0.f;
        for (int a = tid; a < D; a += 1024) {
            const float minv = jacobi_inv(s.diag[a]);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const float g = s.g[3 * a + cc];
                joint_loc     = fmaf(g, minv * g, joint_loc);
            }
            const float g = s.g[3 * a + c];
            xs[4 * a] = 0.f, rs[4 * a] = g, ps[4 * a] = 0.f, ss[4 * a] = 0.f;
            u_s[a] = minv * g;
        }
        rz0      = block_sum_f<16>(joint_loc, red0);  // (its barrier publishes u_s)
        at_floor = pcg_at_floor(st, rz0);
        it       = 0;
        const float target = pcg_joint_target(st, pcg_tol, rz0) * (1.0f / 3.0f);
        float gamma_old = 1.f, alpha_old = 1.f;
        __syncthreads();
        while (!at_floor && it < max_iter) {
            float g_loc = 0.f, d_loc = 0.f;
            for (int a = tid; a < D; a += 1024) {
                const int cnt = min(s.ell_cnt[a], s.ell_cap);
                float w = 0.f;
                for (int q = 0; q < cnt; ++q) {
                    const float2 en = s.ell[(size_t)q * D + a];
                    w = fmaf(en.x, u_s[__float_as_int(en.y)], w);
                }
                ((float*)s.mb_w)[4 * a + c] = w;
                g_loc = fmaf(rs[4 * a], u_s[a], g_loc), d_loc = fmaf(w, u_s[a], d_loc);
            }
            const float gw = wave_total(g_loc), dw = wave_total(d_loc);
            if ((tid & 63) == 0) red0[tid >> 6] = gw, red1[tid >> 6] = dw;
            __syncthreads();
            float gamma = 0.f, delta = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) gamma += red0[i], delta += red1[i];
            if (!(gamma > target)) break;
            const float beta  = cg_beta(it == 0, gamma, gamma_old);
            const float denom = cg_denom(it == 0, gamma, delta, beta, alpha_old);
            if (!(denom > 0.f)) break;
            const float alpha = gamma / denom;
            for (int a = tid; a < D; a += 1024) {
                const float minv = jacobi_inv(s.diag[a]);
                float p = ps[4 * a], sn = ss[4 * a], x = xs[4 * a], r = rs[4 * a];
                cg_update_row(alpha, beta, u_s[a], ((float*)s.mb_w)[4 * a + c], p, sn, x, r);
                ps[4 * a] = p, ss[4 * a] = sn, xs[4 * a] = x, rs[4 * a] = r;
                u_s[a] = minv * r;  // (own row only; the gathers of this iteration are behind the reduction's barrier)
            }
            ++it;
            gamma_old = gamma, alpha_old = alpha;
            __syncthreads();
        }
    }
    if (!at_floor) {  // t += x, four rows' loads in flight per thread
        for (int a0 = tid; a0 < D; a0 += 4 * 1024) {
            float xv[4], tv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int a = min(a0 + q * 1024, D - 1);
                xv[q] = xs[4 * a], tv[q] = s.t[3 * a + c];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (a0 + q * 1024 < D) s.t[3 * (a0 + q * 1024) + c] = tv[q] + xv[q];
        }
    }
    if (tid == 0) pcg_book_launch_of_three(st, rz0, it, at_floor);  // (at the floor: no iterations, and the mark)
}

// plans the team form can serve: (m, t) of every row + the partial sums in one CU's LDS (Dpad <= 19 584), a member's rows on
// its threads (it is USED above the register-resident kernels: more than 2 048 nodes)
bool solve_team_pcg_fits(int D) {
    return sizeof(float2) * (size_t)((D + 3) & ~3) + sizeof(float) * TEAM_NT + 1024 <= 158 * 1024 && (D + TEAM_W - 1) / TEAM_W <= TEAM_NT;
}
int solve_team_pcg_rounds() { return TEAM_ROUNDS; }

hipError_t launch_team_pcg(const SolveView& s, SolveState* state, int max_iter, float pcg_tol, TeamPcg* tp, hipStream_t st) {
    hipError_t e = allow_big_lds(pcg_team_kernel);
    if (e == hipSuccess) e = allow_big_lds(pcg_team_guard_kernel);
    if (e != hipSuccess) return e;
    const size_t lds = std::max(sizeof(float2) * (size_t)s.Dpad + sizeof(float) * TEAM_NT, TEAM_MIN_LDS);
    if (max_iter + 1 > TEAM_ROUNDS) return hipErrorInvalidValue;  // (route_pcg asks solve_team_pcg_fits first)
    {   // The barrier rounds of a launch are numbered from `epoch0`, a kernel ARGUMENT: a captured launch replayed from a HIP
        // graph would meet its own flag words of the replay before and sail through its barriers.  Refused loudly (the
        // launched form above 2 048 nodes synchronises with its stream and was never capturable either).
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return hipErrorStreamCaptureUnsupported;
    }
    // Two team launches of different plans must not share the device: each wants every CU of XCDs 0-2 for its members, and
    // two half-assembled teams would wait for each other until both time out (correct — the guard launches take over — but
    // 20 ms lost).  Launches on ONE stream are ordered anyway, and a process that only ever uses one stream for them pays
    // nothing here.  The first launch on a SECOND stream waits for the device once; from then on every team launch records
    // an event behind itself and a launch on another stream than the one before waits for it.  Per device, under a lock:
    // plans may be driven from several host threads.
    struct Turn {
        hipEvent_t ev      = nullptr;
        hipStream_t stream = nullptr;
        bool any = false, several = false;
    };
    static std::mutex mu;
    static std::map<int, Turn> turns;
    int dev = 0;
    e       = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    Turn& turn = turns[dev];
    if (turn.any && turn.stream != st) {
        if (!turn.several) {
            if ((e = hipEventCreateWithFlags(&turn.ev, hipEventDisableTiming)) != hipSuccess) return e;
            if ((e = hipDeviceSynchronize()) != hipSuccess) return e;  // (once per process and device: no event behind the launches so far)
            turn.several = true;
        } else if ((e = hipStreamWaitEvent(st, turn.ev, 0)) != hipSuccess) {
            return e;
        }
    }
    // rounds epoch0 .. epoch0 + max_iter of this launch.  Where they would wrap or reach 0 (the value of a word nobody has
    // written), the flag words are cleared behind the plan's earlier launches and the rounds start again at 1.
    unsigned epoch0     = tp->epoch;
    const unsigned span = (unsigned)max_iter + 8u;
    if (epoch0 == 0u || epoch0 > ~0u - span) {
        if ((e = hipMemsetAsync(s.team_words, 0, sizeof(unsigned long long) * solve_team_pcg_words(), st)) != hipSuccess) return e;
        epoch0 = 1u;
    }
    tp->epoch = epoch0 + span;
    pcg_team_kernel<<<8 * TEAM_W, TEAM_NT, lds, st>>>(s, state, epoch0, max_iter, pcg_tol, tp->host_abort,
                                                             dev_env_int("DFA_MB_TEAM_ABORT", 0));
    pcg_team_guard_kernel<<<3, 1024, sizeof(float) * (size_t)s.Dpad, st>>>(s, state, max_iter, pcg_tol, tp->host_abort);
    tp->launches += 1;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (turn.several) e = hipEventRecord(turn.ev, st);
    turn.stream = st, turn.any = true;
    return e;
}

}  // namespace dfa
