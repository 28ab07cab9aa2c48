// solve_pcg.hip — the block-Jacobi PCG of one linearisation of the reference-mode solve: the forms that run in ONE
// workgroup per coordinate (register-resident up to 2 048 nodes; streaming inside the same launch when a row pair does not
// fit), and route_pcg, which chooses between them, the teams (solve_pcg_team.hip) and the launched form
// (solve_pcg_launched.hip).  Why the PCG comes in these forms: solve.hpp, MI355X mapping; what an iteration IS —
// preconditioner, stopping rules, Chronopoulos-Gear scalars, row update, booking —: pcg_rules.hpp.
#include <hip/hip_runtime.h>

#include "dev_switch.hpp"
#include "device_math.hpp"
#include "pcg_rules.hpp"
#include "solve.hpp"
#include "solve_internal.hpp"

namespace dfa {

// rows of equal length in index order: `from` holds the permutation as the atomic cursors left it (ranks in [0, D), rows
// grouped by length, hist[b] = end of bin b), `to` receives the order-stable one.  Called by all NT threads.
template <int NT, int R>
__device__ __forceinline__ void stable_equal_runs(const int32_t* from, int32_t* to, const int32_t* cnt_of_row, const int* hist, int D) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int rank = (int)threadIdx.x + NT * i;
        if (rank >= D) continue;
        const int row = from[rank];
        const int bin = 256 - min(cnt_of_row[row], 256);
        const int beg = bin > 0 ? hist[bin - 1] : 0, end = hist[bin];
        int before = 0;
        for (int q = beg; q < end; ++q) before += from[q] < row;
        to[beg + before] = row;
    }
}

// ------------------------------------------------------------------------------------------
// block-Jacobi PCG, one persistent workgroup of 1024 threads; thread owns rows tid + 1024*i.

// Streaming PCG for systems too large for the register-resident kernel (D > 2048 or rows wider than
// its slots): one persistent workgroup, RPT rows per thread, the matrix re-read from L2 every
// iteration.  A single CU moves 64 B/clk through its vector memory path, so the bytes per iteration
// are what matters: the prologue counting-sorts the rows by length (wave-uniform loop bounds with
// almost no padding) and repacks the ELL image rank-major with 16-bit columns — 6 B per non-zero,
// fully coalesced — into the plan's workspace.
// The whole workgroup (NT threads, NT * RPT >= D) runs this: the way out of the register-resident kernel when a row pair
// does not fit its slots (it used to be a launch of its own behind every register-resident one, which returned at once
// in the common case: 5 launches per C2 frame).
template <int NT, int RPT>
__device__ __forceinline__ void pcg_stream_body(const SolveView& s, SolveState* __restrict__ st, int max_iter, float pcg_tol,
                                                char* smem) {
    float4* p_s = (float4*)smem;                                      // D entries
    float* red0 = (float*)(smem + sizeof(float4) * (size_t)s.Dpad);  // 2 x 16 wave partials
    float* red1 = red0 + 16;
    int* hist   = (int*)(red1 + 16);                                  // 260 bins
    const int tid = threadIdx.x;
    const int D   = s.D;

    // ---- rows sorted by length (descending): rank -> row in s.pk_perm
    for (int i = tid; i < 260; i += NT) hist[i] = 0;
    __syncthreads();
    int my_cnt[RPT];
#pragma unroll
    for (int h = 0; h < RPT; ++h) {
        const int row = tid + NT * h;
        my_cnt[h]     = row < D ? min(s.ell_cnt[row], 256) : -1;
        if (my_cnt[h] >= 0) atomicAdd(&hist[256 - my_cnt[h]], 1);
    }
    __syncthreads();
    if (tid < 64) {
        int loc[5], sum = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int b = tid * 5 + j;
            loc[j]      = b < 257 ? hist[b] : 0;
            sum += loc[j];
        }
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (tid >= o) incl += t;
        }
        int off = incl - sum;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int b = tid * 5 + j;
            if (b < 257) hist[b] = off;
            off += loc[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < RPT; ++h)
        if (my_cnt[h] >= 0) (s.deterministic ? s.pk_perm2 : s.pk_perm)[atomicAdd(&hist[256 - my_cnt[h]], 1)] = tid + NT * h;
    __syncthreads();  // workgroup-scope visibility of pk_perm
    if (s.deterministic) {  // (hist[b] is now the end of bin b)
        stable_equal_runs<NT, RPT>(s.pk_perm2, s.pk_perm, s.ell_cnt, hist, D);
        __syncthreads();
    }

    // ---- my rows = ranks tid + NT*i; repack them rank-major (coalesced from now on)
    int row[RPT], rcnt[RPT], wmax[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int rank = tid + NT * i;
        row[i]         = rank < D ? s.pk_perm[rank] : -1;
        rcnt[i]        = row[i] >= 0 ? min(s.ell_cnt[row[i]], 256) : 0;
        for (int q = 0; q < rcnt[i]; ++q) {
            const float2 e                  = s.ell[(size_t)q * D + row[i]];
            s.pk_vals[(size_t)q * D + rank] = e.x;
            s.pk_cols[(size_t)q * D + rank] = (uint16_t)__float_as_int(e.y);
        }
        int m = rcnt[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
        wmax[i] = m;  // wave-uniform
    }
    __syncthreads();

    float x[RPT][3], r[RPT][3], p[RPT][3], minv[RPT];
    float rz_loc = 0.f;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        if (row[i] >= 0) {
            minv[i] = jacobi_inv(s.diag[row[i]]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[i][c] = 0.f;
                r[i][c] = s.g[3 * row[i] + c];
                p[i][c] = minv[i] * r[i][c];
                rz_loc  = fmaf(r[i][c], p[i][c], rz_loc);
            }
            p_s[row[i]] = make_float4(p[i][0], p[i][1], p[i][2], 0.f);
        } else {
            minv[i] = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) x[i][c] = r[i][c] = p[i][c] = 0.f;
        }
    }
    double rz           = block_sum<NT / 64>(rz_loc, red1);  // the barrier inside also publishes p_s
    const double rz0    = rz;
    const double floor_ = 1e-12;  // squared-residual-ratio floor of float arithmetic
    const double tol2   = (double)pcg_tol * (double)pcg_tol > floor_ ? (double)pcg_tol * (double)pcg_tol : floor_;
    int it              = 0;
    const bool skip     = pcg_at_floor(st, rz0);
    const double target = fmax(tol2 * rz0, (double)solve_floor(st));
    if (!skip) {
        while (it < max_iter) {
            if (!(rz > 0.0)) break;
            float ap[RPT][3];
            float pap_loc = 0.f;
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int rank  = tid + NT * i;
                const int rankc = rank < D ? rank : 0;
                float ax = 0.f, ay = 0.f, az = 0.f;
                // 8 (coalesced, rank-major) loads in flight per lane; wmax is wave-uniform.  Loads are
                // unconditional (slots up to the ELL capacity are valid memory) and masked AFTER the
                // load: a load under a per-element condition makes hipcc branch around it and wait
                // vmcnt(0) each time — 16 serial L2 round trips per chunk.
                for (int q0 = 0; q0 < wmax[i]; q0 += 8) {
                    int colv[8];
                    float valv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int q = min(q0 + u, 255);
                        colv[u]     = s.pk_cols[(size_t)q * D + rankc];
                        valv[u]     = s.pk_vals[(size_t)q * D + rankc];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const bool ok = q0 + u < rcnt[i];
                        colv[u]       = ok ? colv[u] : 0;
                        valv[u]       = ok ? valv[u] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float4 pc = p_s[colv[u]];
                        ax = fmaf(valv[u], pc.x, ax), ay = fmaf(valv[u], pc.y, ay), az = fmaf(valv[u], pc.z, az);
                    }
                }
                ap[i][0] = ax, ap[i][1] = ay, ap[i][2] = az;
                pap_loc = fmaf(p[i][0], ax, fmaf(p[i][1], ay, fmaf(p[i][2], az, pap_loc)));
            }
            const double pAp = block_sum<NT / 64>(pap_loc, red0);
            if (!(pAp > 0.0)) break;
            const float alpha = (float)(rz / pAp);
            float rzn_loc     = 0.f;
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    x[i][c] = fmaf(alpha, p[i][c], x[i][c]);
                    r[i][c] = fmaf(-alpha, ap[i][c], r[i][c]);
                    rzn_loc = fmaf(r[i][c], minv[i] * r[i][c], rzn_loc);
                }
            }
            const double rz_new = block_sum<NT / 64>(rzn_loc, red1);
            ++it;
            if (rz_new <= target) break;
            const float beta = (float)(rz_new / rz);
            // every thread has read p_s for this iteration (two barriers passed since the SpMV)
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
#pragma unroll
                for (int c = 0; c < 3; ++c) p[i][c] = fmaf(beta, p[i][c], minv[i] * r[i][c]);
                if (row[i] >= 0) p_s[row[i]] = make_float4(p[i][0], p[i][1], p[i][2], 0.f);
            }
            rz = rz_new;
            __syncthreads();
        }
    }
    // t += delta
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        if (row[i] >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s.t[3 * row[i] + c] += x[i][c];
        }
    }
    if (tid == 0) pcg_book_launch(st, rz0, it, skip);
}

// ------------------------------------------------------------------------------------------
// PCG with the WHOLE matrix in registers (D <= 2 * NT rows).
//
// The matrix is constant over the PCG iterations, and a single CU can stream at most 64 B/clk
// through its vector memory path: re-reading a padded ELL image every iteration costs more than
// everything else in the loop together (measured: 6.1 k of 10.5 k cycles per iteration).  Here a
// thread keeps its rows' entries in registers for the whole solve — E values and E/2 words of
// packed 16-bit columns (as LDS byte offsets) — so the only per-iteration memory traffic left is the LDS gather of p
// (one ds_read_b128 per non-zero).
//
// Register arrays need compile-time indices, so row lengths must be (nearly) uniform across the
// lanes of a wave or the padding eats the gain.  The prologue therefore counting-sorts the rows
// by length in LDS and gives thread t the t-th LONGEST row ("A", slots 0.. upwards) and the t-th
// SHORTEST row ("B", slots E-1.. downwards): lengths vary slowly along a wave, nA + nB is about
// the true row-pair length, and both loop bounds are wave-uniform (no divergence, no selects).
// Entries of B that do not fit (rare) are streamed from L2 each iteration.
//
// NC = 3: one workgroup, the three coordinates share alpha / beta (CG on A (x) I3 as one system).
// NC = 1: JtJ = A (x) I3 is three INDEPENDENT scalar systems with the same matrix — workgroup c of three
// solves coordinate c on its own CU.  The gather shrinks from one ds_read_b128 + 3 FMAs per non-zero to one
// ds_read_b32 + 1 FMA (the LDS pipe moves 128 B/clk: 8 clocks per wave-wide b128 read, 2 per b32 read).  Every
// coordinate stops at (r, z)_c <= tol^2 (r0, z0)_joint / 3, which implies the joint stopping rule.
template <int NT, int E, int NC>
__global__ __launch_bounds__(NT) void pcg_paired_kernel(SolveView s, SolveState* __restrict__ st, int max_iter,
                                                        float pcg_tol) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D     = s.D;
    const int c0    = NC == 1 ? (int)blockIdx.x : 0;  // first coordinate of this workgroup
    float4* p_s     = (float4*)smem;  // D x 16 B (NC = 3) / D x 4 B (NC = 1) in the same 16 B x Dpad region
    float* p_s1     = (float*)smem;
    float* red0     = (float*)(smem + sizeof(float4) * (size_t)s.Dpad);
    float* red1     = red0 + 16;
    int* hist       = (int*)(red1 + 16);  // 258 bins
    int* perm       = hist + 260;         // D row ids, longest row first
    if (st->done) return;
    const int tid = threadIdx.x;
    if (st->converged) {  // no-op iteration (see SolveState::converged); booked once, by whoever solves this plan
        if (tid == 0 && blockIdx.x == 0) st->gn_iters += 1, st->gn_noop += 1;
        return;
    }
    // pairs of rows per thread.  Every instantiation has one; the [P] dimension of the register arrays stays because the
    // compiler allots 112 / 210 VGPRs without it where it allots 114 / 212 with it (profiles/pcg_rules_refactor.md).
    constexpr int P = 1;
    constexpr int R = 2 * P;  // rows per thread

    // ---- (r0, z0) of the joint system first, rows in natural order: it scales both stopping rules, and a gradient at
    // the round-off floor ends the launch here, before the sort and the 25 us of loading the matrix into registers
    float rzj_loc = 0.f;
#pragma unroll
    for (int h = 0; h < R; ++h) {
        const int row = tid + NT * h;
        if (row < D) {
            const float minv = jacobi_inv(s.diag[row]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float g = s.g[3 * row + c];
                rzj_loc       = fmaf(g, minv * g, rzj_loc);
            }
        }
    }
    const float rz0 = block_sum_f<NT / 64>(rzj_loc, red1);
    const bool skip = pcg_at_floor(st, rz0);
    if (skip) {  // the same decision in every workgroup; the first one books the (empty) iteration
        if (tid == 0 && blockIdx.x == 0) {
            st->gn_iters += 1;
            solve_mark_at_floor(st);
        }
        return;
    }

    // ---- rows sorted by length (descending), counting sort in LDS
    // (the second copy of pcg_stream_body's sort, on purpose: as a shared function it cost 1.2 % at C2, profiles/pcg_row_ranking_refactor.md)
    for (int i = tid; i < 260; i += NT) hist[i] = 0;
    __syncthreads();
    int my_cnt[R];
#pragma unroll
    for (int h = 0; h < R; ++h) {
        const int row = tid + NT * h;
        my_cnt[h]     = row < D ? min(s.ell_cnt[row], 256) : -1;
        if (my_cnt[h] >= 0) atomicAdd(&hist[256 - my_cnt[h]], 1);  // bin 0 = longest
    }
    __syncthreads();
    if (tid < 64) {  // exclusive scan of 257 bins by one wave (5 bins per lane)
        int loc[5], sum = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int b = tid * 5 + j;
            loc[j]      = b < 257 ? hist[b] : 0;
            sum += loc[j];
        }
        int incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (tid >= o) incl += t;
        }
        int off = incl - sum;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int b = tid * 5 + j;
            if (b < 257) hist[b] = off;
            off += loc[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < R; ++h)
        if (my_cnt[h] >= 0) (s.deterministic ? perm + s.Dpad : perm)[atomicAdd(&hist[256 - my_cnt[h]], 1)] = tid + NT * h;
    __syncthreads();
    if (s.deterministic) {  // (the launcher sized the LDS for a second array of row ids; hist[b] is now the end of bin b)
        stable_equal_runs<NT, R>(perm + s.Dpad, perm, s.ell_cnt, hist, D);
        __syncthreads();
    }

    // ---- this thread's pairs: pair j = rank j*NT + t (long, "A") and rank D-1-j*NT-t (short, "B")
    int rowA[P], rowB[P], nA[P], nB[P], cntA_[P], cntB_[P];
    bool unfit_any = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int ia = j * NT + tid, ib = D - 1 - j * NT - tid;
        rowA[j]      = (ia < D && ia <= ib) ? perm[ia] : -1;
        rowB[j]      = (ib >= 0 && ib > ia) ? perm[ib] : -1;
        const int cntA = rowA[j] >= 0 ? min(s.ell_cnt[rowA[j]], 256) : 0;
        const int cntB = rowB[j] >= 0 ? min(s.ell_cnt[rowB[j]], 256) : 0;
        cntA_[j] = cntA, cntB_[j] = cntB;
        int na         = min(cntA, E);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) na = max(na, __shfl_xor(na, o, 64));
        na             = (na + 1) & ~1;  // even: a packed column word never mixes A and B slots
        const int capB = E - na;         // wave-uniform
        const int regB = min(cntB, capB);
        int nb         = regB;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nb = max(nb, __shfl_xor(nb, o, 64));
        // wave-uniform by construction; readfirstlane tells the compiler, so that the slot-range tests of the
        // PCG loop become scalar branches instead of per-lane selects over both accumulators
        nA[j] = __builtin_amdgcn_readfirstlane(na), nB[j] = __builtin_amdgcn_readfirstlane(min((nb + 1) & ~1, capB));
        unfit_any |= cntA > E || cntB > capB;
    }
    // A pair that does not fit E slots (k = 8 graphs always, k = 4 hardly ever): the system is streamed from L2 instead,
    // all three coordinates by the first workgroup — decided from the row lengths alone, before any matrix entry is
    // loaded, and inside this launch.
    if (__syncthreads_or(unfit_any)) {
        if (NC == 3 || blockIdx.x == 0) pcg_stream_body<NT, 2 * P>(s, st, max_iter, pcg_tol, smem);
        return;
    }
    float mval[P][E];
    uint32_t mcol[P][E / 2];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int cntA = cntA_[j], cntB = cntB_[j];
        const int na = nA[j];
        const int regB = min(cntB, E - na);
        const int rA = rowA[j] >= 0 ? rowA[j] : 0, rB = rowB[j] >= 0 ? rowB[j] : 0;
        // values and columns -> registers for the whole solve (slot q: entry q of A for q < nA, entry
        // E-1-q of B otherwise); two 16-bit columns per register
#pragma unroll
        for (int q2 = 0; q2 < E / 2; ++q2) {
            uint32_t packed = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q     = 2 * q2 + h;
                const bool isA  = q < na;
                const int ent   = isA ? q : E - 1 - q;
                const int r     = isA ? rA : rB;
                const bool live = isA ? (q < cntA) : (E - 1 - q < regB);
                const float2 e  = s.ell[(size_t)ent * D + r];  // unconditional 8-byte load, masked after
                float v         = e.x;
                int col         = __float_as_int(e.y);
                if (!live) v = 0.f, col = 0;
                mval[j][q] = v;
                packed |= (uint32_t)(col << (NC == 3 ? 4 : 2)) << (16 * h);  // byte offset of p[col] in LDS
            }
            mcol[j][q2] = packed;
            if ((q2 & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound the loads in flight
        }
    }
    float xA[P][NC], rA_[P][NC], pA[P][NC], xB[P][NC], rB_[P][NC], pB[P][NC], minvA[P], minvB[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        minvA[j] = minvB[j] = 0.f;
        if (rowA[j] >= 0) minvA[j] = jacobi_inv(s.diag[rowA[j]]);
        if (rowB[j] >= 0) minvB[j] = jacobi_inv(s.diag[rowB[j]]);
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) {
            const int c    = c0 + cc;
            const float ga = rowA[j] >= 0 ? s.g[3 * rowA[j] + c] : 0.f;
            const float gb = rowB[j] >= 0 ? s.g[3 * rowB[j] + c] : 0.f;
            xA[j][cc] = xB[j][cc] = 0.f;
            rA_[j][cc] = ga, rB_[j][cc] = gb;
            pA[j][cc] = minvA[j] * ga, pB[j][cc] = minvB[j] * gb;
        }
        if (NC == 3) {
            if (rowA[j] >= 0) p_s[rowA[j]] = make_float4(pA[j][0], pA[j][1], pA[j][NC - 1], 0.f);
            if (rowB[j] >= 0) p_s[rowB[j]] = make_float4(pB[j][0], pB[j][1], pB[j][NC - 1], 0.f);
        } else {
            if (rowA[j] >= 0) p_s1[rowA[j]] = pA[j][0];
            if (rowB[j] >= 0) p_s1[rowB[j]] = pB[j][0];
        }
    }
    __syncthreads();  // p in LDS
    float rz = rz0;   // (NC = 1 forms its own (r, z) inside the loop)
    const float joint  = pcg_joint_target(st, pcg_tol, rz0);
    // NC = 1: this coordinate's share of the joint target; a coordinate already below it does no iteration
    const float target = NC == 3 ? joint : joint * (1.0f / 3.0f);
    int it             = 0;
    const char* pbase   = (const char*)p_s;
#ifdef DFA_PCG_PROFILE
    long long pc_[6] = {0, 0, 0, 0, 0, 0};
    long long last_  = clock64();
#endif
    // a = A p for this thread's rows (p gathered from LDS)
    auto matvec = [&](float (&aA)[P][NC], float (&aB)[P][NC]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
#pragma unroll
            for (int c = 0; c < NC; ++c) aA[j][c] = aB[j][c] = 0.f;
            // Two slots share a packed column word.  The empty asm makes the word opaque per iteration (otherwise
            // the compiler hoists the unpacking out of the PCG loop and doubles the registers the columns occupy)
            // and, being volatile, keeps the slot-range tests below real scalar branches: if-converted they cost
            // a select per slot AND the FMAs of both accumulators (measured: 4.5 VALU per non-zero, now 2).
            auto slots2 = [&](const int q, float (&acc)[NC]) __attribute__((always_inline)) {
                uint32_t cw = mcol[j][q / 2];
                asm volatile("" : "+v"(cw));
                const float v0 = mval[j][q], v1 = mval[j][q + 1];
                if (NC == 3) {
                    const float4 g0 = *(const float4*)(pbase + (cw & 0xffffu));
                    const float4 g1 = *(const float4*)(pbase + (cw >> 16));
                    asm volatile("" ::"v"(g0.w), "v"(g1.w));  // keep ds_read_b128
                    acc[0]      = fmaf(v1, g1.x, fmaf(v0, g0.x, acc[0]));
                    acc[NC / 2] = fmaf(v1, g1.y, fmaf(v0, g0.y, acc[NC / 2]));
                    acc[NC - 1] = fmaf(v1, g1.z, fmaf(v0, g0.z, acc[NC - 1]));
                } else {
                    const float g0 = *(const float*)(pbase + (cw & 0xffffu));
                    const float g1 = *(const float*)(pbase + (cw >> 16));
                    acc[0]         = fmaf(v1, g1, fmaf(v0, g0, acc[0]));
                }
            };
            auto slots4 = [&](const int q, float (&acc)[NC]) __attribute__((always_inline)) {  // 4 gathers in flight
                uint32_t c01 = mcol[j][q / 2], c23 = mcol[j][q / 2 + 1];
                asm volatile("" : "+v"(c01), "+v"(c23));
                const float v0 = mval[j][q], v1 = mval[j][q + 1], v2 = mval[j][q + 2], v3 = mval[j][q + 3];
                if (NC == 3) {
                    const float4 g0 = *(const float4*)(pbase + (c01 & 0xffffu));
                    const float4 g1 = *(const float4*)(pbase + (c01 >> 16));
                    const float4 g2 = *(const float4*)(pbase + (c23 & 0xffffu));
                    const float4 g3 = *(const float4*)(pbase + (c23 >> 16));
                    asm volatile("" ::"v"(g0.w), "v"(g1.w), "v"(g2.w), "v"(g3.w));
                    acc[0]      = fmaf(v3, g3.x, fmaf(v2, g2.x, fmaf(v1, g1.x, fmaf(v0, g0.x, acc[0]))));
                    acc[NC / 2] = fmaf(v3, g3.y, fmaf(v2, g2.y, fmaf(v1, g1.y, fmaf(v0, g0.y, acc[NC / 2]))));
                    acc[NC - 1] = fmaf(v3, g3.z, fmaf(v2, g2.z, fmaf(v1, g1.z, fmaf(v0, g0.z, acc[NC - 1]))));
                } else {
                    const float g0 = *(const float*)(pbase + (c01 & 0xffffu));
                    const float g1 = *(const float*)(pbase + (c01 >> 16));
                    const float g2 = *(const float*)(pbase + (c23 & 0xffffu));
                    const float g3 = *(const float*)(pbase + (c23 >> 16));
                    acc[0]         = fmaf(v3, g3, fmaf(v2, g2, fmaf(v1, g1, fmaf(v0, g0, acc[0]))));
                }
            };
            // row A: slots [0, nA) upwards; row B: slots [E - nB, E) from the top (nA, nB even, wave-uniform).  A row's
            // two-slot remainder is a branch of ITS OWN step, at that step's constant slots: placed behind the break, the
            // remainders of all steps are merged into one block that reads mval at a merged index, and the compiler
            // keeps a second copy of the array in scratch memory for it (DESIGN_NOTES, compiler note).
            // (More gathers in flight per step measured slower, profiles/r10_pcg_gather.md: with rows A and B swept together,
            // 8 ds_read_b32 ahead of the first wait, the C2 frame is 2.6 % longer than with 4.)
#pragma unroll
            for (int q0 = 0; q0 < E; q0 += 4) {
                if (q0 >= nA[j]) break;
                if (q0 + 4 <= nA[j]) slots4(q0, aA[j]);
                else slots2(q0, aA[j]);
            }
#pragma unroll
            for (int q0 = 0; q0 < E; q0 += 4) {
                if (q0 >= nB[j]) break;
                if (q0 + 4 <= nB[j]) slots4(E - 4 - q0, aB[j]);
                else slots2(E - 2 - q0, aB[j]);
            }
        }
    };
    auto publish = [&](const float (&vA)[P][NC], const float (&vB)[P][NC]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            if (NC == 3) {
                if (rowA[j] >= 0) p_s[rowA[j]] = make_float4(vA[j][0], vA[j][NC / 2], vA[j][NC - 1], 0.f);
                if (rowB[j] >= 0) p_s[rowB[j]] = make_float4(vB[j][0], vB[j][NC / 2], vB[j][NC - 1], 0.f);
            } else {
                if (rowA[j] >= 0) p_s1[rowA[j]] = vA[j][0];
                if (rowB[j] >= 0) p_s1[rowB[j]] = vB[j][0];
            }
        }
    };
    if (NC == 3) {
        // textbook PCG: two reductions and the publication of p = three barriers per iteration
        while (it < max_iter) {
            if (!(rz > 0.f)) break;
            PROF_MARK(5);
            float aA[P][NC], aB[P][NC];
            float pap_loc = 0.f;
            matvec(aA, aB);
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int c = 0; c < NC; ++c) pap_loc = fmaf(pA[j][c], aA[j][c], fmaf(pB[j][c], aB[j][c], pap_loc));
            PROF_MARK(0);
            const float pAp = block_sum_f<NT / 64>(pap_loc, red0);
            PROF_MARK(1);
            if (!(pAp > 0.f)) break;
            const float alpha = rz / pAp;
            float rzn_loc     = 0.f;
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    xA[j][c]  = fmaf(alpha, pA[j][c], xA[j][c]);
                    xB[j][c]  = fmaf(alpha, pB[j][c], xB[j][c]);
                    rA_[j][c] = fmaf(-alpha, aA[j][c], rA_[j][c]);
                    rB_[j][c] = fmaf(-alpha, aB[j][c], rB_[j][c]);
                    rzn_loc = fmaf(rA_[j][c], minvA[j] * rA_[j][c], fmaf(rB_[j][c], minvB[j] * rB_[j][c], rzn_loc));
                }
            PROF_MARK(2);
            const float rz_new = block_sum_f<NT / 64>(rzn_loc, red1);
            PROF_MARK(3);
            ++it;
            if (rz_new <= target) break;
            const float beta = rz_new / rz;
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    pA[j][c] = fmaf(beta, pA[j][c], minvA[j] * rA_[j][c]);
                    pB[j][c] = fmaf(beta, pB[j][c], minvB[j] * rB_[j][c]);
                }
            publish(pA, pB);
            rz = rz_new;
            __syncthreads();
            PROF_MARK(4);
        }
    }
    if (NC == 1) {
        // Chronopoulos-Gear form of the same recurrence: the matrix multiplies u = M^-1 r, both inner products
        // (r, u) and (A u, u) come out of ONE reduction, and s = A p follows by recurrence — two barriers per
        // iteration instead of three (a reduction costs ~550 clocks of a ~4 700-clock iteration here).
        // In LDS: u (the prologue stored M^-1 r0).  pA / pB start as the zero direction.
        float sA[P][NC], sB[P][NC], uA[P][NC], uB[P][NC];
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                uA[j][c] = pA[j][c], uB[j][c] = pB[j][c];
                pA[j][c] = pB[j][c] = sA[j][c] = sB[j][c] = 0.f;
            }
        float gamma_old = 1.f, alpha_old = 1.f;
        __syncthreads();  // every wave has read the prologue's sums before red0 / red1 are written again
        while (it < max_iter) {
            PROF_MARK(5);
            float wA[P][NC], wB[P][NC];
            matvec(wA, wB);
            float g_loc = 0.f, d_loc = 0.f;
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    g_loc = fmaf(rA_[j][c], uA[j][c], fmaf(rB_[j][c], uB[j][c], g_loc));
                    d_loc = fmaf(wA[j][c], uA[j][c], fmaf(wB[j][c], uB[j][c], d_loc));
                }
            PROF_MARK(0);
            const float gw = wave_total(g_loc), dw = wave_total(d_loc);
            if ((tid & 63) == 0) red0[tid >> 6] = gw, red1[tid >> 6] = dw;
            __syncthreads();
            float gamma = 0.f, delta = 0.f;
#pragma unroll
            for (int i = 0; i < NT / 64; ++i) gamma += red0[i], delta += red1[i];
            PROF_MARK(1);
            if (!(gamma > target)) break;  // converged: (r, M^-1 r) of the iterate in x
            const float beta  = cg_beta(it == 0, gamma, gamma_old);
            const float denom = cg_denom(it == 0, gamma, delta, beta, alpha_old);
            if (!(denom > 0.f)) break;
            const float alpha = gamma / denom;
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    cg_update_row(alpha, beta, uA[j][c], wA[j][c], pA[j][c], sA[j][c], xA[j][c], rA_[j][c]);
                    cg_update_row(alpha, beta, uB[j][c], wB[j][c], pB[j][c], sB[j][c], xB[j][c], rB_[j][c]);
                    uA[j][c]  = minvA[j] * rA_[j][c];
                    uB[j][c]  = minvB[j] * rB_[j][c];
                }
            ++it;
            gamma_old = gamma, alpha_old = alpha;
            PROF_MARK(2);
            publish(uA, uB);  // every wave is past this iteration's gather (the reduction's barrier)
            __syncthreads();
            PROF_MARK(4);
        }
    }
#ifdef DFA_PCG_PROFILE
    if (tid == 0 && c0 == 0)
        for (int i = 0; i < 6; ++i) st->prof[i] += pc_[i];
#endif
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (rowA[j] >= 0) s.t[3 * rowA[j] + c0 + c] += xA[j][c];
            if (rowB[j] >= 0) s.t[3 * rowB[j] + c0 + c] += xB[j][c];
        }
    if (tid == 0) {
        if (NC == 3) pcg_book_launch(st, rz0, it, false);
        else pcg_book_launch_of_three(st, rz0, it, false);
    }
}

// ------------------------------------------------------------------------------------------
// launchers

int solve_pcg_max_nodes() { return 32768; }  // bounded by the transposition's LDS histogram (4 B x D)

// register-resident kernel: NT threads own 2*NT rows, a pair of rows in E matrix slots per thread
// (NC = 3: one workgroup for the joint system; NC = 1: three workgroups, one coordinate each)
template <int NT, int E, int NC>
static hipError_t launch_paired_pcg(const SolveView& s, SolveState* state, int max_iter, float pcg_tol,
                                    hipStream_t st) {
    hipError_t e = allow_big_lds(pcg_paired_kernel<NT, E, NC>);
    if (e != hipSuccess) return e;
    const size_t sh = sizeof(float4) * (size_t)s.Dpad + 32 * sizeof(float) + sizeof(int) * (260 + (size_t)s.Dpad * (s.deterministic ? 2 : 1));
    pcg_paired_kernel<NT, E, NC><<<NC == 1 ? 3 : 1, NT, sh, st>>>(s, state, max_iter, pcg_tol);
    return hipGetLastError();
}

// The PCG of one linearisation.  Up to 2 048 nodes: the register-resident kernel, one workgroup per coordinate (a system
// that does not fit the registers is streamed inside the same launch); above: the many-workgroup PCG, which reads the
// assembled ELL directly (the single-workgroup streaming kernel spends ~1 ms per launch sorting and repacking the matrix
// by itself at 8 k nodes).
// Development builds (-DDFA_DEV_AB) also hold the forms the tests compare against, selected by DFA_PCG_VARIANT (read at
// every call: the tests switch it): 1 register-resident with the three coordinates in ONE workgroup (shared CG scalars,
// as the oracle), 3 many-workgroup at any size.
// May this plan's PCG take the team form now?  gave_up: it could, but a team of an earlier launch (placement, starvation, a
// row too long) has said so in pinned memory — no synchronisation: the word is read as it stands.
// (development builds: DFA_MB_TEAM=0 the launched form, =2 the team form at any size)
enum class TeamUse { no, yes, gave_up };
static TeamUse team_pcg_use(const TeamPcg* team, int D, int max_iter) {
    if (!(team && team->ctl && !team->disabled && solve_team_pcg_fits(D) && max_iter < solve_team_pcg_rounds() && dev_env_int("DFA_MB_TEAM", 1) != 0))
        return TeamUse::no;
    return team->host_abort && *(volatile int*)team->host_abort != 0 ? TeamUse::gave_up : TeamUse::yes;
}

static hipError_t route_pcg(const SolveView& s, SolveState* state, int max_iter, float pcg_tol, int* host_flag, MbGraphCache* gc,
                            TeamPcg* team, hipEvent_t& main_done, hipStream_t st) {
    const int D = s.D;
#ifdef DFA_DEV_AB
    const int v2 = dev_env_int("DFA_PCG_VARIANT", -1);
    if (dev_env_int("DFA_MB_TEAM", 1) == 2 && team_pcg_use(team, D, max_iter) == TeamUse::yes)
        return launch_team_pcg(s, state, max_iter, pcg_tol, team, st);
    if (v2 == 3) return launch_mb_pcg(s, state, max_iter, pcg_tol, host_flag, gc, st);
    if (v2 == 1 && D <= 1024) return launch_paired_pcg<512, 64, 3>(s, state, max_iter, pcg_tol, st);
    if (v2 == 1 && D <= 2048) return launch_paired_pcg<1024, 32, 3>(s, state, max_iter, pcg_tol, st);
#endif
    // 512 threads leave 256 VGPRs per lane (64 slots per row pair: k = 8 rows fit), 1024 threads 128 VGPRs (32 slots: k = 4)
    if (D <= 1024) return launch_paired_pcg<512, 64, 1>(s, state, max_iter, pcg_tol, st);
    if (D <= 2048) return launch_paired_pcg<1024, 32, 1>(s, state, max_iter, pcg_tol, st);
    const TeamUse use = team_pcg_use(team, D, max_iter);
    if (use == TeamUse::yes) return launch_team_pcg(s, state, max_iter, pcg_tol, team, st);
    if (use == TeamUse::gave_up) team->disabled = true;  // from then on this plan takes the launched form
    return launch_mb_pcg(s, state, max_iter, pcg_tol, host_flag, gc, st);
}

// does the PCG of this plan run without any host synchronisation (the register-resident kernels, the team form)?  The
// launched many-workgroup form reads its stop flag back once per chunk of launches — and the plan's `converged` flag with it.
bool solve_pcg_is_async(const SolveView& s, const TeamPcg* team, int max_iter) {
    if (s.D <= 2048) return dev_env_int("DFA_PCG_VARIANT", -1) != 3;
    return dev_env_int("DFA_PCG_VARIANT", -1) != 3 && team_pcg_use(team, s.D, max_iter) == TeamUse::yes;
}

hipError_t solve_pcg(const SolveView& s, SolveState* state, int max_iter, float pcg_tol, int* host_flag, MbGraphCache* gc,
                     TeamPcg* team, hipEvent_t main_done, hipStream_t st) {
    const hipError_t e = route_pcg(s, state, max_iter, pcg_tol, host_flag, gc, team, main_done, st);
    if (main_done) (void)hipEventRecord(main_done, st);  // paths without a fallback launch
    return e;
}

__global__ void count_noop_kernel(SolveState* __restrict__ st, int n) { st->gn_iters += n, st->gn_noop += n; }
hipError_t solve_count_noop(SolveState* state, int n, hipStream_t st) {
    count_noop_kernel<<<1, 1, 0, st>>>(state, n);
    return hipGetLastError();
}

}  // namespace dfa
