// solve_assemble.hip — assembly of the sparse normal equations of the reference-mode solve, A = sum_rows tau w w^T and
// g = sum_rows tau w e (formulation: solve.hpp), once per linearisation: a gather, not a scatter — ONE WORKGROUP PER NODE
// reduces the node's rows (transpose graph: solve_graph.hip; row records: solve_rows.hpp) into an LDS hash keyed by column
// (fixed-point LDS atomics stay on the CU; no global atomics on the matrix at all) and writes one ELL row + one rhs entry +
// the Jacobi diagonal.  assemble_kernel, and assemble_det_kernel for the order-stable variant.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev_switch.hpp"
#include "device_math.hpp"
#include "solve.hpp"
#include "solve_internal.hpp"
#include "solve_rows.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------
// assembly: one 256-thread workgroup per node.  Its ~128 k rows (transpose graph) are spread
// over the 4 waves, every row contributes k (column, tau w_a w_b) pairs to an LDS hash keyed by
// column; the four waves then compact the hash into the node's ELL row, ascending by column.  Each row is one packed record
// (k ids, k weights, e, tau) read with 16-byte loads from a single cache line.

constexpr int HASH      = 512;
constexpr int HASH_MASK = HASH - 1;

// The hash's sums are 64-bit FIXED-POINT integers, not floats.  On gfx950 an LDS float add (ds_add_f32) executes one lane
// after the other whatever the addresses — 192 cycles per wave instruction against 8 for ds_add_u64 without conflicts
// (tools/microbench_lds_atomic.hip) — and 7 of them per row were 56 % of this kernel's time (C4: 345 -> 152 us with the adds
// taken out).  An addend tau w_a w_b is a float whose magnitude is at most `amax` = the largest tau (max_j |w_j|)^2 of any
// row under the current robust weights (data rows: RBF and Tukey weights <= 1; regularisation rows: +-1 x w_reg^2) — found
// by the linearisation that evaluates those weights (SolveState::amax), so the grid follows the PROBLEM's scale: weights
// that are all tiny (sparse nodes, a narrow dg_w) or a huge lambda cost no bits.  Scaled by 2^40 / (amax rounded up to a
// power of two) an addend is an exact integer unless it is below 2^-17 of that bound (then it is cut to the grid: 2^-41 of
// the bound per addend).  The sum of up to 2^22 rows fits 63 bits, is EXACT otherwise, and does not depend on the order of
// the adds.
struct FixedScale {
    float up;     // float -> fixed: a power of two
    double down;  // fixed -> float
};
__device__ __forceinline__ FixedScale solve_fixed_scale(float amax) {
    int e = 0;
    (void)frexpf(fmaxf(amax, 1e-30f), &e);  // amax < 2^e
    e = e < -80 ? -80 : e > 100 ? 100 : e;
    FixedScale f;
    f.up   = ldexpf(1.f, 40 - e);
    f.down = ldexp(1.0, e - 40);
    return f;
}
// a node with more than 2^22 rows (a plan of millions of vertices on a handful of nodes) gives up one bit of the grid per
// doubling of its list instead of overflowing
__device__ __forceinline__ FixedScale fixed_scale_for_rows(FixedScale f, int rows) {
    const int extra = 32 - __clz((unsigned)max(rows, 1) >> 22);  // 0 up to 2^22 - 1 rows
    if (extra > 0) f.up = ldexpf(f.up, -extra), f.down = ldexp(f.down, extra);
    return f;
}
// The magnitude |v| up goes to `cell` (v >= 0: every data row) or to the cell HASH entries further on (v < 0: the
// off-diagonal entries of regularisation rows); the sum is their difference.  Converting a NON-NEGATIVE integer-valued
// float x to 64 bits takes 7 instructions — hi = floor(x / 2^32) and lo = x - hi 2^32 in [0, 2^32) are exact (a power-of-two
// scaling; x with its high bits removed has no more significant bits than x), and the integer is the register pair
// {lo, hi} — where the compiler's signed conversion takes 13 (absolute value, two floors, a sign fix-up with carries).
__device__ __forceinline__ void fixed_add(long long* cell, float v, float up) {
    const float x  = truncf(fabsf(v) * up);
    const float hf = floorf(x * 2.3283064365386963e-10f);  // 2^-32
    const uint32_t hi = (uint32_t)hf, lo = (uint32_t)fmaf(hf, -4294967296.f, x);
    atomicAdd(reinterpret_cast<unsigned long long*>(v < 0.f ? cell + HASH : cell), ((unsigned long long)hi << 32) | lo);
}

#ifdef DFA_PCG_PROFILE  // development builds: a workgroup's life in the assembly (tools/ref_assemble_phases.py)
__device__ unsigned long long asm_tbuf[32768 * 8];
extern "C" __attribute__((visibility("default"))) int dfa_dev_asm_timing(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(asm_tbuf), sizeof(unsigned long long) * 8 * (size_t)n);
}
#endif

// ------------------------------------------------------------------------------------------
// Behind a linearisation that ends with its rows (the hand-off: solve_linearise.hip, header comment) the assembly launch
// has the linearisation's nb per-workgroup partials (cost_partials != nullptr) in front of it instead of a finished
// SolveState, and takes over two jobs.
//
// 1. Every workgroup forms amax itself: a thread's share of the nb <= LIN_MAX_BLOCKS maxima — four neighbouring floats,
//    one 16-byte load, those past nb masked (the array is LIN_MAX_BLOCKS long whatever nb) — is asked for beside the
//    node_ptr / node_list loads of its init, reduced by wave and handed through LDS across the barrier the init has
//    anyway.  A maximum does not depend on the order, none is negative, and the floats are the doubles that the booking
//    workgroup reduces: the bits of SolveState::amax.
__device__ __forceinline__ float amax_partials_load(const double* cost_partials, int nb) {
    static_assert(LIN_MAX_BLOCKS == 4 * 256, "one float4 per thread of a 256-thread workgroup");
    const float4 m = reinterpret_cast<const float4*>(lin_max_floats(cost_partials))[threadIdx.x];
    const int i    = 4 * (int)threadIdx.x;
    return fmaxf(fmaxf(i < nb ? m.x : 0.f, i + 1 < nb ? m.y : 0.f), fmaxf(i + 2 < nb ? m.z : 0.f, i + 3 < nb ? m.w : 0.f));
}
// (the wave's maximum by the six DPP steps of wave_total, device_math.hpp: a lane without a source reads 0, which no
// maximum of non-negative numbers minds)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max0(float v) {
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false)));
}
__device__ __forceinline__ void amax_partials_publish(float am, float* amax_w /*[4], LDS: read behind the next barrier*/) {
    am = dpp_max0<0x111, 0xf>(am), am = dpp_max0<0x112, 0xf>(am), am = dpp_max0<0x114, 0xf>(am), am = dpp_max0<0x118, 0xf>(am);
    am = dpp_max0<0x142, 0xa>(am), am = dpp_max0<0x143, 0xc>(am);
    // the wave's number and its maximum are scalars, and every lane stores the one word: a lane test here would be the
    // kernel's `lane` and `wave` computed early and held in two vector registers across the whole list
    const float wave_max = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(am), 63));
    amax_w[__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6] = wave_max;
}
// (the same number in every lane: handed to the scalar unit, so that the scale derived from it costs no vector registers)
__device__ __forceinline__ float amax_partials_collect(const float* amax_w) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fmaxf(fmaxf(amax_w[0], amax_w[1]), fmaxf(amax_w[2], amax_w[3])))));
}
// 2. One extra workgroup (index D) books the cost: what the linearisation's last workgroup does in the other form — the
//    same clamped loads, masked adds in index order and 256-wide tree (lin_sum_partials), the same state update
//    (lin_book_cost) — in front of the `done` / `converged` test of the entry, and only if the linearisation really ran
//    (SolveState::lin_pending: one that returned at entry has left the partials of an earlier launch).  It writes `done`
//    = 0 while the other workgroups read `done`: with gn_tol == 0, the only launches that hand off, nothing ever sets it.
//    (sm, smx: 256 doubles each — the workgroup's hash values, which it has no other use for)
__device__ __forceinline__ void assemble_book_cost(SolveState* st, const double* cost_partials, int nb, double* sm, double* smx) {
    if (!st->lin_pending) return;
    lin_sum_partials<false>(cost_partials, (unsigned int)nb, true, sm, smx);
    if (threadIdx.x == 0) {
        lin_book_cost(st, sm[0], smx[0], 1, 0, 0.f, false);
        st->lin_pending = 0;
    }
}

// One list entry of node a — slot `slot` of a row whose record is (idx, w, et = (e.x, e.y, e.z, tau)): its share of the gradient
// and of the diagonal into the thread's registers, its off-diagonal pairs into the hash.
template <int K>
__device__ __forceinline__ void assemble_entry(int a, int slot, const int (&idx)[K], const float (&w)[K], float4 et, float up, int* key,
                                               long long* val, int* ovf, float& gx, float& gy, float& gz, float& dsum) {
    float wa = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) wa = (j == slot) ? w[j] : wa;
    const float tw = et.w * wa;
    gx += tw * et.x, gy += tw * et.y, gz += tw * et.z;
    if (et.w == 0.f) return;
    // first probe of all k columns read together (keys never change once set): the common
    // case "column already present" costs one LDS read + one fire-and-forget ds_add instead
    // of a returning CAS per column
    // (measured and not kept, tools/ref_assemble_phases.py at C4 / C3: every lane taking its columns in the order
    // (lane + t) mod K, so that a step's adds spread over K addresses — 149 / 86 us against 141 / 81, the selects cost
    // more than the conflicts)
    uint32_t h0[K];
    int k0[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        h0[j] = ((uint32_t)idx[j] * 2654435761u) >> (32 - 9);
        k0[j] = key[h0[j]];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int b = idx[j];
        if (b < 0) continue;
        const float v = tw * w[j];
        if (b == a) {  // the diagonal is hit by every row: kept in a register
            dsum += v;
            continue;
        }
        if (k0[j] == b) {  // the column is in the table where its first probe looks: nearly every pair after the first rows
            fixed_add(&val[h0[j]], v, up);
            continue;
        }
        uint32_t h = h0[j];
        int cur    = k0[j];
#pragma unroll 1
        for (int probes = 0;; ++probes) {
            if (cur == -1) cur = atomicCAS(&key[h], -1, b), cur = cur == -1 ? b : cur;
            if (cur == b) {
                fixed_add(&val[h], v, up);
                break;
            }
            if (probes >= HASH) {
                *ovf = 1;
                break;
            }
            h   = (h + 1) & HASH_MASK;
            cur = key[h];
        }
    }
}

// A node's list is walked in one of two forms, T the template's choice:
//   T == 1  the plain loop: a thread's entries one after the other, each a chain node_list[p] -> row record -> hash adds.
//           With its ~36 registers the most workgroups are resident, which is what counts where a grid runs in several
//           rounds (measured at C4 / C3, tools/ref_assemble_phases.py: a thread's rows 2 or 4 at a time with their loads
//           in flight together — a workgroup lives 18 us instead of 23 but fewer are resident: 140-163 / 81-91 us
//           against 141 / 81).
//   T > 1   the list in flight: a thread's entries in chunks of T (256 T entries per workgroup and chunk) — the T
//           node_list entries together (addresses clamped into the list, entries past its end masked), then the T row
//           records together, and only then the hash work, in the order p, p + 256, ... of the plain loop, so that every
//           float sum of a thread sees the same addends in the same order (the fixed-point sums do not depend on order).
//           The first chunk's entries are asked for in front of the hash initialisation, which they do not depend on.
//           For a grid that is resident in ONE round (solve_assemble_resident_blocks; C2: 2 048 workgroups = 256 CUs x 8),
//           where the launch lasts as long as its slowest workgroup and a list of ~520 entries (C2: 302 ... 651) is
//           1 + 2 dependent round trips instead of 1 + 2 x 3.  It must stay within 64 VGPRs: the residency of the plain loop
//           (K = 4, T = 3: 64 VGPRs, no scratch, 8 waves per SIMD; it is launched for k == K only, so that the record is
//           its three 16-byte loads and nothing else of load_record).  Measured at C2: 114.3 -> 99.4 us per frame of five
//           launches, a workgroup's list + hash phase 11.1 -> 9.4 us (profiles/r11_assembly_in_flight.md; the same
//           profile shows a fifth of the C2 grid starting only when the first workgroups leave, in either form, whatever
//           the occupancy query says: not explained yet).
template <int K, int T>
__global__ __launch_bounds__(256) void assemble_kernel(SolveView s, SolveState* __restrict__ st, int save_base, float amax_unset,
                                                       const double* __restrict__ cost_partials /* the hand-off, or nullptr */) {
    __shared__ int key[HASH];
    __shared__ long long val[2 * HASH];  // [0, HASH): sums of the non-negative addends, [HASH, 2 HASH): of the negative ones' magnitudes
    __shared__ float gpart[4][3];
    __shared__ float amax_w[4];
    __shared__ int wave_cnt[4];
    __shared__ int ovf;
    if ((int)blockIdx.x == s.D) {  // the booking workgroup (launched only with the hand-off)
        assemble_book_cost(st, cost_partials, lin_blocks(s.N, s.D, s.k), reinterpret_cast<double*>(val), reinterpret_cast<double*>(val) + 256);
        return;
    }
    if (st->done || st->converged) return;
    // (workgroup -> node in launch order.  A contiguous node range per XCD — so that the rows a node shares with its
    // neighbours are fetched into one L2 instead of up to eight — left the launch at 345 us at C4: it was never bound by
    // the fetches; profiles/r06_xcd_map.md.)
    const int a = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#ifdef DFA_PCG_PROFILE
    long long t0_ = clock64(), t1_, t2_, t3_, t4_;
    const unsigned long long w0_ = wall_clock64();
#endif
    const int beg = s.node_ptr[a], end = s.node_ptr[a + 1];
    [[maybe_unused]] uint32_t ent[T];
    if constexpr (T > 1) {  // (an empty list reads entry 0 of the array, which every plan has, and uses nothing of it)
#pragma unroll
        for (int t = 0; t < T; ++t) ent[t] = s.node_list[max(min(beg + 256 * t + (int)threadIdx.x, end - 1), 0)];
    }
    float amax_st = cost_partials ? amax_partials_load(cost_partials, lin_blocks(s.N, s.D, s.k)) : st->amax;
    for (int i = threadIdx.x; i < HASH; i += 256) key[i] = -1, val[i] = val[i + HASH] = 0ll;
    if (threadIdx.x == 0) ovf = 0;
    if (cost_partials) amax_partials_publish(amax_st, amax_w);
    __syncthreads();
    if (cost_partials) amax_st = amax_partials_collect(amax_w);
#ifdef DFA_PCG_PROFILE
    t1_ = clock64();
#endif

    const FixedScale fx = fixed_scale_for_rows(solve_fixed_scale(amax_st > 0.f ? amax_st : amax_unset), end - beg);
    float gx = 0.f, gy = 0.f, gz = 0.f, dsum = 0.f;
    if constexpr (T > 1) {
        SolveView sk = s;  // (this form is launched for k == K only: the record's 16-byte loads and nothing else of load_record)
        sk.k         = K;
        for (int base = beg + (int)threadIdx.x; base - (int)threadIdx.x < end; base += 256 * T) {
            if (base - (int)threadIdx.x != beg) {
#pragma unroll
                for (int t = 0; t < T; ++t) ent[t] = s.node_list[min(base + 256 * t, end - 1)];
            }
            int slot[T], idx[T][K];
            float w[T][K];
            float4 et[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const size_t r = ent[t] / (uint32_t)K;
                slot[t]        = (int)(ent[t] - (uint32_t)r * (uint32_t)K);
                et[t]          = load_record<K>(sk, r, idx[t], w[t]);  // (e.x, e.y, e.z, tau)
            }
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (base + 256 * t < end) assemble_entry<K>(a, slot[t], idx[t], w[t], et[t], fx.up, key, val, &ovf, gx, gy, gz, dsum);
        }
    } else {
        for (int p = beg + (int)threadIdx.x; p < end; p += 256) {
            const uint32_t e = s.node_list[p];
            const size_t r   = e / (uint32_t)s.k;
            const int slot   = (int)(e - (uint32_t)r * (uint32_t)s.k);
            int idx[K];
            float w[K];
            const float4 et = load_record<K>(s, r, idx, w);  // (e.x, e.y, e.z, tau)
            assemble_entry<K>(a, slot, idx, w, et, fx.up, key, val, &ovf, gx, gy, gz, dsum);
        }
    }
    // the diagonal: one add per wave into its (pre-inserted) slot
    dsum = wave_total(dsum);
    if (lane == 0 && dsum != 0.f) {
        uint32_t h = ((uint32_t)a * 2654435761u) >> (32 - 9);
        for (int probes = 0; probes < HASH; ++probes, h = (h + 1) & HASH_MASK) {
            const int cur = atomicCAS(&key[h], -1, a);
            if (cur == -1 || cur == a) {
                fixed_add(&val[h], dsum, fx.up);
                break;
            }
        }
    }
#ifdef DFA_PCG_PROFILE
    t2_ = clock64();
#endif
    gx = wave_total(gx), gy = wave_total(gy), gz = wave_total(gz);
    if (lane == 0) gpart[wave][0] = gx, gpart[wave][1] = gy, gpart[wave][2] = gz;
    __syncthreads();
#ifdef DFA_PCG_PROFILE
    t3_ = clock64();
#endif
    // compact the hash into the ELL row (slot-major: entry q of row a at [q*D + a]: a slot of all rows is one
    // contiguous 8*D-byte segment), entries in ascending column order:
    // the PCG gathers p[col] of 64 rows per wave instruction, and rows sorted by column spread those reads over
    // the LDS banks (hash order: 5.38 clocks per wave instruction on the C2 tables, sorted: 3.90).  Each wave owns
    // HASH/4 consecutive hash slots (two per lane, held in registers); the valid keys are first packed into key[0,
    // total) in slot order, then every key's place is the number of smaller keys in the row (~15, broadcast reads).
    constexpr int PER_WAVE = HASH / 4;
    constexpr int PER_LANE = PER_WAVE / 64;
    int kk[PER_LANE];
    float vv[PER_LANE];
    int wcnt = 0;
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int hq = wave * PER_WAVE + 64 * i + lane;
        kk[i]        = key[hq];
        vv[i]        = (float)((double)(val[hq] - val[hq + HASH]) * fx.down);
        wcnt += __popcll(__ballot(kk[i] >= 0));
    }
    if (lane == 0) wave_cnt[wave] = wcnt;
    __syncthreads();  // (also: every wave has read its hash slots before key[] is overwritten below)
    int pos0 = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        pos0 += w < wave ? wave_cnt[w] : 0;
        total += wave_cnt[w];
    }
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const uint64_t m = __ballot(kk[i] >= 0);
        if (kk[i] >= 0) key[pos0 + __popcll(m & ((1ull << lane) - 1ull))] = kk[i];
        pos0 += __popcll(m);
    }
    __syncthreads();
    int rank[PER_LANE] = {};
    for (int q = 0; q < total; ++q) {
        const int kq = key[q];
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) rank[i] += kq < kk[i];
    }
    float diag = 0.f;
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        if (kk[i] < 0) continue;
        if (rank[i] < s.ell_cap) s.ell[(size_t)rank[i] * s.D + a] = make_float2(vv[i], __int_as_float(kk[i]));
        if (kk[i] == a) s.diag[a] = vv[i], diag = 1.f;
    }
    const bool has_diag = __syncthreads_or(diag != 0.f);
    if (threadIdx.x == 0) {
        s.ell_cnt[a] = min(total, s.ell_cap);
        if (!has_diag) s.diag[a] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gc = (gpart[0][c] + gpart[1][c]) + (gpart[2][c] + gpart[3][c]);
            s.g[3 * a + c] = gc;
            if (save_base) s.g_base[3 * a + c] = gc, s.t_base[3 * a + c] = s.t[3 * a + c];
        }
        // 2048 device-scope atomics on one word cost ~11 ns each: only the (few) blocks that raise
        // the running maximum issue one
        if (total > *(volatile int*)&st->max_row_nnz) atomicMax(&st->max_row_nnz, total);
        if (total > s.ell_cap || ovf) st->overflow = 1;
#ifdef DFA_PCG_PROFILE
        t4_ = clock64();
        if (a == 7 && !s.team_ctl) st->prof[6] = (t1_ - t0_) * 1000000 + (t2_ - t1_), st->prof[7] = (t3_ - t2_) * 1000000 + (t4_ - t3_);  // (plans with a team PCG: its own counters)
        if (a < 32768) {
            unsigned long long* o = asm_tbuf + 8 * (size_t)a;
            o[0] = w0_, o[1] = wall_clock64() - w0_, o[2] = (unsigned long long)(end - beg), o[3] = (unsigned long long)total;
            o[4] = t1_ - t0_, o[5] = t2_ - t1_, o[6] = t3_ - t2_, o[7] = t4_ - t3_;
        }
#endif
    }
}

// ------------------------------------------------------------------------------------------
// Order-stable variant (SolveView::deterministic).  Both assemblies sum the off-diagonal entries on the fixed-point grid
// and write every row in ascending column order: those bits are the same (tests/test_gpu_pcg_sorted_rows.py).  Three
// things still make two runs of the default path differ in the last bits: the transposition fills a node's row list in
// the order its LDS cursor atomics land, and that order feeds the float sums of the gradient and the diagonal; the
// diagonal's four wave sums are added in float here, on the fixed-point grid above; and the PCG kernels place rows of
// equal length by an atomic cursor (which thread owns which row decides the order of the inner products' partial
// sums).  Here: lists sorted (sort_node_lists_kernel, solve_graph.hip), float sums per wave added in wave order, equal-length rows in index order.
template <int K>
__global__ __launch_bounds__(256) void assemble_det_kernel(SolveView s, SolveState* __restrict__ st, int save_base, float amax_unset,
                                                           const double* __restrict__ cost_partials /* the hand-off, or nullptr */) {
    __shared__ int key[HASH];
    __shared__ long long val[2 * HASH];  // fixed-point sums (see FixedScale, fixed_add): integer adds commute, any order gives the same bits
    __shared__ float gpart[4][3], dpart[4], amax_w[4];
    __shared__ int ovf, nkeys;
    if ((int)blockIdx.x == s.D) {  // the booking workgroup (launched only with the hand-off)
        assemble_book_cost(st, cost_partials, lin_blocks(s.N, s.D, s.k), reinterpret_cast<double*>(val), reinterpret_cast<double*>(val) + 256);
        return;
    }
    if (st->done || st->converged) return;
    const int a    = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float amax_st  = cost_partials ? amax_partials_load(cost_partials, lin_blocks(s.N, s.D, s.k)) : st->amax;
    for (int i = threadIdx.x; i < HASH; i += 256) key[i] = -1, val[i] = val[i + HASH] = 0ll;
    if (threadIdx.x == 0) ovf = 0, nkeys = 0;
    if (cost_partials) amax_partials_publish(amax_st, amax_w);
    __syncthreads();
    if (cost_partials) amax_st = amax_partials_collect(amax_w);
    const int beg = s.node_ptr[a], end = s.node_ptr[a + 1];
    const FixedScale fx = fixed_scale_for_rows(solve_fixed_scale(amax_st > 0.f ? amax_st : amax_unset), end - beg);
    // pass 1: the set of columns (keys only), the gradient and the diagonal
    float gx = 0.f, gy = 0.f, gz = 0.f, dsum = 0.f;
    for (int p = beg + (int)threadIdx.x; p < end; p += 256) {
        const uint32_t e = s.node_list[p];
        const size_t r   = e / (uint32_t)s.k;
        const int slot   = (int)(e - (uint32_t)r * (uint32_t)s.k);
        int idx[K];
        float w[K];
        const float4 et = load_record<K>(s, r, idx, w);
        float wa = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) wa = (j == slot) ? w[j] : wa;
        const float tw = et.w * wa;
        gx += tw * et.x, gy += tw * et.y, gz += tw * et.z;
        if (et.w != 0.f) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int b = idx[j];
                if (b < 0) continue;
                if (b == a) {
                    dsum += tw * w[j];
                    continue;
                }
                uint32_t h = ((uint32_t)b * 2654435761u) >> (32 - 9);
                for (int probes = 0;; ++probes) {
                    const int cur = atomicCAS(&key[h], -1, b);
                    if (cur == -1 || cur == b) break;
                    if (probes >= HASH) {
                        ovf = 1;
                        break;
                    }
                    h = (h + 1) & HASH_MASK;
                }
            }
        }
    }
    dsum = wave_total(dsum), gx = wave_total(gx), gy = wave_total(gy), gz = wave_total(gz);
    if (lane == 0) dpart[wave] = dsum, gpart[wave][0] = gx, gpart[wave][1] = gy, gpart[wave][2] = gz;
    __syncthreads();
    const float dtot = (dpart[0] + dpart[1]) + (dpart[2] + dpart[3]);
    if (threadIdx.x == 0 && dtot != 0.f) {  // the diagonal is a column like the others (as in assemble_kernel: only if non-zero)
        uint32_t h = ((uint32_t)a * 2654435761u) >> (32 - 9);
        for (int probes = 0; probes < HASH; ++probes, h = (h + 1) & HASH_MASK)
            if (key[h] == -1) {
                key[h] = a;
                break;
            }
    }
    __syncthreads();
    // pass 2: the values, into this wave's copy (the slot of a column: read-only probes now)
    for (int p = beg + (int)threadIdx.x; p < end; p += 256) {
        const uint32_t e = s.node_list[p];
        const size_t r   = e / (uint32_t)s.k;
        const int slot   = (int)(e - (uint32_t)r * (uint32_t)s.k);
        int idx[K];
        float w[K];
        const float4 et = load_record<K>(s, r, idx, w);
        if (et.w == 0.f) continue;
        float wa = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) wa = (j == slot) ? w[j] : wa;
        const float tw = et.w * wa;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int b = idx[j];
            if (b < 0 || b == a) continue;
            uint32_t h = ((uint32_t)b * 2654435761u) >> (32 - 9);
            for (int probes = 0; probes <= HASH && key[h] != b; ++probes) h = (h + 1) & HASH_MASK;
            if (key[h] == b) fixed_add(&val[h], tw * w[j], fx.up);
        }
    }
    __syncthreads();
    // output: entry of column c at the position of c among the row's columns (ascending)
    int total = 0;
    for (int i = threadIdx.x; i < HASH; i += 256) total += key[i] >= 0;
    total = (int)wave_total((float)total);
    if (lane == 0) atomicAdd(&nkeys, total);
    __syncthreads();
    total = nkeys;
    bool has_diag = false;
    for (int i = threadIdx.x; i < HASH; i += 256) {
        const int kk = key[i];
        if (kk < 0) continue;
        int pos = 0;
        for (int q = 0; q < HASH; ++q) pos += key[q] >= 0 && key[q] < kk;
        const float vv = kk == a ? dtot : (float)((double)(val[i] - val[i + HASH]) * fx.down);
        if (pos < s.ell_cap) s.ell[(size_t)pos * s.D + a] = make_float2(vv, __int_as_float(kk));
        if (kk == a) s.diag[a] = vv, has_diag = true;
    }
    const bool any_diag = __syncthreads_or(has_diag);
    if (threadIdx.x == 0) {
        s.ell_cnt[a] = min(total, s.ell_cap);
        if (!any_diag) s.diag[a] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gc = (gpart[0][c] + gpart[1][c]) + (gpart[2][c] + gpart[3][c]);
            s.g[3 * a + c] = gc;
            if (save_base) s.g_base[3 * a + c] = gc, s.t_base[3 * a + c] = s.t[3 * a + c];
        }
        if (total > *(volatile int*)&st->max_row_nnz) atomicMax(&st->max_row_nnz, total);
        if (total > s.ell_cap || ovf) st->overflow = 1;
    }
}

// ------------------------------------------------------------------------------------------
// launcher

// entries of a thread in flight together, per template K (1: that K has the plain loop only).  K = 8 and 16 hold 16 and 28
// record words per entry: two entries in flight cost them waves (K = 8: 52 -> 76 VGPRs, 8 -> 6 waves per SIMD; K = 16:
// 85 -> 130, 5 -> 3), so they keep the plain loop.
constexpr int asm_chunk(int K) { return K == 4 ? 3 : 1; }

template <int K>
static int resident_blocks_of() {
    if (asm_chunk(K) == 1) return 0;
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, assemble_kernel<K, asm_chunk(K)>, 256, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;  // (unknown: the plain loop)
    }
    return cus * per_cu;
}

int solve_assemble_resident_blocks(int k) {
    return k <= 4 ? resident_blocks_of<4>() : k <= 8 ? resident_blocks_of<8>() : resident_blocks_of<16>();
}

template <int K>
static void launch_assemble(const SolveView& s, SolveState* state, int save_base, float amax_unset, bool in_flight, const double* partials,
                            int nb, hipStream_t st) {
    const int grid = s.D + (nb > 0 ? 1 : 0);  // (the hand-off's booking workgroup: the last index)
    if (asm_chunk(K) > 1 && in_flight && s.k == K) assemble_kernel<K, asm_chunk(K)><<<grid, 256, 0, st>>>(s, state, save_base, amax_unset, partials);
    else assemble_kernel<K, 1><<<grid, 256, 0, st>>>(s, state, save_base, amax_unset, partials);
}

hipError_t solve_assemble(const SolveView& s, SolveState* state, int save_base, float w_reg_sq, int resident_blocks,
                          const double* handoff_partials, hipStream_t st) {
    // The rows carry w_reg^2 as their tau; the scale of the fixed-point sums comes from SolveState::amax, which the
    // re-weighting linearisation in front of this launch has found.  Should no such linearisation have stored one (amax is
    // still the 0 of solve_reset — nothing in the driver does that today), the sums take the bound every addend obeys,
    // max(1, w_reg^2), instead of a grid for addends of 1e-30 that the first real one would overflow.
    const float amax_unset = std::max(1.0f, w_reg_sq);
    const int nb           = handoff_partials ? solve_residual_blocks(s) : 0;  // the linearisation's workgroups
    if (s.deterministic) KDISPATCH(assemble_det_kernel, s.k, <<<s.D + (nb > 0 ? 1 : 0), 256, 0, st>>>(s, state, save_base, amax_unset, handoff_partials));
    else {
        // the list in flight only where the whole grid is resident in one round; larger plans keep the plain loop, which
        // won there (assemble_kernel).  DFA_ASM_IN_FLIGHT=0 / 1 (development builds): one form for every plan (A/B, tests).
        bool in_flight  = s.D <= resident_blocks;
        const int force = dev_env_int("DFA_ASM_IN_FLIGHT", -1);
        if (force >= 0) in_flight = force != 0;
        if (s.k <= 4) launch_assemble<4>(s, state, save_base, amax_unset, in_flight, handoff_partials, nb, st);
        else if (s.k <= 8) launch_assemble<8>(s, state, save_base, amax_unset, in_flight, handoff_partials, nb, st);
        else launch_assemble<16>(s, state, save_base, amax_unset, in_flight, handoff_partials, nb, st);
    }
    return hipGetLastError();
}

}  // namespace dfa
