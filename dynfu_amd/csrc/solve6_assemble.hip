// solve6_assemble.hip — the normal equations of the north-star solve (formulation: solve6.hpp), one launch per
// Gauss-Newton iteration, one workgroup per node: the node's rows are staged in LDS, every lane walks its work unit's
// records (the plan of solve6_pattern.hip) and owns that unit's 8 x 8 moment; then H_ab = M_a S_ab M_b^T, the regulariser,
// the damping, the inverse of the diagonal block, the gradient and the start of the PCG.  One workgroup more does the
// energy's bookkeeping when the linearisation has not (gn_tol <= 0).
#include <hip/hip_runtime.h>

#include "solve6.hpp"
#include "solve6_internal.hpp"

namespace dfa {

namespace {

// column c of the inverse of a symmetric positive definite 6x6 (every caller lane factorises for itself: six lanes invert
// the block in the time of one column); zero if the factorisation fails: z = 0 for this node, as the oracle does
__device__ __forceinline__ void inv6_column(const float* M, float* out, int c, float (&x)[6]) {
    float L[6][6];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            float sm = M[6 * i + j];
#pragma unroll
            for (int q = 0; q < j; ++q) sm -= L[i][q] * L[j][q];
            if (i == j) {
                ok      = ok && sm > 0.f;
                L[i][i] = sqrtf(sm);
            } else {
                L[i][j] = sm / L[j][j];
            }
        }
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        float sm = i == c ? 1.f : 0.f;
#pragma unroll
        for (int q = 0; q < i; ++q) sm -= L[i][q] * y[q];
        y[i] = sm / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        float sm = y[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) sm -= L[q][i] * x[q];
        x[i] = sm / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = ok ? x[i] : 0.f, out[6 * i + c] = x[i];
}

// Values of block row a.  A data row's 6-vector for neighbour j factors as f_j * M_j l (l: 8 numbers per
// vertex, M_j: 6 x 8 per node, s6_node_now), so the block H_ab = sum_v rho f_a f_b (M_a l)(M_b l)^T is
// M_a S_ab M_b^T with the 8 x 8 moment S_ab = sum_v (rho f_a f_b) l l^T: the rows that touch node a are read
// as 8 + k floats instead of 6 k, S is accumulated, and M is applied once per block at the end.
// History at 4 k nodes, k = 8 (one Gauss-Newton iteration): one lane per row with LDS atomics 3.7 ms (64-way
// same-address conflicts); every (slot, c) thread scanning every row 2.2 ms (VALU-bound); per-wave private LDS copies
// of the moments, rows streamed 1.0 ms, with factored rows 0.81 ms (LDS-bandwidth-bound: 4 KiB read + written per row
// and wave; the "first form", in the tree until round 3); registers instead of LDS copies, a wave per slot, 0.65 ms (second
// form); symmetric blocks, a quad of lanes per work unit 0.315 ms (third form); a LANE per work unit — below.

typedef float v2f __attribute__((ext_vector_type(2)));

// Fourth form (round 3).  The third form (a quad of lanes owned a unit's 8 x 8 moment, 16 records per wave instruction) was
// bound by instruction ISSUE, not by memory or LDS: SQ counters at C3 gave 22 k vector instructions per workgroup of which
// 10 % were the products, the SIMDs' issue slots ~90 % taken, and neither removing exposed load waits nor an XCD-aware
// node order moved the time (tools/ns_assemble_phases.py).  Per 16 records a wave spent ~30 instructions
// on decoding the record, the validity selects, the addresses and eight DPP broadcasts, for eight packed FMAs.  Now:
//  (1) a LANE PER UNIT: every lane walks its own records (s6_pattern: S6_UNITS units per node, every n-th record of one
//      block's list) and owns that unit's whole moment — decode, addresses and LDS reads serve 64 records per wave
//      instruction instead of 16, and nothing is exchanged between lanes until the node is finished;
//  (2) SYMMETRY of the moment itself: S = sum c l l^T has 36 distinct entries, not 64 — 16 packed + 4 scalar FMAs per
//      record (and 4 packed multiplies for c l);
//  (3) slot 0 (every row's own neighbour) is a list like the others (its records are (row, own slot), its coefficient the
//      same rho f_a f_j): no separate loop, no per-pass cross-lane reduction; the gradient's 8 sums ride on its units;
//  (4) a lane's records come in batches of NG registers, loaded from clamped addresses before the staging barrier;
//  (5) rows staged by unconditional 16-byte loads from selected addresses (with a branch per kind of chunk the compiler
//      waited for every load before issuing the next: two loads of different width into one register).
// Kept from the third form: block (a, b) computed once, by the workgroup of the smaller index, written to both rows
// (H_ba = H_ab^T bit for bit); the coefficient rho f_a f_j of every (row, neighbour) formed once when the rows are staged;
// the regulariser's edges of the node staged in LDS; mirror blocks transposed through LDS; the PCG's start in the tail.
constexpr int S6_REGIN = 24;  // arriving regularisation edges staged in LDS (more: read from global memory)

// position of S[i][j] (= S[j][i]) in a unit's 36 accumulators: even rows i = 2t as pairs (j, j + 1) from j = i — 20
// numbers; odd rows i = 2t + 1 as pairs from j = i + 1 — 12 numbers; the odd rows' diagonal entries — 4 numbers
__host__ __device__ constexpr int s6_sym(int i, int j) {
    if (i > j) { const int t = i; i = j; j = t; }
    const int t = i >> 1;
    if ((i & 1) == 0) return 2 * ((t == 0 ? 0 : t == 1 ? 4 : t == 2 ? 7 : 9)) + (j - i);
    if (j == i) return 32 + t;
    return 20 + 2 * (t == 0 ? 0 : t == 1 ? 3 : 5) + (j - i - 1);
}

constexpr int S6_ASM_WAVES = 4;  // waves per SIMD the register allocation aims at (four workgroups per CU by LDS: <= 128 VGPRs, 3-4 spilled)
#ifdef DFA_S6_DEBUG  // development builds only (tools/ns_plan_check.py): the summed moments and M of 256 nodes from DFA_S6_DEBUG on
__device__ float s6_dbg[256 * (S6_MAXSLOT * 36 + 8)];
extern "C" __attribute__((visibility("default"))) int dfa_dev_s6_moments(float* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(s6_dbg), sizeof(float) * 256 * (S6_MAXSLOT * 36 + 8));
}
__device__ float s6_dbgm[256 * S6_MAXSLOT * 48];
extern "C" __attribute__((visibility("default"))) int dfa_dev_s6_m(float* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(s6_dbgm), sizeof(float) * 256 * S6_MAXSLOT * 48);
}
#endif
S6_TIMING_BUFFER(dfa_dev_s6_timing)
constexpr size_t s6_assemble_lds(int K, int RC) {  // dynamic segment: the staged rows, later the units' moments + the blocks' sums
    const size_t rows = (size_t)((RC * (2 + K / 4 + 1) + 255) / 256) * 4096, closing = (size_t)(S6_UNITS / 2 * 36 + S6_MAXSLOT * 36) * 4;
    return rows > closing ? rows : closing;
}
template <int K, int S6_RC, bool KEXACT>  // KEXACT: k == K (the common case: divisions by k are shifts)
__global__ __launch_bounds__(256, S6_ASM_WAVES) void s6_assemble2_kernel(Solve6View s, Solve6State* st, float wreg2, float damping,
                                                                         const S6Forcing forcing) {
    extern __shared__ __attribute__((aligned(16))) char s6_dyn[];
    // a staged row = the vertex's record as s6_linearise wrote it: l = (lW, lD) (32 bytes) | h_j = sqrt(rho) f_j, j < K |
    // sqrt(rho) r, -, -, - : RS bytes, in the order of the 16-byte chunks the row is fetched in (the LDS-DMA writes a wave's 64
    // chunks to 1 KiB in lane order).  Nothing is prepared per pass: rho f_a f_j = h_a h_j is formed where it is used.
    constexpr int RS = 32 + 4 * K + 16, CFO = 32, MTO = 32 + 4 * K;
    // after the passes the dynamic segment holds, in turn: the moments of half of the units [0, 18 KiB); the blocks' sums (36
    // floats per slot) behind them; M of the column nodes (48 floats per slot) and the transposition tile over the — by then
    // dead — units.  (All 256 units at once would be 36 KiB: the fourth workgroup of a CU would not fit.)
    float* upart     = reinterpret_cast<float*>(s6_dyn);                                                   // [S6_UNITS / 2][36]
    float(*accS)[36] = reinterpret_cast<float(*)[36]>(s6_dyn + sizeof(float) * 36 * (S6_UNITS / 2));
    float* smb       = reinterpret_cast<float*>(s6_dyn);
    __shared__ float g8w[4][8];           // -J^T r in l coordinates, per wave
    __shared__ float g8s[8];
    __shared__ float diag[36];
    __shared__ float gsh[6];              // -J^T W r of the node
    __shared__ float rout[8][24];         // edges leaving a: neighbour (bits), weight, residual (3), vectors (18)
    __shared__ float rin[S6_REGIN][24];   // edges arriving at a: source node (bits), weight, residual (3), vectors (18)
    __shared__ uint32_t bfirst[S6_MAXSLOT];  // first unit | units << 16 of every block that has units
    // (workgroup -> node in launch order.  Consecutive nodes on one XCD — node (b mod 8) D / 8 + b / 8 for workgroup b, so that
    // a vertex record is fetched into one L2 instead of up to k — measured 0.048 against 0.050 ms at C2 and 0.156 against
    // 0.150 at C3: not kept, profiles/r06_xcd_map.md.)
    const int a = blockIdx.x;
    const int tid = threadIdx.x, k = s.k;
    if (a == s.D) {  // one workgroup more than nodes: the energy of the linearisation this launch follows, the state block's bookkeeping
        if (forcing.decided) return;  // (the linearisation's last workgroup has done both)
        s6_cost_total(s, st);
        if (tid == 0) s6_bookkeeping(st, forcing);
        return;
    }
    if (forcing.decided && st->gn_stop) return;  // (uniform) the outer iteration has ended: no normal equations
    S6_TICK(tk0);
#ifdef DFA_S6_TIMING
    const unsigned long long wk0 = wall_clock64();
    unsigned long long tk_stage = 0, tk_prep = 0, tk_up = 0;
#endif

    const int cnt = s.bcnt[a], fu = s.bfu[a];
    const int beg = s.node_ptr[a], len = s.node_ptr[a + 1] - beg;
    const int wave = tid >> 6, lane = tid & 63;
    const int32_t* pptr = s.pair_ptr + (size_t)a * (s.cap + 1);
    const int rib = s.rnode_ptr[a], nri = s.rnode_ptr[a + 1] - rib;
    if (tid < S6_MAXSLOT) bfirst[tid] = 0u;
    // positions of the moment's entries the closing part's lane z reads: S[p][2 z + h] at symt[z][2 p + h]
    __shared__ __attribute__((aligned(16))) int symt[4][16];
    if (tid >= 128 && tid < 192) symt[(tid - 128) >> 4][tid & 15] = s6_sym((tid & 15) >> 1, 2 * ((tid - 128) >> 4) + (tid & 1));
    // the row's columns and the mirror slots: read by every phase of the closing part (two dependent global loads there)
    __shared__ int32_t scol[S6_MAXSLOT];
    __shared__ uint8_t srs[S6_MAXSLOT];
    __shared__ uint32_t rent[S6_REGIN];  // the arriving edges' (source node k + slot): one round trip less in the closing part
    // (everything the prologue needs from global memory is requested first, by unconditional loads from clamped indices, and
    // parked afterwards: a load under its own `if` followed by its LDS store made six dependent round trips of it)
    constexpr int EPT = (S6_RC + 255) / 256;
    const int col_i       = (int)((size_t)a * s.cap) + min(tid, s.cap - 1);
    const int32_t scol_v  = s.bcols[col_i];
    const uint8_t srs_v   = s.rslot[col_i];
    const uint32_t rent_v = s.rnode_list[rib + min(tid & 63, max(nri, 1) - 1)];  // (an empty list reads its neighbour's first entry: unused)
    uint32_t ent0[EPT];
#pragma unroll
    for (int q = 0; q < EPT; ++q) ent0[q] = s.node_list[beg + min(tid + 256 * q, max(len, 1) - 1)];
    // ---- this lane's work unit (s6_pattern: utab): every un-th record of block uq's list, from its phase on
    const int nup        = cnt > fu ? cnt - fu : 0;
    const uint32_t uinfo = s.utab[(size_t)a * S6_UNITS + tid];
    if (tid < S6_MAXSLOT) scol[tid] = tid < cnt ? scol_v : -1, srs[tid] = tid < cnt ? srs_v : (uint8_t)255;
    else if (tid >= 64 && tid < 64 + S6_REGIN) rent[tid - 64] = tid - 64 < nri ? rent_v : 0u;
    const int uq         = (int)(uinfo & 63u);
    const int un         = (int)((uinfo >> 16) & 1023u);
    const bool uhas      = uq < cnt && (uq == 0 || uq >= fu) && un > 0;
    const bool uown      = uhas && uq == 0;  // a unit of slot 0: it also sums the gradient
    int ucur = 0, uend = 0;                  // this lane's next record; end of the list
    {
        const int q0 = uhas ? uq : 0, b0 = pptr[q0], b1 = pptr[q0 + 1];
        if (uhas) ucur = b0 + (int)((uinfo >> 6) & 1023u), uend = b1;
    }
    v2f me[10], mo[6], G[4];  // even rows of the moment (pairs), odd rows beyond the diagonal (pairs); the gradient
    float md[4];              // the odd rows' diagonal entries
#pragma unroll
    for (int e = 0; e < 10; ++e) me[e] = v2f{0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 6; ++e) mo[e] = v2f{0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) G[e] = v2f{0.f, 0.f}, md[e] = 0.f;
    // a lane's records are fetched a BATCH of NG at a time into registers that are indexed statically: unconditional loads
    // from clamped addresses, all in flight together.  The first batch of a pass flies during the staging; a second one in a
    // pass is rare.  (One record ahead in a rotating register made the compiler wait for the load in the same trip.)
    constexpr int NG = 8;
    uint32_t rb[NG];
    auto load_batch = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int at = ucur + g * un;
            rb[g]        = s.pair_list[uhas && at < uend ? at : 0];
        }
    };
    constexpr int RS4 = 2 + K / 4 + 1, NCH = (S6_RC * RS4 + 255) / 256;  // 16-byte chunks of a record; chunks per thread and pass
    __shared__ uint32_t sent[2][S6_RC];  // (vertex k + slot) of the rows of this pass / the next one
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
        const int r = tid + 256 * q;
        if (r < min(S6_RC, len)) sent[0][r] = ent0[q];
    }
    int pass = 0;
    S6_TICK(tk1);
    for (int r0 = 0; r0 < len; r0 += S6_RC, pass ^= 1) {
        const int nr = min(S6_RC, len - r0);
        S6_TICK(tp0);
        __syncthreads();  // the pass before is done with the staged rows (and has stored this pass's list entries)
        const size_t e0 = (size_t)(beg + r0);
        // the next pass's list entries: loaded now, parked in LDS at the end of this pass (one register meanwhile)
        uint32_t nxt_ent[EPT];
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int r = tid + 256 * q;
            nxt_ent[q]  = r0 + S6_RC + r < len ? s.node_list[e0 + S6_RC + r] : 0u;
        }
        // The rows of the pass: one record per vertex (s6_linearise), gathered through the node's row list; RS4 chunks per row —
        // l (2 x 16 bytes), f (K / 4 x 16 bytes) from the vertex's 64-byte line, (weight, weight x residual, 0, 0) from the
        // per-vertex array — one chunk per lane and step, straight into LDS (global_load_lds_dwordx4: no staging registers, no
        // ds_write pass; rows past the end fetch row 0 again, into rows nobody reads).
        // (the chunk's row and part are recomputed in every pass: hoisted out of the pass loop, as the compiler would have it,
        // they are 2 x NCH registers that live — spilled — through the whole kernel.  The list entries are all read before the
        // first DMA is issued: the compiler orders a ds_read behind an LDS-DMA in flight with s_waitcnt vmcnt(0), one memory
        // round trip per chunk.)
        unsigned tl = (unsigned)tid;
        asm volatile("" : "+v"(tl));
        uint32_t ens[NCH];
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            const unsigned r = (tl + 256u * q) / (unsigned)RS4;
            ens[q]           = sent[pass][min(r, (unsigned)nr - 1u)];
        }
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            const unsigned i = tl + 256u * q, r = i / (unsigned)RS4, c = i - (unsigned)RS4 * r;
            const size_t v = KEXACT ? ens[q] / (unsigned)K : ens[q] / (unsigned)k;  // (K: a shift)
            const float4* src = reinterpret_cast<const float4*>(s.rec + (12 + K) * v) + c;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(s6_dyn + 16 * (256 * q + 64 * wave)), 16, 0, 0);
        }
        // this lane's next NG records fly while the rows settle
        load_batch();
        __syncthreads();
        S6_TICK(tp1);
        S6_TICK(tp2);
        // ---- the records of this pass: a lane takes its unit's records while their rows are staged (the lists ascend)
        {
            bool act       = uhas && ucur < uend;
            const bool gw  = __any(uown);  // (this wave has units of slot 0)
            auto walk_batch = [&]() __attribute__((always_inline)) {
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (!__any(act)) break;
                    // (an active lane is at the g-th record of its batch: it advanced in every trip so far)
                    const uint32_t pr = rb[g];  // row of the node's list << 8 | the row's own slot << 4 | neighbour slot
                    const unsigned rr = (pr >> 8) - (unsigned)r0;
                    const bool in     = act && rr < (unsigned)nr;
                    const unsigned ri = in ? rr : 0u;
                    const char* rp  = s6_dyn + RS * ri;
                    const float4 la = reinterpret_cast<const float4*>(rp)[0], lb = reinterpret_cast<const float4*>(rp)[1];
                    const float ho  = *reinterpret_cast<const float*>(rp + CFO + ((pr >> 2) & 60u));  // h_a: sqrt(rho) f_a
                    const float hj  = *reinterpret_cast<const float*>(rp + CFO + ((pr << 2) & 60u));  // h_j
                    const float cf  = in ? ho * hj : 0.f;                                             // rho f_a f_j
                    const v2f L[4]  = {v2f{la.x, la.y}, v2f{la.z, la.w}, v2f{lb.x, lb.y}, v2f{lb.z, lb.w}};
                    const v2f cc    = v2f{cf, cf};
                    v2f F[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) F[t] = cc * L[t];
                    constexpr int eo[4] = {0, 4, 7, 9}, oo[4] = {0, 3, 5, 6};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const v2f fe = v2f{F[t].x, F[t].x}, fo = v2f{F[t].y, F[t].y};
#pragma unroll
                        for (int q = 0; q < 4 - t; ++q) me[eo[t] + q] = __builtin_elementwise_fma(fe, L[t + q], me[eo[t] + q]);
                        md[t] = fmaf(F[t].y, L[t].y, md[t]);
#pragma unroll
                        for (int q = 0; q < 3 - t; ++q) mo[oo[t] + q] = __builtin_elementwise_fma(fo, L[t + 1 + q], mo[oo[t] + q]);
                    }
                    if (gw) {  // -J^T r: the slot-0 units' rows, each once
                        const float gr = uown && in ? -*reinterpret_cast<const float*>(rp + MTO) * ho : 0.f;  // -(sqrt(rho) r) h_a
                        const v2f gg   = v2f{gr, gr};
#pragma unroll
                        for (int t = 0; t < 4; ++t) G[t] = __builtin_elementwise_fma(gg, L[t], G[t]);
                    }
                    if (in) ucur += un;
                    act = in && ucur < uend;
                }
            };
            // (the first batch was loaded before the staging barrier; a refill — rare — is a path of its own: with the refill
            // at the bottom of ONE loop the batch registers were loop-carried loads and the common path waited for them in every
            // trip — C3 0.143 -> 0.120 ms.  Pulling the next pass's records towards L2 meanwhile, by 4-byte LDS-DMA loads into a
            // scrap area issued from an asm statement, made it 0.135: not kept.)
            walk_batch();
            while (__any(act)) {
                load_batch();  // (more than NG records of a unit in one pass)
                walk_batch();
            }
        }
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int r = tid + 256 * q;
            if (r < S6_RC) sent[pass ^ 1][r] = nxt_ent[q];
        }
#ifdef DFA_S6_TIMING
        {
            S6_TICK(tp4);
            tk_stage += tp1 - tp0, tk_prep += tp2 - tp1, tk_up += tp4 - tp2;
        }
#endif
    }
    S6_TICK(tk2);
    // ---- the units' moments: lanes 2 i and 2 i + 1 (the same block, s6_pattern) are added by DPP, the even lanes park the
    // pair's moment in LDS (128 x 36 floats, in the rows' area), then every block is the sum of its pairs in unit order
    __syncthreads();  // the passes are over: the rows' area is free (and bfirst is cleared, scol / rent are written)
    S6_TICK(tk2a);
    if (uhas && ((uinfo >> 6) & 1023u) == 0u) bfirst[uq] = (uint32_t)(tid >> 1) | ((uint32_t)(un >> 1) << 16);
    {   // the gradient: summed over the wave (only the slot-0 units hold anything)
        float gv[8];
#pragma unroll
        for (int t = 0; t < 4; ++t) gv[2 * t] = G[t].x, gv[2 * t + 1] = G[t].y;
        if (__any(uown)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) gv[e] = wave_sum_all(gv[e]);
        }
        if (lane < 8) {
            float x = gv[0];
#pragma unroll
            for (int e = 1; e < 8; ++e) x = lane == e ? gv[e] : x;
            g8w[wave][lane] = x;
        }
    }
    {
        auto pair = [](float x) __attribute__((always_inline)) {  // x + the other lane of the pair's (quad_perm [1, 0, 3, 2])
            return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));
        };
        float w[36];
#pragma unroll
        for (int e = 0; e < 10; ++e) w[2 * e] = pair(me[e].x), w[2 * e + 1] = pair(me[e].y);
#pragma unroll
        for (int e = 0; e < 6; ++e) w[20 + 2 * e] = pair(mo[e].x), w[21 + 2 * e] = pair(mo[e].y);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[32 + e] = pair(md[e]);
        if ((tid & 1) == 0) {
            float4* d0 = reinterpret_cast<float4*>(upart + 36 * (tid >> 1));
#pragma unroll
            for (int e = 0; e < 9; ++e) d0[e] = make_float4(w[4 * e], w[4 * e + 1], w[4 * e + 2], w[4 * e + 3]);
        }
    }
    // ---- what the epilogue needs from global memory is requested now (the moments' registers are free), into registers — the
    // node's regularisation edges (leaving: 1 value per thread, arriving: up to 3) and M of the row's column nodes (48 floats
    // per slot) — and parked in LDS once the moments are summed: the round trip passes under the sums and their barriers
    constexpr int RINQ = (S6_REGIN * 24 + 255) / 256, MQ = (S6_MAXSLOT * 48 + 255) / 256;
    // (one unconditional 4-byte load from a selected address per value: a branch per field makes them wait for each other)
    auto edge_field = [&](int f, size_t e) __attribute__((always_inline)) {  // field f of edge e: 0 neighbour, 1 weight, 2-4 residual, 5-22 vectors
        const float* p = reinterpret_cast<const float*>(s.reg_idx + e);
        p = f == 1 ? s.rhub + e : p;
        p = f >= 2 && f < 5 ? s.rres + 3 * e + (f - 2) : p;
        p = f >= 5 && f < 23 ? s.rvec + 18 * e + (f - 5) : p;
        return *p;
    };
    float rov, riv[RINQ], mreg[MQ];
    {
        const int q = tid < k * 24 ? tid / 24 : 0, f = tid - 24 * (tid / 24);
        rov = edge_field(f, (size_t)(a * k + q));
    }
#pragma unroll
    for (int t = 0; t < RINQ; ++t) {
        const int i = tid + 256 * t, q = i / 24, f = i - 24 * q;
        riv[t]      = edge_field(f, (size_t)rent[i < min(nri, S6_REGIN) * 24 ? q : 0]);
    }
#pragma unroll
    for (int t = 0; t < MQ; ++t) {
        const int i = tid + 256 * t, slot = i / 48;
        mreg[t]     = i < cnt * 48 ? s.mnode[48 * (size_t)scol[slot] + (i - 48 * slot)] : 0.f;
    }
    S6_TICK(tk2b);
    __syncthreads();
    S6_TICK(tk2c);
    for (int i = tid; i < (1 + nup) * 36; i += 256) {
        const int bi = i / 36, e = i - 36 * bi, slot = bi == 0 ? 0 : fu + bi - 1;
        const uint32_t bf = bfirst[slot];
        const int u0 = (int)(bf & 0xffffu), n = (int)(bf >> 16);
        float sum = 0.f;
        for (int u = 0; u < n; ++u) sum += upart[36 * (u0 + u) + e];
        accS[slot][e] = sum;
    }
    if (tid < 8) g8s[tid] = (g8w[0][tid] + g8w[1][tid]) + (g8w[2][tid] + g8w[3][tid]);
    __syncthreads();
#ifdef DFA_S6_DEBUG
    if (a >= DFA_S6_DEBUG && a < DFA_S6_DEBUG + 256) {
        const int da = a - DFA_S6_DEBUG;
        for (int i = tid; i < S6_MAXSLOT * 36; i += 256) s6_dbg[(size_t)da * (S6_MAXSLOT * 36 + 8) + i] = (&accS[0][0])[i];
        if (tid < 8) s6_dbg[(size_t)da * (S6_MAXSLOT * 36 + 8) + S6_MAXSLOT * 36 + tid] = g8s[tid];
    }
#endif
    S6_TICK(tk3);
    // H_ab = M_a S_ab M_b^T, regularisation, output: thread (slot, row) finishes row `row` of the block in `slot` — of slot 0
    // and of the upper slots; an upper block also goes, transposed, to the row of its column.
    // M of the row's column nodes (48 floats per slot) and the edges: from the registers they arrived in
#pragma unroll
    for (int t = 0; t < MQ; ++t) {
        const int i = tid + 256 * t;
        if (i < cnt * 48) smb[i] = mreg[t];
    }
    if (tid < k * 24) {
        const int f = tid - 24 * (tid / 24);
        (&rout[0][0])[tid] = f == 1 ? wreg2 * rov : f == 23 ? 0.f : rov;
    }
#pragma unroll
    for (int t = 0; t < RINQ; ++t) {
        const int i = tid + 256 * t, q = i / 24, f = i - 24 * q;
        if (i < min(nri, S6_REGIN) * 24)
            (&rin[0][0])[i] = f == 0 ? __int_as_float((int)(rent[q] / (unsigned)k)) : f == 1 ? wreg2 * riv[t] : f == 23 ? 0.f : riv[t];
    }
    __syncthreads();
#ifdef DFA_S6_DEBUG
    if (a >= DFA_S6_DEBUG && a < DFA_S6_DEBUG + 256)
        for (int i = tid; i < cnt * 48; i += 256) s6_dbgm[(size_t)(a - DFA_S6_DEBUG) * S6_MAXSLOT * 48 + i] = smb[i];
#endif
    S6_TICK(tk4);
    // A QUAD of lanes per (block, row), ten blocks (240 threads) per round: lane z takes columns 2 z, 2 z + 1 of M_a S and every
    // fourth regularisation edge, the four partial rows are added by DPP.  (One thread per (block, row) — 102 of the 256 at C3 —
    // walked 112 FMAs, ~90 LDS reads and both edge loops alone: 7 of the workgroup's 42 us.)
    const int nfin = 1 + nup;
    constexpr int BPR = 10;
    float* ttile = reinterpret_cast<float*>(s6_dyn) + S6_MAXSLOT * 48;  // BPR x 36 floats behind M (the units' moments are dead)
    auto quad_sum = [](float x) __attribute__((always_inline)) {
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));  // quad_perm [1, 0, 3, 2]
        x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true));  // quad_perm [2, 3, 0, 1]
        return x;
    };
    for (int b0 = 0; b0 < nfin; b0 += BPR) {
        const int quad = tid >> 2, z = tid & 3, lb = quad / 6, my_row = quad - 6 * lb, sidx = b0 + lb;
        const bool on  = tid < 4 * 6 * BPR && sidx < nfin;
        const int slot = on ? (sidx == 0 ? 0 : fu + sidx - 1) : 0;
        const int col  = scol[slot];
        float accr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gacc = 0.f;
        if (on) {
            // columns 2 z, 2 z + 1 of row my_row of M_a S (slot 0 of M is node a itself), then their share of (M_a S) M_b^T
            const int4* st4 = reinterpret_cast<const int4*>(&symt[z][0]);
            int sy[16];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int4 v = st4[e];
                sy[4 * e] = v.x, sy[4 * e + 1] = v.y, sy[4 * e + 2] = v.z, sy[4 * e + 3] = v.w;
            }
            const float* S0 = &accS[slot][0];
            float v0 = 0.f, v1 = 0.f;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const float ma = smb[8 * my_row + p];
                v0 = fmaf(ma, S0[sy[2 * p]], v0), v1 = fmaf(ma, S0[sy[2 * p + 1]], v1);
            }
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                const float2 mb = *reinterpret_cast<const float2*>(smb + 48 * slot + 8 * d + 2 * z);
                accr[d]         = fmaf(v1, mb.y, v0 * mb.x);
            }
            if (slot == 0) {
                const float2 mo2 = *reinterpret_cast<const float2*>(smb + 8 * my_row + 2 * z);
                gacc             = fmaf(mo2.y, g8s[2 * z + 1], mo2.x * g8s[2 * z]);
            }
            // regularisation edges leaving a (a -> m): rows c of e = T_a g_m - g^_m with vectors (an_c at a, -e_{3+c} at m)
            for (int q = z; q < k; q += 4) {
                const float* E = rout[q];
                const int m    = __float_as_int(E[0]);
                if (m < 0 || (slot != 0 && col != m)) continue;
                const float wt = E[1];
                for (int cc = 0; cc < 3; ++cc) {
                    const float* an = E + 5 + 6 * cc;
                    if (slot == 0) {
                        gacc -= wt * an[my_row] * E[2 + cc];
#pragma unroll
                        for (int d = 0; d < 6; ++d) accr[d] += wt * an[my_row] * an[d];
                    } else {
                        accr[3 + cc] -= wt * an[my_row];
                    }
                }
            }
            // regularisation edges arriving at a (n -> a)
            if (my_row >= 3) {
                const int cc = my_row - 3;
                for (int e = z; e < nri; e += 4) {
                    const bool staged    = e < S6_REGIN;  // (rarely not: more arriving edges than the staged ones)
                    const float* E       = rin[staged ? e : 0];
                    const unsigned entry = staged ? 0u : s.rnode_list[rib + e];
                    const int n          = staged ? __float_as_int(E[0]) : (int)(entry / (unsigned)k);
                    if (slot != 0 && col != n) continue;
                    const float wt = staged ? E[1] : wreg2 * s.rhub[entry];
                    if (slot == 0) {
                        gacc += wt * (staged ? E[2 + cc] : s.rres[3 * (size_t)entry + cc]);
                        accr[my_row] += wt;
                    } else {
#pragma unroll
                        for (int d = 0; d < 6; ++d)
                            accr[d] -= wt * (staged ? E[5 + 6 * cc + d] : s.rvec[18 * (size_t)entry + 6 * cc + d]);
                    }
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 6; ++d) accr[d] = quad_sum(accr[d]);
        gacc = quad_sum(gacc);
        if (on && z == 0) {
            if (slot == 0) {
                accr[my_row] += damping;
                s.g[6 * (size_t)a + my_row] = gacc, gsh[my_row] = gacc;
#pragma unroll
                for (int d = 0; d < 6; ++d) diag[my_row * 6 + d] = accr[d];
            }
            float2* out = reinterpret_cast<float2*>(s.bvals + ((size_t)a * s.cap + slot) * 36 + 6 * my_row);
            out[0] = make_float2(accr[0], accr[1]), out[1] = make_float2(accr[2], accr[3]), out[2] = make_float2(accr[4], accr[5]);
            // the mirror block H_ba = H_ab^T goes out row by row too (24 contiguous bytes per thread, the block's 144 from six
            // threads): transposed through LDS — written element by element it cost 4 bytes per store into somebody else's
            // cache lines (PMC: 135 MB written per launch at C3 for a 21 MB matrix)
            float* tile = ttile + 36 * lb + my_row;  // column my_row of the block's transpose
#pragma unroll
            for (int d = 0; d < 6; ++d) tile[6 * d] = accr[d];
        }
        __syncthreads();
        if (on && z == 0 && slot != 0) {
            const int rs = srs[slot];
            if (rs != 255) {
                const float* tr = ttile + 36 * lb + 6 * my_row;  // row my_row of the transposed block
                float2* out2    = reinterpret_cast<float2*>(s.bvals + ((size_t)col * s.cap + rs) * 36 + 6 * my_row);
                out2[0] = make_float2(tr[0], tr[1]), out2[1] = make_float2(tr[2], tr[3]), out2[2] = make_float2(tr[4], tr[5]);
            }
        }
        if (b0 + BPR < nfin) __syncthreads();  // (the tile is reused by the next round)
    }
    S6_TICK(tk5);
    if (tid < 6) {
        // column tid of M^-1 (= its row tid: symmetric), and with it the start of the PCG for this node:
        // x = 0, r = g, u = M^-1 g, p = s = t = 0
        float col[6];
        inv6_column(diag, s.minv + 36 * (size_t)a, tid, col);
        float u = 0.f;
#pragma unroll
        for (int d = 0; d < 6; ++d) u += col[d] * gsh[d];
        const size_t i = 6 * (size_t)a + tid;
        s.x[i] = 0.f, s.r[i] = gsh[tid], s.u[0][i] = u;
        s.p[i] = 0.f, s.s[i] = 0.f, s.t[0][i] = 0.f, s.t[1][i] = 0.f;
    }
#ifdef DFA_S6_TIMING
    if (tid == 0 && a < 16384) {
        unsigned long long* o = s6_tbuf + 16 * (size_t)a;
        const unsigned long long tk6 = clock64();
        o[0] = tk0, o[1] = tk1 - tk0, o[2] = tk_stage, o[3] = tk_prep, o[4] = tk2a - tk2, o[5] = tk_up, o[6] = tk3 - tk2, o[7] = tk4 - tk3,
        o[8] = tk5 - tk4, o[9] = tk6 - tk5, o[10] = tk6 - tk0, o[11] = wall_clock64() - wk0, o[12] = (unsigned long long)len,
        o[13] = (unsigned long long)cnt, o[14] = wk0, o[15] = ((tk2b - tk2a) << 32) | (tk2c - tk2b);
    }
#endif
}

}  // namespace

hipError_t s6_assemble(const Solve6View& s, Solve6State* state, const Solve6Params& p, int gn_in_outer, hipStream_t st) {
    const float wreg2 = p.lambda / ((float)s.D * (float)s.k);
    const S6Forcing f = s6_forcing(p, gn_in_outer);
    {
        // rows staged per pass: what fits in 28 KiB — with the static arrays 36 KiB, four workgroups per CU
#define S6A2(KK, RC)                                                                                              \
    do {                                                                                                          \
        if (s.k == (KK)) S6A2X(KK, RC, true);                                                                     \
        else S6A2X(KK, RC, false);                                                                                \
    } while (0)
#define S6A2X(KK, RC, EX)                                                                                         \
    do {                                                                                                          \
        constexpr size_t sh = s6_assemble_lds(KK, RC);                                                            \
        if (sh > 48 * 1024) {                                                                                     \
            const hipError_t ae = allow_dynamic_lds((const void*)s6_assemble2_kernel<KK, RC, EX>, (int)sh);         \
            if (ae != hipSuccess) return ae;                                                                      \
        }                                                                                                         \
        s6_assemble2_kernel<KK, RC, EX><<<s.D + 1, 256, sh, st>>>(s, state, wreg2, p.damping, f);                         \
    } while (0)
        if (s.k <= 4) S6A2(4, 448);
        else S6A2(8, 352);
#undef S6A2
#undef S6A2X
    }
    return hipGetLastError();
}

}  // namespace dfa
