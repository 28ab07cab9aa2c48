// solve6_pattern.hip — once per frame of the north-star solve, after the graphs (solve6_graph.hip): the block-row
// pattern of the normal matrix (columns ascending behind the diagonal), per node the (row, neighbour) pair lists by slot
// and the work units of its assembly workgroup (solve6_assemble.hip walks them), and the mirror slots of the symmetric
// blocks.
#include <hip/hip_runtime.h>

#include "solve6.hpp"
#include "solve6_internal.hpp"

namespace dfa {

namespace {

constexpr int S6_HASH = 128;

__device__ __forceinline__ int hash_slot(int* keys, int b) {
    unsigned h = ((unsigned)b * 2654435761u) >> 25;  // 7 bits
    for (int probe = 0; probe < S6_HASH; ++probe) {
        // (a plain read first: thousands of pairs look up a few dozen keys, and an LDS atomic per look-up on a handful of
        // addresses serialises the wave; an entry, once written, never changes)
        int seen = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
        if (seen == -1) seen = atomicCAS(&keys[h], -1, b);
        if (seen == -1 || seen == b) return (int)h;
        h = (h + 1) & (S6_HASH - 1);
    }
    return -1;
}

constexpr int S6_DEAL  = 8;             // a node's sorted rows are dealt out in this many interleaved runs (s6_pattern_kernel)
S6_TIMING_BUFFER(dfa_dev_s6_pattern_timing)

// Sparsity pattern of block row a (fixed by the graphs of the frame, built once per set_problem):
// the diagonal first, then every node that shares a vertex with a or is joined to it by a
// regularisation edge, ascending.
__global__ __launch_bounds__(256) void s6_pattern_kernel(Solve6View s, Solve6State* st) {
    __shared__ int keys[S6_HASH];
    __shared__ int cnt_sh;
    __shared__ uint32_t sortbuf[S6_SORT_MAX];
    const int a = blockIdx.x, tid = threadIdx.x, k = s.k;
    S6_TICK(pk0);
    for (int i = tid; i < S6_HASH; i += 256) keys[i] = -1;
    if (tid == 0) cnt_sh = 0;
    // The transposition fills a node's list in whatever order its workgroups' atomics land; sort it so
    // that the assembly adds the rows in ascending (vertex, slot) order: run-to-run reproducible sums.
    {
        const int beg = s.node_ptr[a], len = s.node_ptr[a + 1] - beg;
        if (len > 1 && len <= S6_SORT_MAX) {
            int n2 = 1;
            while (n2 < len) n2 <<= 1;
            for (int i = tid; i < n2; i += 256) sortbuf[i] = i < len ? s.node_list[beg + i] : 0xffffffffu;
            __syncthreads();
            s6_sort_lds(sortbuf, n2, tid);
            // ... and deal the sorted rows out in S6_DEAL interleaved runs (rows 0, 8, 16, ..., then 1, 9, ...): the assembly
            // stages the list a few hundred rows at a time, and a vertex's neighbours come in clusters along the sorted list —
            // in sorted order one pass held all the records of some blocks and none of others, and the lanes (one block each)
            // waited for the fullest (3.5 us of a workgroup's 42 at C3).  Now every pass is a uniform sample.
            const int per = len / S6_DEAL, extra = len - per * S6_DEAL;
            for (int i = tid; i < len; i += 256) {
                const int g = i % S6_DEAL, t = i / S6_DEAL;
                s.node_list[beg + g * per + min(g, extra) + t] = sortbuf[i];
            }
        }
        if (tid == 0) {  // the few regularisation edges arriving at a: insertion sort
            const int rb = s.rnode_ptr[a], re = s.rnode_ptr[a + 1];
            for (int i = rb + 1; i < re; ++i) {
                const uint32_t x = s.rnode_list[i];
                int j = i - 1;
                for (; j >= rb && s.rnode_list[j] > x; --j) s.rnode_list[j + 1] = s.rnode_list[j];
                s.rnode_list[j + 1] = x;
            }
        }
    }
    __syncthreads();
    S6_TICK(pk1);
    // ---- the columns of block row a: every neighbour of every vertex of a's rows (and the regularisation partners) into a
    // 128-entry LDS hash; the position a pair's neighbour landed at is remembered per pair (a byte: 254 = a itself, 255 =
    // none), so that the pair's slot is a table look-up once the columns are ranked.  The bytes live in the (now idle) sort
    // buffer when they fit, else in global scratch.
    const int pbeg = s.node_ptr[a], plen = s.node_ptr[a + 1] - pbeg, npairs = plen * k;
    uint8_t* es_lds   = reinterpret_cast<uint8_t*>(sortbuf);
    const bool in_lds = npairs <= (int)sizeof(sortbuf);
    uint8_t* es       = in_lds ? es_lds : s.eslot + (size_t)pbeg * k;
    bool lost = false;
    // (four rows of a thread at a time: their list entries requested together, then their neighbour ids — row by row the two
    // dependent loads of every row were a chain of 2 x rows / 256 round trips)
    for (int r0 = tid; r0 < plen; r0 += 4 * 256) {
        unsigned v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = s.node_list[pbeg + min(r0 + 256 * i, plen - 1)] / (unsigned)k;
        int nb[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) nb[i][j] = j < k ? s.idx[(size_t)v[i] * k + j] : -1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + 256 * i;
            if (r >= plen) break;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (j >= k) break;
                const int b = nb[i][j];
                int hp      = 255;
                if (b == a) hp = 254;
                else if (b >= 0) {
                    hp = hash_slot(keys, b);
                    if (hp < 0) lost = true, hp = 255;
                }
                es[(size_t)r * k + j] = (uint8_t)hp;
            }
        }
    }
    if (tid < k) {
        const int m = s.reg_idx[a * k + tid];
        if (m >= 0 && m != a && hash_slot(keys, m) < 0) lost = true;
    }
    for (int e = s.rnode_ptr[a] + tid; e < s.rnode_ptr[a + 1]; e += 256) {
        const int n = (int)(s.rnode_list[e] / (unsigned)k);
        if (n != a && hash_slot(keys, n) < 0) lost = true;
    }
    __syncthreads();
    S6_TICK(pk2);
    __shared__ uint8_t hrank[S6_HASH];  // hash position -> slot of that column (255: not stored)
    if (tid < S6_HASH) {
        int r = 254;
        if (keys[tid] >= 0) {
            r = 0;
            for (int h = 0; h < S6_HASH; ++h) r += keys[h] >= 0 && keys[h] < keys[tid];
            if (r + 1 < s.cap) s.bcols[(size_t)a * s.cap + r + 1] = keys[tid];
            atomicAdd(&cnt_sh, 1);
        }
        hrank[tid] = (uint8_t)(r + 1 < s.cap ? r + 1 : 255);
    }
    __syncthreads();
    const int nblk = cnt_sh + 1, stored = nblk < s.cap ? nblk : s.cap;
    for (int i = stored + tid; i < s.cap; i += 256) s.bcols[(size_t)a * s.cap + i] = -1;  // the matvec reads no count
    if (tid == 0) {
        s.bcols[(size_t)a * s.cap] = a;
        s.bcnt[a] = stored;
        // (a running maximum: most workgroups find it already at or above theirs and skip the same-address atomic)
        if (nblk > __atomic_load_n(&st->max_row_blocks, __ATOMIC_RELAXED)) atomicMax(&st->max_row_blocks, nblk);
        if (nblk > s.cap || plen > 60000) st->overflow = 1;  // (16-bit offsets in the split below)
    }
    if (lost) st->overflow = 1;
    // The matrix is symmetric, H_ba = H_ab^T: the assembly computes a block once, in the row of the smaller node index, and
    // writes it to both rows.  Pair lists are kept for slot 0 (the row's own neighbour: one record per row) and for the "upper"
    // slots (column > a; the columns ascend, so these are the slots from `fu` on), the others stay empty.
    __shared__ int pcnt[64], pstart[64];
    __shared__ int fu_sh;
    if (tid < S6_HASH / 2) {  // first wave: slots 1 .. fu - 1 are the columns below a = the keys below a
        const uint64_t l0 = __ballot(keys[tid] >= 0 && keys[tid] < a), l1 = __ballot(keys[tid + 64] >= 0 && keys[tid + 64] < a);
        if (tid == 0) {
            const int f = min(1 + __popcll(l0) + __popcll(l1), stored);
            fu_sh = f, s.bfu[a] = f;
        }
    }
    __syncthreads();
    S6_TICK(pk3);
    const int fu = fu_sh;
    // ---- the pattern by slot (s6_assemble2_kernel): a STABLE split of the (row, neighbour) pairs by slot, as a counting sort —
    // thread t takes a contiguous run of pairs, counts its pairs per slot into its own column of hist (16-bit), the columns
    // are scanned per slot (wave w: slots w, w + 4, ...), then every thread writes its pairs, in order, from its offsets on:
    // lists in ascending pair order, run-to-run identical, O(pairs) work (ballots per slot and 64 pairs: 83 of the kernel's
    // 194 us per workgroup at C3).
    // (S6_SPLIT listed slots — slot 0 and the upper ones, in slot order — per round: all 48 at once are 24 KiB of counters, which
    // left room for three workgroups per CU instead of five)
    // (Round 4, tools/ns_pattern_phases.py with finer marks at C3: of the split's 29 us a thread spends 6 translating its bytes,
    // 4 clearing + counting, 3 in the scan and 16 WRITING — 8 300 four-byte stores per workgroup, each lane of a wave to
    // another list: the store transactions, not LDS, are what it waits for.  Giving every thread whole rows with its bytes in
    // a run padded to an odd number of words — no bank shared by the lanes of a pass, where 32-40-byte runs share four —
    // changed nothing: 29.0 us either way.)
    constexpr int S6_SPLIT = 24;
    __shared__ uint16_t hist[S6_SPLIT][256];
    __shared__ int run_sh;
    const int nlisted = stored > fu ? 1 + stored - fu : 1;  // listed slot li: slot 0 (li = 0) or slot fu + li - 1
    const int per_thread = (npairs + 255) / 256, p0 = min(tid * per_thread, npairs), p1 = min(p0 + per_thread, npairs);
    for (int p = p0; p < p1; ++p) {  // hash position -> listed slot index (255: none)
        const int hp = es[p];
        const int sl = hp == 254 ? 0 : hp == 255 ? 255 : (int)hrank[hp];
        es[p] = (uint8_t)(sl == 0 ? 0 : (sl >= fu && sl < stored) ? sl - fu + 1 : 255);
    }
    if (tid < 64) pcnt[tid] = 0;
    if (tid == 0) run_sh = pbeg * k;  // the lists of node a live in pair_list[pbeg k, (pbeg + plen) k): slot 0 (every row), then the upper slots
    for (int l0 = 0; l0 < nlisted; l0 += S6_SPLIT) {
        const int nl = min(S6_SPLIT, nlisted - l0);
        for (int i = tid; i < S6_SPLIT * 256 / 8; i += 256) reinterpret_cast<uint4*>(&hist[0][0])[i] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        for (int p = p0; p < p1; ++p) {
            const int li = (int)es[p] - l0;
            if (li >= 0 && li < nl) hist[li][tid] += 1;
        }
        __syncthreads();
        {
            const int wave = tid >> 6, lane = tid & 63;
            for (int li = wave; li < nl; li += 4) {
                uint2* hq      = reinterpret_cast<uint2*>(&hist[li][4 * lane]);  // threads 4 lane .. 4 lane + 3
                const uint2 hv = *hq;
                const uint32_t c0 = hv.x & 0xffffu, c1 = hv.x >> 16, c2 = hv.y & 0xffffu, c3 = hv.y >> 16;
                const uint32_t mine = c0 + c1 + c2 + c3;
                uint32_t incl = mine;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t t = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += t;
                }
                const uint32_t e0 = incl - mine, e1 = e0 + c0, e2 = e1 + c1, e3 = e2 + c2;
                *hq = make_uint2(e0 | (e1 << 16), e2 | (e3 << 16));
                if (lane == 63) pcnt[l0 + li == 0 ? 0 : fu + l0 + li - 1] = (int)incl;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int run = run_sh;
            for (int li = l0; li < l0 + nl; ++li) {
                const int q = li == 0 ? 0 : fu + li - 1;
                if (li == 1)
                    for (int z = 1; z < fu; ++z) pstart[z] = run;  // (the lower slots: empty lists)
                pstart[q] = run, run += pcnt[q];
            }
            run_sh = run;
            if (l0 + nl >= nlisted) {
                if (nlisted == 1)
                    for (int z = 1; z < stored; ++z) pstart[z] = run;
                pstart[stored] = run;
            }
        }
        __syncthreads();
        // the pairs of this thread, in order, each to the next free place of its slot's list
        for (int p = p0; p < p1; ++p) {
            const int li = (int)es[p] - l0;
            if (li < 0 || li >= nl) continue;
            const int r = p / k, q = l0 + li == 0 ? 0 : fu + l0 + li - 1;
            const uint32_t oj  = s.node_list[pbeg + r] % (unsigned)k;  // the row's own neighbour slot
            const uint32_t off = hist[li][tid];
            hist[li][tid]      = (uint16_t)(off + 1u);
            s.pair_list[pstart[q] + (int)off] = ((uint32_t)r << 8) | (oj << 4) | (uint32_t)(p - r * k);
        }
        if (l0 + S6_SPLIT < nlisted) __syncthreads();  // (the counters are cleared for the next round)
    }
    S6_TICK(pk4);
    __syncthreads();
    if (tid <= stored) s.pair_ptr[(size_t)a * (s.cap + 1) + tid] = pstart[tid];
    // ---- work units of the assembly: S6_UNITS per node, one per LANE of its workgroup.  A unit walks every n-th record of ONE
    // block's list (slot 0 — every row — or an upper slot), starting at its `phase`; a block with c of the node's T records
    // gets 2 (1 + floor((S6_UNITS / 2 - blocks) c / T)) units, so every unit of the workgroup walks about T / S6_UNITS records,
    // the units of a block are neighbours (neighbouring lanes read neighbouring rows) and lanes 2 i, 2 i + 1 always work
    // for the same block.
    __shared__ int ustart[64], ucount[64];
    if (tid < 64) {
        const int q    = tid == 0 ? 0 : fu + tid - 1;  // lane = block: slot 0, then the upper slots
        const int mine = (tid == 0 || q < stored) ? pcnt[tid == 0 ? 0 : q] : 0;
        const int nblk2 = __popcll(__ballot(mine > 0));
        int total = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
        const int n = mine > 0 ? 2 * (1 + (int)(((long long)(S6_UNITS / 2 - nblk2) * mine) / total)) : 0;  // (even: see the assembly's closing part)
        int incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (tid >= o) incl += t;
        }
        ustart[tid] = incl - n, ucount[tid] = n;
    }
    __syncthreads();
    {
        uint32_t info = 63u;  // idle
        for (int i = 0; i < 64; ++i) {
            const int u0 = ustart[i], n = ucount[i];
            if (tid >= u0 && tid < u0 + n) info = (uint32_t)(i == 0 ? 0 : fu + i - 1) | ((uint32_t)(tid - u0) << 6) | ((uint32_t)n << 16);
        }
        s.utab[(size_t)a * S6_UNITS + tid] = info;
    }
    S6_TICK(pk5);
#ifdef DFA_S6_TIMING
    if (tid == 0 && a < 16384) {
        unsigned long long* o = s6_tbuf + 16 * (size_t)a;
        const unsigned long long pk6 = clock64();
        o[0] = pk0, o[1] = pk1 - pk0, o[2] = pk2 - pk1, o[3] = pk3 - pk2, o[4] = pk4 - pk3, o[5] = pk5 - pk4, o[6] = pk6 - pk5, o[10] = pk6 - pk0;
    }
#endif
}

// slot of node a in the block row of each of its columns (the mirror position of block (a, slot)); 255 = not there
__global__ __launch_bounds__(256) void s6_rslot_kernel(Solve6View s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.D * s.cap) return;
    const int a = i / s.cap, q = i - a * s.cap;
    int r = 255;
    if (q < s.bcnt[a]) {
        const int b = s.bcols[i];
        if (q == 0) r = 0;
        else if (b >= 0) {
            const int32_t* cb = s.bcols + (size_t)b * s.cap;
            const int nb      = s.bcnt[b];
            for (int t = 1; t < nb; ++t)
                if (cb[t] == a) r = t;
        }
    }
    s.rslot[i] = (uint8_t)r;
}

}  // namespace

hipError_t s6_launch_pattern(const Solve6View& s, Solve6State* state, hipStream_t st) {
    s6_pattern_kernel<<<s.D, 256, 0, st>>>(s, state);
    s6_rslot_kernel<<<(s.D * s.cap + 255) / 256, 256, 0, st>>>(s);
    return hipGetLastError();
}

}  // namespace dfa
