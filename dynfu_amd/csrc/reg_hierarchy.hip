// reg_hierarchy.hip — the multi-level regularisation graph of the north-star solve (rule: include/dynfu_amd.h,
// dfa_solver6_set_reg_hierarchy; restated in numpy by tests/reg_hierarchy_statement.py).  Two stages, both on the caller's
// stream, nothing returns to the host:
//   levels  rh_insert_kernel   a lane per node: its cell at every level >= 1 into an open-addressing table, the cell's
//                              representative the minimum of the node indices that arrive (atomicMin: whatever the order)
//           rh_level_kernel    a lane per node: the highest level whose cell it represents
//   rows    rh_rows_kernel     a wave per node: level 0 from the flat search's list (the k + 1 nearest of all nodes, what
//                              s6_reg_graph_kernel reads), every level above it by the wave's own scan of the nodes of that
//                              level and up — the candidate list and (distance, index) order of knn_device.hpp —, entries
//                              already in the row skipped and the next nearest taken
// The sets of the levels >= 1 are known on the device only, and they are small (a sixteenth of the level below on a surface
// at beta = 4) and asked for by their own members only: a scan filtered by level[] costs D / 64 steps per lane for those few
// waves and needs neither a compacted copy of the positions nor a grid whose size the host would have to know.
#include <hip/hip_runtime.h>

#include "knn_device.hpp"
#include "solve6.hpp"

namespace dfa {

namespace {

constexpr unsigned long long RH_EMPTY = ~0ull;  // (no key: a key's level field is at most 7)
constexpr int RH_CELL_LIMIT = 1 << 20;          // |c0| below this: three 20-bit fields hold the cells of every level >= 1

// c0 = floor(p / epsilon), correctly rounded float32 division; false: the node represents no cell
__device__ __forceinline__ bool rh_cell0(const float* __restrict__ node_pos, int n, float epsilon, int (&c0)[3]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float f = floorf(__fdiv_rn(node_pos[3 * (size_t)n + c], epsilon));
        ok            = ok && fabsf(f) < (float)RH_CELL_LIMIT;  // (false for NaN and +-inf)
        c0[c]         = ok ? (int)f : 0;
    }
    return ok;
}
__device__ __forceinline__ int rh_floor_div(int a, int b) { return a / b - (a % b < 0 ? 1 : 0); }  // b > 0
// beta^l, held at 2^20: every divisor from there on sends a cell to 0 or -1, as the power itself would
__device__ __forceinline__ int rh_next_power(int pw, int beta) {
    return (int)min((long long)pw * beta, (long long)RH_CELL_LIMIT);
}
// level l >= 1 and its cell (each coordinate in [-2^19, 2^19)) as one word
__device__ __forceinline__ unsigned long long rh_key(int l, const int (&c0)[3], int pw) {
    unsigned long long key = (unsigned long long)l;
#pragma unroll
    for (int c = 0; c < 3; ++c) key = key << 20 | (unsigned long long)(rh_floor_div(c0[c], pw) + (RH_CELL_LIMIT >> 1));
    return key;
}
__device__ __forceinline__ unsigned int rh_hash(unsigned long long x, unsigned int mask) {
    x ^= x >> 30, x *= 0xbf58476d1ce4e5b9ull, x ^= x >> 27, x *= 0x94d049bb133111ebull, x ^= x >> 31;
    return (unsigned int)x & mask;
}

// table: `cap` (a power of two, at least twice the keys that can arrive) words of RH_EMPTY, rep: `cap` words of 0xffffffff
__global__ __launch_bounds__(256) void rh_insert_kernel(const float* __restrict__ node_pos, int D, float epsilon, int beta,
                                                        int levels, unsigned long long* __restrict__ table,
                                                        unsigned int* __restrict__ rep, unsigned int mask) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= D) return;
    int c0[3];
    if (!rh_cell0(node_pos, n, epsilon, c0)) return;
    int pw = 1;
    for (int l = 1; l < levels; ++l) {
        pw                           = rh_next_power(pw, beta);
        const unsigned long long key = rh_key(l, c0, pw);
        // (at most half of the table is ever taken: the probe ends at the key or at an empty word)
        for (unsigned int slot = rh_hash(key, mask);; slot = (slot + 1) & mask) {
            const unsigned long long old = atomicCAS(&table[slot], RH_EMPTY, key);
            if (old == RH_EMPTY || old == key) {
                atomicMin(&rep[slot], (unsigned int)n);
                break;
            }
        }
    }
}

__global__ __launch_bounds__(256) void rh_level_kernel(const float* __restrict__ node_pos, int D, float epsilon, int beta,
                                                       int levels, const unsigned long long* __restrict__ table,
                                                       const unsigned int* __restrict__ rep, unsigned int mask,
                                                       int32_t* __restrict__ level) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= D) return;
    int c0[3], lv = 0;
    if (rh_cell0(node_pos, n, epsilon, c0)) {
        int pw = 1;
        for (int l = 1; l < levels; ++l) {
            pw                           = rh_next_power(pw, beta);
            const unsigned long long key = rh_key(l, c0, pw);
            unsigned int slot            = rh_hash(key, mask);
            unsigned long long t;  // (the insert pass put the key there; an empty word ends the probe whatever happens)
            while ((t = table[slot]) != key && t != RH_EMPTY) slot = (slot + 1) & mask;
            if (t == key && rep[slot] == (unsigned int)n) lv = l;  // (cells nest: the levels a node represents are 1 .. lv)
        }
    }
    level[n] = lv;
}

struct RhSlots {
    int levels, slots[S6_REG_LEVELS];
};

// One wave per node.  raw: the flat search's D x kreg list (the node itself among its entries); k <= 8 columns per row.
__global__ __launch_bounds__(256) void rh_rows_kernel(const float* __restrict__ node_pos, const int32_t* __restrict__ level,
                                                      int D, const int32_t* __restrict__ raw, int kreg, RhSlots cfg, int k,
                                                      int32_t* __restrict__ reg_idx) {
    constexpr int K = 8;
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= D) return;
    int row[K], cnt = 0;  // (uniform over the wave)
#pragma unroll
    for (int j = 0; j < K; ++j) row[j] = -1;
    auto append = [&](int m) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j == cnt) row[j] = m;
        ++cnt;
    };
    for (int j = 0; j < kreg && cnt < cfg.slots[0]; ++j) {
        const int m = raw[(size_t)n * kreg + j];
        if (m >= 0 && m != n) append(m);
    }
    const int top = min(level[n], cfg.levels - 1);
    const f3 q    = mk3(node_pos[3 * (size_t)n], node_pos[3 * (size_t)n + 1], node_pos[3 * (size_t)n + 2]);
    for (int l = 1; l <= top; ++l) {
        const int need = min(cfg.slots[l], K - cnt);  // (the slots sum to at most k <= K)
        if (need <= 0) continue;
        // the lane's share of the nodes of level l and up; the `need` the row takes are among the need + cnt nearest of all
        // of them, hence among the K nearest of the lanes that hold them
        KnnList<K> best;
        best.init();
        for (int m = lane; m < D; m += 64)
            if (m != n && level[m] >= l)
                best.push(dist2(q, node_pos[3 * (size_t)m], node_pos[3 * (size_t)m + 1], node_pos[3 * (size_t)m + 2]), m);
        // merge (knn_wave_search's): the wave's minimum of the lanes' heads, K rounds at the most
        int pos = 0, taken = 0;
        for (int round = 0; round < K && taken < need; ++round) {
            unsigned long long key = KnnList<K>::EMPTY;
#pragma unroll
            for (int t = 0; t < K; ++t)
                if (t == pos) key = best.key[t];
            const unsigned long long win = wave_min_u64(key);
            const int m                  = (int)(unsigned int)win;
            if (m == 0x7fffffff) break;  // (uniform) no candidate left
            if (key == win) ++pos;
            bool seen = false;
#pragma unroll
            for (int j = 0; j < K; ++j) seen = seen || row[j] == m;
            if (!seen) append(m), ++taken;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) reg_idx[(size_t)n * k + j] = row[j];
    }
}

}  // namespace

hipError_t reg_hierarchy_levels(const float* node_pos, int D, float epsilon, int beta, int levels, int32_t* level,
                                unsigned long long* table, unsigned int* rep, hipStream_t st) {
    if (D <= 0) return hipSuccess;
    const size_t cap = reg_hierarchy_table(D, levels);
    hipError_t e     = hipMemsetAsync(table, 0xff, sizeof(unsigned long long) * cap, st);
    if (e == hipSuccess) e = hipMemsetAsync(rep, 0xff, sizeof(unsigned int) * cap, st);
    if (e != hipSuccess) return e;
    const unsigned int mask = (unsigned int)(cap - 1);
    rh_insert_kernel<<<(D + 255) / 256, 256, 0, st>>>(node_pos, D, epsilon, beta, levels, table, rep, mask);
    rh_level_kernel<<<(D + 255) / 256, 256, 0, st>>>(node_pos, D, epsilon, beta, levels, table, rep, mask, level);
    return hipGetLastError();
}

hipError_t reg_hierarchy_rows(const float* node_pos, int D, const int32_t* raw_reg, int kreg, const S6RegHierarchy& h, int k,
                              int32_t* reg_idx, hipStream_t st) {
    if (D <= 0) return hipSuccess;
    hipError_t e = reg_hierarchy_levels(node_pos, D, h.epsilon, h.beta, h.levels, h.level, h.table, h.rep, st);
    if (e != hipSuccess) return e;
    RhSlots cfg{};
    cfg.levels = h.levels;
    for (int l = 0; l < S6_REG_LEVELS; ++l) cfg.slots[l] = l < h.levels ? h.slots[l] : 0;
    rh_rows_kernel<<<(D + 3) / 4, 256, 0, st>>>(node_pos, h.level, D, raw_reg, kreg, cfg, k, reg_idx);
    return hipGetLastError();
}

}  // namespace dfa
