// solve_rows.hpp — the row graph and the packed row record of the reference-mode solve, stated once (internal).
//
// Row r of the R = N + D k residual rows (solve.hpp: formulation) exists twice in a plan:
//   the row graph   ridx[r][k], rw[r][k]: node per slot (-1 = empty) and slot weight — what the searches leave, what the
//                   transposition (solve_graph.hip) and the linearisation read;
//   the row record  re[r]: solve_rec_words(k) consecutive words (solve.hpp: solve_rec_ids16 / _words / _tail) =
//                   head: k node ids (16-bit where solve_rec_ids16(k), 0xffff = empty; else 32-bit, -1 = empty), k weights
//                   tail: e = b - sum w t (3 words), tau
//                   — one or two cache lines per row, all an assembly workgroup reads of it.
// Who writes which words:
//   head   store_record_head   once per problem, by prepare_rows_kernel / graph_rows_kernel (solve_graph.hip)
//   tail   a float4 store at solve_rec_tail(k), once per linearisation, by linearise_kernel (solve_linearise.hip)
//   read   load_record         head and tail together, by assemble_kernel / assemble_det_kernel (solve_assemble.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "solve.hpp"

namespace dfa {

// a row's k node ids and weights: 16-byte loads when k is the template's K (the common case), k dwords else; absent: -1 / 0
template <int K>
__device__ __forceinline__ void load_row_graph(const SolveView& s, size_t r, int (&n)[K], float (&w)[K]) {
    if (s.k == K) {  // (uniform)
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const int4 iv   = reinterpret_cast<const int4*>(s.ridx + r * K)[q];
            const float4 wv = reinterpret_cast<const float4*>(s.rw + r * K)[q];
            n[4 * q] = iv.x, n[4 * q + 1] = iv.y, n[4 * q + 2] = iv.z, n[4 * q + 3] = iv.w;
            w[4 * q] = wv.x, w[4 * q + 1] = wv.y, w[4 * q + 2] = wv.z, w[4 * q + 3] = wv.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) n[j] = j < s.k ? s.ridx[r * s.k + j] : -1, w[j] = j < s.k ? s.rw[r * s.k + j] : 0.f;
    }
}

// head of row r's packed record (the words before (e, tau)): its k node ids — 16-bit where solve_rec_ids16(k) — and k weights
template <int K>
__device__ __forceinline__ void store_record_head(const SolveView& s, size_t r, const int (&ids)[K], const float (&ws)[K], bool wide) {
    const int k = s.k;
    float* rec = s.re + r * (size_t)solve_rec_words(k);
    if (wide) {  // the record's head (the words before (e, tau)) as float4 stores: a lane's record is 48 or 64 contiguous bytes
        float4* rec4 = reinterpret_cast<float4*>(rec);
        if (solve_rec_ids16(k)) {  // K / 2 words of 16-bit id pairs, then K weights
            uint32_t pk[K / 2];
#pragma unroll
            for (int j = 0; j < K / 2; ++j) {
                const uint32_t lo = ids[2 * j] < 0 ? 0xffffu : (uint32_t)ids[2 * j], hi = ids[2 * j + 1] < 0 ? 0xffffu : (uint32_t)ids[2 * j + 1];
                pk[j]             = (lo & 0xffffu) | (hi << 16);
            }
#pragma unroll
            for (int q = 0; q < K / 8; ++q)
                rec4[q] = make_float4(__uint_as_float(pk[4 * q]), __uint_as_float(pk[4 * q + 1]), __uint_as_float(pk[4 * q + 2]), __uint_as_float(pk[4 * q + 3]));
#pragma unroll
            for (int q = 0; q < K / 4; ++q) rec4[K / 8 + q] = make_float4(ws[4 * q], ws[4 * q + 1], ws[4 * q + 2], ws[4 * q + 3]);
        } else {  // K ids, then K weights
#pragma unroll
            for (int q = 0; q < K / 4; ++q)
                rec4[q] = make_float4(__int_as_float(ids[4 * q]), __int_as_float(ids[4 * q + 1]), __int_as_float(ids[4 * q + 2]), __int_as_float(ids[4 * q + 3]));
#pragma unroll
            for (int q = 0; q < K / 4; ++q) rec4[K / 4 + q] = make_float4(ws[4 * q], ws[4 * q + 1], ws[4 * q + 2], ws[4 * q + 3]);
        }
        return;
    }
    if (solve_rec_ids16(k)) {  // k / 2 words of 16-bit ids (0xffff = empty slot), then k weights
        uint16_t* h = reinterpret_cast<uint16_t*>(rec);
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) h[j] = ids[j] < 0 ? (uint16_t)0xffffu : (uint16_t)ids[j], rec[k / 2 + j] = ws[j];
        return;
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) rec[j] = __int_as_float(ids[j]), rec[k + j] = ws[j];
}

// one row record = solve_rec_words(k) consecutive words (head: prepare_rows_kernel, tail: linearise_kernel)
template <int K>
__device__ __forceinline__ float4 load_record(const SolveView& s, size_t r, int (&idx)[K], float (&w)[K]) {
    const float* rec = s.re + r * (size_t)solve_rec_words(s.k);
    if (s.k == K && (K % 8) == 0) {  // 16-bit ids: K / 8 + K / 4 + 1 aligned 16-byte loads (K = 8: one cache line)
        const float4* v = (const float4*)rec;
#pragma unroll
        for (int q = 0; q < K / 8; ++q) {
            const float4 i4 = v[q];
            const uint32_t u[4] = {__float_as_uint(i4.x), __float_as_uint(i4.y), __float_as_uint(i4.z), __float_as_uint(i4.w)};
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const int lo = (int)(u[h] & 0xffffu), hi = (int)(u[h] >> 16);
                idx[8 * q + 2 * h]     = lo == 0xffff ? -1 : lo;
                idx[8 * q + 2 * h + 1] = hi == 0xffff ? -1 : hi;
            }
        }
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const float4 w4 = v[K / 8 + q];
            w[4 * q] = w4.x, w[4 * q + 1] = w4.y, w[4 * q + 2] = w4.z, w[4 * q + 3] = w4.w;
        }
        return v[K / 8 + K / 4];
    }
    if (solve_rec_ids16(s.k)) {  // (k a multiple of 8 below the kernel's K)
        const uint16_t* ids = reinterpret_cast<const uint16_t*>(rec);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            idx[j] = j < s.k ? (ids[j] == 0xffffu ? -1 : (int)ids[j]) : -1;
            w[j]   = j < s.k ? rec[s.k / 2 + j] : 0.f;
        }
        const float* tl = rec + solve_rec_tail(s.k);
        return make_float4(tl[0], tl[1], tl[2], tl[3]);
    }
    if (s.k == K && (K % 4) == 0) {
        const float4* v = (const float4*)rec;  // (2K+4)*4 bytes is a multiple of 16
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const float4 i4 = v[q], w4 = v[K / 4 + q];
            idx[4 * q] = __float_as_int(i4.x), idx[4 * q + 1] = __float_as_int(i4.y);
            idx[4 * q + 2] = __float_as_int(i4.z), idx[4 * q + 3] = __float_as_int(i4.w);
            w[4 * q] = w4.x, w[4 * q + 1] = w4.y, w[4 * q + 2] = w4.z, w[4 * q + 3] = w4.w;
        }
        return v[K / 2];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        idx[j] = j < s.k ? __float_as_int(rec[j]) : -1;
        w[j]   = j < s.k ? rec[s.k + j] : 0.f;
    }
    return make_float4(rec[2 * s.k], rec[2 * s.k + 1], rec[2 * s.k + 2], rec[2 * s.k + 3]);
}

}  // namespace dfa
