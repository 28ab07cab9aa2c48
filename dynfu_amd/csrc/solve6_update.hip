// solve6_update.hip — the launches of the north-star solve that produce node transforms, and with them g^_n and M_n
// for the next linearisation (s6_node_now): s6_begin (start of a solve: the caller's transforms, a cleared state block)
// and s6_update (the PCG's twist applied on the left, or a rejected step undone; it also closes the PCG's bookkeeping);
// and s6_warp, the solve's own warp of its vertices by the blend the linearisation uses.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "solve6.hpp"
#include "solve6_internal.hpp"

namespace dfa {

namespace {

// ------------------------------------------------------------------------------------ update
__global__ __launch_bounds__(256) void s6_update_kernel(Solve6View s, Solve6State* st, int launched, int linear_iter,
                                                        int* __restrict__ mirror, int h, int apply) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    // Gauss-Newton control (written by the linearisation's last workgroup, by no thread of this launch): 0 = apply the step; 1 = the outer iteration
    // has ended, nothing moves; 2 = ended by a rejected step: the transforms before that step come back (every update
    // launch until the next outer iteration does this again: the same values)
    const int stop = st->gn_stop;
    if (blockIdx.x == 0 && threadIdx.x < 64 && apply) {
        // a PCG that used every launch it was given: its last (r, u) is still in the per-workgroup partials of the last launch
        const bool ran = !st->pcg_done && launched > 0 && st->pcg_last_it == launched;  // (uniform)
        bool reached   = !ran;
        if (ran) {
            const int nb = s6_matvec_blocks(s.D);
            float g = 0.f;
            for (int i = threadIdx.x; i < nb; i += 64) g += s.g_part[launched & 1][i];
            g = wave_sum_all(g);
            const float rz0 = st->rz0;
            reached         = !(g > st->tol2 * rz0);
            if (threadIdx.x == 0 && h >= 0 && h < S6_HIST) st->pcg_rel_hist[h] = g > 0.f && rz0 > 0.f ? sqrtf(g / rz0) : 0.f;
        }
        if (threadIdx.x == 0) {
            st->cost = 0.0, st->valid = 0ull;  // accumulators of the next linearisation
            const bool cut = !reached && launched < linear_iter;  // stopped by the plan's prediction, not by the caller's cap
            if (cut) st->pcg_short += 1;
            // (an iteration without a PCG — the outer iteration had ended — tells the launch budget so: S6_MIRROR_SKIPPED)
            if (mirror && h >= 0 && h < S6_HIST) mirror[h] = stop ? S6_MIRROR_SKIPPED : cut ? -st->pcg_last_it : st->pcg_last_it;
        }
    }
    if (n >= s.D) return;
    if (stop == 2) {
        const DQ q = dq_load(s.dq_prev + 8 * (size_t)n);
        dq_store(s.dq + 8 * (size_t)n, q);
        s6_node_now(s, n, q);
        return;
    }
    if (stop || !apply) return;
    const float* tw = s.x + 6 * (size_t)n;
    const DQ q      = dq_load(s.dq + 8 * (size_t)n);
    dq_store(s.dq_prev + 8 * (size_t)n, q);
    const f3 gh     = mk3(s.ghat[3 * n], s.ghat[3 * n + 1], s.ghat[3 * n + 2]);
    const float th  = sqrtf(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]);
    const float sc  = th > 1e-6f ? sinf(0.5f * th) / th : 0.5f;
    const Quat qo   = Quat{cosf(0.5f * th), sc * tw[0], sc * tw[1], sc * tw[2]};
    Quat rn         = qmul(qo, q.r);
    const f3 t0     = qvec(qmul(q.d, qconj(q.r)));
    const f3 tc     = mk3(2.f * t0.x - gh.x, 2.f * t0.y - gh.y, 2.f * t0.z - gh.z);
    const f3 tr     = qvec(qmul(qmul(qo, pureq(tc)), qconj(qo)));
    const f3 t      = mk3(tr.x + gh.x + tw[3], tr.y + gh.y + tw[4], tr.z + gh.z + tw[5]);
    rn              = qscale(rn, 1.f / sqrtf(qdot(rn, rn)));
    const Quat dn   = qscale(qmul(pureq(t), rn), 0.5f);
    dq_store(s.dq + 8 * (size_t)n, DQ{rn, dn});
    s6_node_now(s, n, DQ{rn, dn});  // for the next linearisation
}

template <int K>
__global__ __launch_bounds__(256) void s6_warp_kernel(Solve6View s, const float* __restrict__ dq,
                                                      float* __restrict__ out_v, float* __restrict__ out_n) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= s.N) return;
    int32_t idx[K];
    float wn[K];
    if (s.k == K) {  // (uniform) 16-byte loads, as the linearisation
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const int4 iv   = reinterpret_cast<const int4*>(s.idx + (size_t)v * K)[q];
            const float4 wv = reinterpret_cast<const float4*>(s.wn + (size_t)v * K)[q];
            idx[4 * q] = iv.x, idx[4 * q + 1] = iv.y, idx[4 * q + 2] = iv.z, idx[4 * q + 3] = iv.w;
            wn[4 * q] = wv.x, wn[4 * q + 1] = wv.y, wn[4 * q + 2] = wv.z, wn[4 * q + 3] = wv.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            idx[j] = j < s.k ? s.idx[(size_t)v * s.k + j] : -1;
            wn[j]  = j < s.k ? s.wn[(size_t)v * s.k + j] : 0.f;
        }
    }
    Blend<K> B;
    blend<K>(dq, idx, wn, s.k, B);
    const f3 c = mk3(s.canon[3 * (size_t)v], s.canon[3 * (size_t)v + 1], s.canon[3 * (size_t)v + 2]);
    const f3 p = B.m > 0.f ? blend_point<K>(B, c) : c;
    const size_t o = s.vperm[v];  // the caller's index of the solver's vertex v
    out_v[3 * o] = p.x, out_v[3 * o + 1] = p.y, out_v[3 * o + 2] = p.z;
    if (out_n && s.canon_n) {
        const f3 n0 = mk3(s.canon_n[3 * (size_t)v], s.canon_n[3 * (size_t)v + 1], s.canon_n[3 * (size_t)v + 2]);
        const f3 n  = B.m > 0.f ? blend_normal<K>(B, n0) : n0;
        out_n[3 * o] = n.x, out_n[3 * o + 1] = n.y, out_n[3 * o + 2] = n.z;
    }
}

__global__ __launch_bounds__(256) void s6_begin_kernel(Solve6View s, Solve6State* st, const float* __restrict__ node_dq, int slots) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S6_HIST) {  // gn_tol > 0: every slot the solve enqueues starts as "skipped"; the ones that run overwrite theirs
        st->cost_hist[i] = 0.0, st->valid_hist[i] = 0u, st->pcg_it_hist[i] = 0, st->pcg_rel_hist[i] = 0.f, st->pcg_tol_hist[i] = 0.f;
        st->stop_hist[i] = i < slots ? 3 : 0;
    }
    if (i <= S6_LIN_SHARDS) st->lin_ticket[i] = 0u;
    if (i == 0) {
        st->cost = 0.0, st->initial_cost = 0.0, st->final_cost = 0.0;
        st->valid = st->valid_first = st->valid_last = 0ull;
        st->have_first = 0, st->gn_iters = 0, st->pcg_iters = 0;  // overflow / max_row_blocks belong to the pattern
        st->pcg_done = 0, st->rz0 = 0.f, st->pcg_short = 0, st->rz0_gn[0] = st->rz0_gn[1] = 0.f;
        st->cur = 0, st->hist_n = min(slots, S6_HIST), st->gn_stop = 0, st->gn_solves = 0, st->gn_rejected = 0, st->gn_converged = 0;
        st->cost_ref = 0.0, st->valid_ref = 0ull;
    }
    if (i < 8 * s.D) s.dq[i] = node_dq[i], s.dq_prev[i] = node_dq[i];
    if (i < s.N) s.rho[i] = 0.f;
    if (i < s.D * s.k) s.rhub[i] = 1.f;
    if (i < s.D) s6_node_now(s, i, dq_load(node_dq + 8 * (size_t)i));
}

}  // namespace

hipError_t s6_begin(const Solve6View& s, Solve6State* state, const float* node_dq, int slots, hipStream_t st) {
    const int n = std::max(std::max(std::max(8 * s.D, s.N), s.D * s.k), S6_HIST + S6_LIN_SHARDS);
    s6_begin_kernel<<<(n + 255) / 256, 256, 0, st>>>(s, state, node_dq, slots);
    return hipGetLastError();
}

hipError_t s6_update(const Solve6View& s, Solve6State* state, int launched, int linear_iter, int* mirror, int gi, int apply,
                     hipStream_t st) {
    s6_update_kernel<<<(s.D + 255) / 256, 256, 0, st>>>(s, state, launched, linear_iter, mirror, gi, apply);
    return hipGetLastError();
}

hipError_t s6_warp(const Solve6View& s, const float* dq, float* out_v, float* out_n, hipStream_t st) {
    if (s.N == 0) return hipSuccess;
    K6DISPATCH(s6_warp_kernel, s.k, <<<(s.N + 255) / 256, 256, 0, st>>>(s, dq, out_v, out_n));
    return hipGetLastError();
}

}  // namespace dfa
