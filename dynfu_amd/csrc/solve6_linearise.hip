// solve6_linearise.hip — the linearisation of the north-star solve (formulation: solve6.hpp), ONE launch per
// Gauss-Newton iteration: a lane per vertex blends, projects, gates and writes the vertex's record (l, the k scalars
// h_j, sqrt(rho) r); further workgroups of the same launch take a regularisation edge per lane; every workgroup leaves
// its share of the energy, and with gn_tol > 0 the last one to arrive sums them and applies the Gauss-Newton stopping
// rule.  s6_forcing: the PCG tolerance that goes with the iteration.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "solve6.hpp"
#include "solve6_internal.hpp"

namespace dfa {

namespace {

// (the blend itself — Blend, blend, blend_point, blend_normal — is blend6_device.hpp, shared with the warped TSDF sweep)

__device__ __forceinline__ float tukey6(float err, float offset, float c) {  // opt_solver.cpp:204-231
    const float e = err / offset;
    if (e < c) {
        const float t = 1.f - (e * e) / (c * c);
        return t * t;
    }
    return 0.f;
}

__device__ __forceinline__ double s6_reg_edge(const Solve6View& s, int e, float wreg2, float psi_reg, int update_w);

// gn_tol > 0: the Gauss-Newton stopping rule (oracle/oracle.h: orc6_params.gn_tol states it; the reference runs Opt with
// earlyOut = true and nonLinearIter as a cap, src/dynfu/dyn_fusion.cpp:183-189) and the bookkeeping s6_bookkeeping does
// otherwise — by ONE thread of the linearisation's last workgroup, after s6_cost_total: the assembly's workgroups, which run
// next, must already know (a launch behind an ended outer iteration returns at entry).  Slots that are skipped write
// nothing: s6_begin has marked every slot "skipped".
__device__ __forceinline__ void s6_decide(Solve6State* st, const S6Decide& d) {
    const bool in = d.gi < S6_HIST;
    const double cost = st->cost;
    const unsigned long long valid = st->valid;
    if (!st->have_first) st->initial_cost = cost, st->valid_first = valid, st->have_first = 1;
    int stop = 0;
    if (d.gn > 0) {
        const double ref = st->cost_ref;
        if (cost > (1.0 + (double)d.gn_tol) * ref) stop = 2;                       // the step raised the energy: undone
        else if (d.closing || ref - cost <= (double)d.gn_tol * ref) stop = 1;      // converged: kept, no further step
    }
    if (stop == 2) {
        st->final_cost = st->cost_ref, st->valid_last = st->valid_ref, st->gn_rejected += 1;
    } else {
        st->final_cost = cost, st->valid_last = valid;
        if (stop == 1) st->gn_converged += d.closing ? 0 : 1;
        else st->cost_ref = cost, st->valid_ref = valid, st->gn_solves += 1;
    }
    if (in) {
        st->cost_hist[d.gi] = cost, st->valid_hist[d.gi] = (unsigned int)valid, st->pcg_it_hist[d.gi] = 0;
        st->pcg_rel_hist[d.gi] = stop ? 0.f : 1.f, st->pcg_tol_hist[d.gi] = stop ? 0.f : sqrtf(d.f.tol2), st->stop_hist[d.gi] = stop;
        if (st->hist_n < d.gi + 1) st->hist_n = d.gi + 1;
    }
    st->gn_iters += 1, st->cur = d.gi, st->gn_stop = stop;
    st->tol2 = d.f.tol2, st->pcg_last_it = 0, st->pcg_done = stop != 0;
    st->ew_gamma = d.f.ew_gamma, st->ew_min2 = d.f.ew_min2, st->ew_max2 = d.f.ew_max2, st->ew_slot = d.f.ew_slot;
}

// Tail of the linearisation when it decides (gn_tol > 0): every workgroup has published its partial sums write-through
// (block_add_cost); thread 0 waits for that store to leave, then arrives — a counter per shard, a top counter for the last
// arriver of each shard (one word would serialise ~2 000 device-scope atomics at ~11 ns each), re-armed by whoever
// completes them — and the LAST workgroup of the launch sums the partials in their fixed order and decides.  The pattern
// of the reference-mode linearise_kernel (solve_linearise.hip).  One launch fewer per Gauss-Newton slot than the one-workgroup kernel
// this replaced — which measured the same frame time (C2 841 against 845 frames/s, C3 317.5 against 316.8: that launch hid
// in the stream's launch pipeline).
__device__ __forceinline__ void s6_linearise_tail(const Solve6View& s, Solve6State* st, const S6Decide& d) {
    __shared__ int is_last;
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int shard   = blockIdx.x % S6_LIN_SHARDS;
        const unsigned int members = (gridDim.x - shard + S6_LIN_SHARDS - 1) / S6_LIN_SHARDS;
        const unsigned int nshards = min((unsigned int)S6_LIN_SHARDS, gridDim.x);
        int last                   = 0;
        if (__hip_atomic_fetch_add(&st->lin_ticket[shard], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == members - 1) {
            __hip_atomic_store(&st->lin_ticket[shard], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(&st->lin_ticket[S6_LIN_SHARDS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nshards - 1) {
                __hip_atomic_store(&st->lin_ticket[S6_LIN_SHARDS], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = 1;
            }
        }
        is_last = last;
    }
    __syncthreads();
    if (!is_last) return;
    s6_cost_total(s, st, true);
    if (threadIdx.x == 0) s6_decide(st, d);
}

// may vertex v (the plan's sorted order) take a data row?  Without a mask: always; with one: where its byte is set
__device__ __forceinline__ bool s6_unmasked(int) { return true; }
__device__ __forceinline__ bool s6_unmasked(int v, const uint8_t* vmask) { return vmask[v] != 0; }

// blocks [0, nlin): the data term, a lane per vertex; blocks from nlin on: the regulariser, a lane per edge.
// MASKED: the plan has a vertex mask (dfa_solver6_set_vertex_mask) and the launch one argument more, the mask in the plan's
// sorted order — a zero byte sends the vertex down the path of a vertex without association: a record of zeros, no energy,
// not counted, its rho left alone.  The instantiations without MASKED have no such argument (Mask is empty) and are the
// code they were before the mask existed.
template <int K, bool MASKED, class... Mask>
__global__ __launch_bounds__(256) void s6_linearise_kernel(Solve6View s, Solve6State* st, Solve6Image img,
                                                           Solve6Params prm, int update_w, int nlin, float wreg2, int gate,
                                                           const S6Decide dec, Mask... vmask) {
    static_assert(sizeof...(Mask) == (MASKED ? 1 : 0), "the mask pointer is the masked instantiation's argument alone");
    if (gate && st->gn_stop) return;  // (uniform) the outer iteration has ended: nothing to linearise, nothing to decide
    if ((int)blockIdx.x >= nlin) {  // (uniform)
        const int e = ((int)blockIdx.x - nlin) * 256 + (int)threadIdx.x;
        block_add_cost(e < s.D * s.k ? s6_reg_edge(s, e, wreg2, prm.psi_reg, update_w) : 0.0, 0u, s, dec.on != 0);
        if (dec.on) s6_linearise_tail(s, st, dec);
        return;
    }
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    double cost = 0.0;
    unsigned int nvalid = 0;
    if (v < s.N) {
        const int k = s.k;
        int32_t idx[K];
        float wn[K];
        if (k == K) {  // (uniform) the vertex's neighbours and weights as 16-byte loads: K / 4 each instead of K dwords
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
                idx[j] = j < k ? s.idx[(size_t)v * k + j] : -1;
                wn[j]  = j < k ? s.wn[(size_t)v * k + j] : 0.f;
            }
        }
        float w_eff = 0.f, rr = 0.f;
        bool ok     = false;
        float h[K], swr = 0.f;
        float4 l0 = make_float4(0.f, 0.f, 0.f, 0.f), l1 = l0;
#pragma unroll
        for (int j = 0; j < K; ++j) h[j] = 0.f;
        Blend<K> B;
        blend<K>(s.dq, idx, wn, k, B);
        const f3 c = mk3(s.canon[3 * (size_t)v], s.canon[3 * (size_t)v + 1], s.canon[3 * (size_t)v + 2]);
        f3 p = c, nl = mk3(0.f, 0.f, 0.f);
        if (B.m > 0.f && s6_unmasked(v, vmask...)) {
            p = blend_point<K>(B, c);
            if (p.z > 0.f) {
                // nearest pixel (proj_icp.cu:80-86 uses __float2int_rn)
                const int u = (int)rintf(img.fx * (p.x / p.z) + img.cx), w = (int)rintf(img.fy * (p.y / p.z) + img.cy);
                if (u >= 0 && w >= 0 && u < img.cols && w < img.rows) {
                    const float4 L  = *reinterpret_cast<const float4*>((const char*)img.vmap + (size_t)w * img.vstep + 16 * (size_t)u);
                    const float4 Ln = *reinterpret_cast<const float4*>((const char*)img.nmap + (size_t)w * img.nstep + 16 * (size_t)u);
                    if (L.x == L.x && Ln.x == Ln.x) {
                        const f3 dl      = mk3(p.x - L.x, p.y - L.y, p.z - L.z);
                        const float dist = sqrtf(dot3(dl, dl));
                        nl               = mk3(Ln.x, Ln.y, Ln.z);
                        bool gate        = dist <= prm.dist_thresh;
                        if (gate && s.canon_n) {
                            const f3 n0 = mk3(s.canon_n[3 * (size_t)v], s.canon_n[3 * (size_t)v + 1], s.canon_n[3 * (size_t)v + 2]);
                            gate        = dot3(blend_normal<K>(B, n0), nl) >= prm.cos_thresh;
                        }
                        if (gate) ok = true, rr = dot3(nl, dl);
                    }
                }
            }
        }
        if (ok) {
            if (update_w) s.rho[v] = tukey6(fabsf(rr), prm.tukey_offset, prm.psi_data);
            w_eff = s.rho[v];
            // n . dp = lW . W + lD . Wd  for the twist's (W, Wd) = (omega^ r, omega^ d + v0^ r), times w~ s / m
            const Quat ac = qconj(B.a), nq = pureq(nl);
            const Quat T = qmul(ac, nq);                                  // a* n^
            const Quat U = qmul(qmul(pureq(c), ac), nq);                  // (c^ a*) n^
            const Quat S = qscale(qmul(qconj(B.b), nq), -1.f);            // -b* n^
            const float np = dot3(nl, p);
            const Quat lD = Quat{-T.w, T.x, T.y, T.z};
            const Quat lW = Quat{-(U.w + S.w) - np * B.a.w, (U.x + S.x) - np * B.a.x, (U.y + S.y) - np * B.a.y,
                                 (U.z + S.z) - np * B.a.z};
            const float im = 1.f / B.m;
            // row of the Jacobian for neighbour j: f_j * M_j l with l = (lW, lD); see s6_node_now.  ONE record per vertex —
            // l, the k scalars f, the robust weight — which the assembly gathers through each node's row list (round 2
            // wrote the record once per neighbour, at the row's place in that node's list: k times the bytes, and an
            // index scatter to build per frame)
            // ... with the robust weight folded in: h_j = sqrt(rho) f_j, so that rho f_a f_b = h_a h_b is ONE product in the
            // assembly, rows without weight vanish by themselves, and -J^T r needs (sqrt(rho) r) h_a
            const float sw = sqrtf(w_eff);
#pragma unroll
            for (int j = 0; j < K; ++j) h[j] = j < k ? sw * (wn[j] * B.s[j] * im) : 0.f;
            l0 = make_float4(lW.w, lW.x, lW.y, lW.z), l1 = make_float4(lD.w, lD.x, lD.y, lD.z);
            swr    = sw * rr;
            cost   = (double)w_eff * (double)rr * (double)rr;
            nvalid = w_eff > 0.f;
        }
        // no association: a record of zeros (l too: 0 x a stale NaN would be NaN)
        float4* rec = reinterpret_cast<float4*>(s.rec + (12 + K) * (size_t)v);  // 2 + K / 4 + 1 chunks of 16 bytes per vertex
        rec[0] = l0, rec[1] = l1;
#pragma unroll
        for (int q = 0; q < K / 4; ++q) rec[2 + q] = make_float4(h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
        rec[2 + K / 4] = make_float4(swr, 0.f, 0.f, 0.f);
    }
    block_add_cost(cost, nvalid, s, dec.on != 0);
    if (dec.on) s6_linearise_tail(s, st, dec);
}

__device__ __forceinline__ double s6_reg_edge(const Solve6View& s, int e, float wreg2, float psi_reg, int update_w) {
    double cost = 0.0;
    const int n = e / s.k, m = s.reg_idx[e];
    float* er = s.rres + 3 * (size_t)e;
    float* vc = s.rvec + 18 * (size_t)e;
    float ev[3] = {0.f, 0.f, 0.f}, vec[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) vec[i] = 0.f;
    if (m >= 0) {
        const f3 y   = dq_point(dq_load(s.dq + 8 * (size_t)n), mk3(s.node_pos[3 * m], s.node_pos[3 * m + 1], s.node_pos[3 * m + 2]));
        const f3 ghm = mk3(s.ghat[3 * m], s.ghat[3 * m + 1], s.ghat[3 * m + 2]);
        const f3 ghn = mk3(s.ghat[3 * n], s.ghat[3 * n + 1], s.ghat[3 * n + 2]);
        ev[0] = y.x - ghm.x, ev[1] = y.y - ghm.y, ev[2] = y.z - ghm.z;
        const float en = sqrtf(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
        if (update_w) s.rhub[e] = en <= psi_reg ? 1.f : psi_reg / en;  // opt_solver.cpp:233-268
        const float l0 = y.x - ghn.x, l1 = y.y - ghn.y, l2 = y.z - ghn.z;
        // rows of [ -[l]x | I ]
        vec[0] = 0.f, vec[1] = l2, vec[2] = -l1, vec[3] = 1.f;
        vec[6] = -l2, vec[7] = 0.f, vec[8] = l0, vec[10] = 1.f;
        vec[12] = l1, vec[13] = -l0, vec[14] = 0.f, vec[17] = 1.f;
        cost = (double)wreg2 * (double)s.rhub[e] * (double)en * (double)en;
    }
    er[0] = ev[0], er[1] = ev[1], er[2] = ev[2];
#pragma unroll
    for (int i = 0; i < 18; ++i) vc[i] = vec[i];
    return cost;
}

}  // namespace

hipError_t s6_linearise(const Solve6View& s, Solve6State* state, const Solve6Image& img, const Solve6Params& p,
                        int update_weights, int gi, int gn_in_outer, int closing, const uint8_t* vmask, hipStream_t st) {
    // (g^, M of the nodes and the cleared cost accumulators come from the launch that produced the transforms:
    // s6_begin / s6_update)
    const float wreg2 = p.lambda / ((float)s.D * (float)s.k);
    const int nlin = (s.N + 255) / 256, nreg = (s.D * s.k + 255) / 256;
    // gn_tol > 0: a linearisation that does not open an outer iteration is skipped once that iteration has ended
    const int gate = p.gn_tol > 0.f && !update_weights;
    const S6Decide dec{p.gn_tol > 0.f ? 1 : 0, gi, gn_in_outer, closing, p.gn_tol, s6_forcing(p, gn_in_outer)};
    // (K6DISPATCH's choice of K, by hand: the kernel has a second template argument)
    const dim3 grid(nlin + nreg), block(256);
    if (vmask) {
        if (s.k <= 4) s6_linearise_kernel<4, true><<<grid, block, 0, st>>>(s, state, img, p, update_weights, nlin, wreg2, gate, dec, vmask);
        else s6_linearise_kernel<8, true><<<grid, block, 0, st>>>(s, state, img, p, update_weights, nlin, wreg2, gate, dec, vmask);
    } else {
        if (s.k <= 4) s6_linearise_kernel<4, false><<<grid, block, 0, st>>>(s, state, img, p, update_weights, nlin, wreg2, gate, dec);
        else s6_linearise_kernel<8, false><<<grid, block, 0, st>>>(s, state, img, p, update_weights, nlin, wreg2, gate, dec);
    }
    return hipGetLastError();
}

S6Forcing s6_forcing(const Solve6Params& p, int gn_in_outer) {
    S6Forcing f{p.pcg_tol * p.pcg_tol, 0.f, 0.f, 0.f, gn_in_outer & 1, p.gn_tol > 0.f ? 1 : 0};
    if (p.pcg_tol_first > 0.f && p.pcg_tol_adapt > 0.f) {
        // adaptive: the first iteration of an outer iteration at pcg_tol_first (no previous gradient under these weights),
        // the others decided on the device; ew_gamma = 0 keeps the tolerance given here
        const float hi = std::max(p.pcg_tol_first, p.pcg_tol);
        f.tol2 = hi * hi, f.ew_min2 = p.pcg_tol * p.pcg_tol, f.ew_max2 = hi * hi;
        f.ew_gamma = gn_in_outer > 0 ? p.pcg_tol_adapt : 0.f;
    } else if (p.pcg_tol_first > 0.f) {
        float e = p.pcg_tol_first;
        for (int i = 0; i < gn_in_outer; ++i) e *= p.pcg_tol_decay;
        const float eta = std::max(p.pcg_tol, e);
        f.tol2 = eta * eta;
    }
    return f;
}

}  // namespace dfa
