// solve_pcg_launched.hip — the block-Jacobi PCG of the reference-mode solve across many workgroups, one launch per
// iteration: the form for plans the teams (solve_pcg_team.hip) cannot serve or have given up on.  Kernels, the cache of
// HIP graphs that replays a chunk of iterations as one host call, and the chunked launcher route_pcg (solve_pcg.hip) calls.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_math.hpp"
#include "pcg_rules.hpp"
#include "solve.hpp"
#include "solve_internal.hpp"

namespace dfa {

// ------------------------------------------------------------------------------------------
// PCG across many workgroups, for plans with more than 2048 nodes (above 8192 the single-workgroup kernels cannot
// hold p in one CU's LDS at all; between 2048 and 8192 they spend ~1 ms per launch sorting and repacking the matrix).
// Preconditioned CG, same stopping rules as the single-workgroup kernels (solve_pcg.hip), one launch per iteration — kernel boundaries are the grid
// barriers (a software barrier over 512 workgroups costs 9 - 41 us on this part, a boundary ~4 us:
// tools/microbench_gridbarrier.hip).  16 lanes per row over the slot-major ELL as assembled, no repacking.  (The first
// form, textbook PCG with two launches per iteration, was replaced by the one below: DESIGN_NOTES.md.)
constexpr int MB_LPR = 16;  // lanes per row

__device__ __forceinline__ float sum_partials_mb(const float* __restrict__ part, int n) {
    float acc = 0.f;
    for (int i = threadIdx.x & 63; i < n; i += 64) acc += part[i];
    return wave_sum_all(acc);  // the same value, the same order, in every wave
}

__global__ __launch_bounds__(256) void pcg_mb_init_kernel(SolveView s, SolveState* __restrict__ st) {
    __shared__ float sh[4];
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a == 0) {
        st->mb_done = st->done || st->converged ? 1 : 0, st->mb_skip = st->done ? 1 : 0, st->mb_iters = 0, st->mb_rz0 = 0.f;
        if (st->converged) st->gn_noop += 1;  // (the finish kernel books the iteration itself)
    }
    float rz = 0.f;
    if (a < s.D) {
        const float minv = jacobi_inv(s.diag[a]);
        const float4 r   = make_float4(s.g[3 * a], s.g[3 * a + 1], s.g[3 * a + 2], 0.f);
        const float4 z   = make_float4(minv * r.x, minv * r.y, minv * r.z, 0.f);
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        s.mb_r[a] = r, s.mb_u[0][a] = z, s.mb_x[a] = zero;
        s.mb_p[a] = s.mb_s[a] = s.mb_t[0][a] = s.mb_t[1][a] = zero;  // (the one-launch form multiplies them by beta_0 = 0)
        rz = fmaf(r.z, z.z, fmaf(r.y, z.y, r.x * z.x));
    }
    rz = wave_sum_all(rz);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = rz;
    __syncthreads();
    if (threadIdx.x == 0) s.mb_gpart[0][blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- Chronopoulos-Gear form: ONE launch per iteration (the two inner products are taken together after the matrix
// product, so an iteration needs one grid-wide synchronisation; the textbook form needs two).  As in
// s6_pcg_step_kernel:  u = M^-1 r, w = A u, m = M^-1 w, t kept by t_i = m_i + beta_i t_(i-1);
//   p_i = u_i + beta_i p_(i-1);  s_i = w_i + beta_i s_(i-1);  x += alpha_i p_i;  r -= alpha_i s_i;  u_(i+1) = u_i - alpha_i t_i;
//   w_(i+1) = A u_(i+1) = A u_i - alpha_i (A m_i + beta_i A t_(i-1))  — gathered from the vectors of launch i - 1;
//   gamma = (r, u), delta = (w, u);  beta_(i+1) = gamma_(i+1) / gamma_i;  alpha_(i+1) = gamma_(i+1) / (delta_(i+1) - beta_(i+1) gamma_(i+1) / alpha_i).
// launch it = -1: w_0 = A u_0, m_0, gamma_0, delta_0 (u_0 = M^-1 g, x = 0 from pcg_mb_init_kernel).  16 lanes per row.
// Same iterates as the textbook form in exact arithmetic; the stopping rules are evaluated on gamma = (r, M^-1 r).
__global__ __launch_bounds__(256) void pcg_mb_step_kernel(SolveView s, SolveState* __restrict__ st, int it, float pcg_tol) {
    __shared__ float sh[2][4];
    const int nb  = solve_mb_blocks(s.D);
    const int cur = it >= 0 ? (it & 1) : 0, nxt = cur ^ 1;  // u, m: read [cur], write [nxt]; t: read [nxt], write [cur]
    const float4* ucur  = s.mb_u[cur];
    const float4* mcur  = s.mb_m[cur];
    const float4* tprev = s.mb_t[nxt];
    // The launch is a chain of dependent round trips and little else.  The row's length and each lane's FIRST matrix entry
    // depend on nothing but the launch arguments: they are requested here, with the stop flag and the partial inner products,
    // and their gathers go out before the scalars are summed — two rounds instead of three (scalars, then entries, then
    // gathers), also for the second entry of a lane (rows of 17-32 entries: every k = 8 row).  A launch that turns out to have nothing to do has loaded a few values in vain.
    const int lane16  = threadIdx.x & (MB_LPR - 1);
    const int a       = (blockIdx.x * 256 + threadIdx.x) / MB_LPR;
    const bool row_ok = a < s.D;
    const int cnt     = row_ok ? s.ell_cnt[a] : 0;
    const float2 e0   = row_ok ? s.ell[(size_t)lane16 * s.D + a] : make_float2(0.f, 0.f);  // (rows shorter than 16: not used)
    const float2 e1   = row_ok ? s.ell[(size_t)(lane16 + MB_LPR) * s.D + a] : make_float2(0.f, 0.f);  // (k = 8 rows have ~27 entries)
    if (st->mb_done) return;
    const bool has0 = lane16 < cnt, has1 = lane16 + MB_LPR < cnt;
    const int col0  = has0 ? __float_as_int(e0.y) : 0, col1 = has1 ? __float_as_int(e1.y) : 0;
    const float4 uu0 = ucur[col0], uu1 = ucur[col1];
    float4 mm0 = make_float4(0.f, 0.f, 0.f, 0.f), tt0 = mm0, mm1 = mm0, tt1 = mm0;
    if (it >= 0) mm0 = mcur[col0], tt0 = tprev[col0], mm1 = mcur[col1], tt1 = tprev[col1];
    float alpha = 0.f, beta = 0.f;
    if (it >= 0) {
        // the inner products of the launch before: every workgroup adds the partials in the same order
        float g = 0.f, d = 0.f;
        for (int i = threadIdx.x; i < nb; i += 256) g += s.mb_gpart[it & 1][i], d += s.mb_dpart[it & 1][i];
        g = wave_sum_all(g), d = wave_sum_all(d);
        if ((threadIdx.x & 63) == 0) sh[0][threadIdx.x >> 6] = g, sh[1][threadIdx.x >> 6] = d;
        __syncthreads();
        const float gamma = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]), delta = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
        float denom = delta;
        bool stop   = !(gamma > 0.f);
        if (it == 0) {
            // (the float constant as the at-floor level is this form's own: DESIGN_NOTES.md, "Open differences between the
            // PCG forms")
            const bool at_floor = pcg_at_floor(st, gamma, (double)1e-12f);
            stop                = stop || at_floor;  // nothing left to solve
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                st->mb_rz0 = gamma;
                if (at_floor) solve_mark_at_floor(st);
            }
        } else {
            beta  = cg_beta(false, gamma, st->mb_gamma_prev[(it + 1) & 1]);
            denom = cg_denom(false, gamma, delta, beta, st->mb_alpha_prev[(it + 1) & 1]);
            stop  = stop || gamma <= pcg_joint_target(st, pcg_tol, st->mb_rz0);
        }
        stop = stop || !(denom > 0.f);  // converged, or breakdown: the same decision in every workgroup
        if (stop) {
            if (blockIdx.x == 0 && threadIdx.x == 0) st->mb_done = 1;
            return;
        }
        alpha = gamma / denom;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->mb_gamma_prev[it & 1] = gamma, st->mb_alpha_prev[it & 1] = alpha;
            st->mb_iters += 1;
        }
    }
    float au[3] = {0.f, 0.f, 0.f}, am[3] = {0.f, 0.f, 0.f}, at[3] = {0.f, 0.f, 0.f};
    for (int q = lane16; q < cnt; q += MB_LPR) {
        const bool first = q == lane16, second = q == lane16 + MB_LPR;
        const float2 e   = first ? e0 : second ? e1 : s.ell[(size_t)q * s.D + a];
        const int col    = __float_as_int(e.y);
        const float val  = e.x;
        const float4 uu  = first ? uu0 : second ? uu1 : ucur[col];
        au[0] = fmaf(val, uu.x, au[0]), au[1] = fmaf(val, uu.y, au[1]), au[2] = fmaf(val, uu.z, au[2]);
        if (it >= 0) {
            const float4 mm = first ? mm0 : second ? mm1 : mcur[col], tt = first ? tt0 : second ? tt1 : tprev[col];
            am[0] = fmaf(val, mm.x, am[0]), am[1] = fmaf(val, mm.y, am[1]), am[2] = fmaf(val, mm.z, am[2]);
            at[0] = fmaf(val, tt.x, at[0]), at[1] = fmaf(val, tt.y, at[1]), at[2] = fmaf(val, tt.z, at[2]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) au[c] = group16_sum(au[c]), am[c] = group16_sum(am[c]), at[c] = group16_sum(at[c]);
    float gpart = 0.f, dpart = 0.f;
    if (row_ok && lane16 == 0) {
        const float minv = jacobi_inv(s.diag[a]);
        float4 u = ucur[a], r = s.mb_r[a];
        float w[3] = {au[0], au[1], au[2]};
        if (it >= 0) {
            const float4 m = mcur[a], tp = tprev[a], p = s.mb_p[a], sv = s.mb_s[a], wv = s.mb_w[a];
            float4 x = s.mb_x[a];
            const float4 tn = make_float4(fmaf(beta, tp.x, m.x), fmaf(beta, tp.y, m.y), fmaf(beta, tp.z, m.z), 0.f);
            const float4 pn = make_float4(fmaf(beta, p.x, u.x), fmaf(beta, p.y, u.y), fmaf(beta, p.z, u.z), 0.f);
            const float4 sn = make_float4(fmaf(beta, sv.x, wv.x), fmaf(beta, sv.y, wv.y), fmaf(beta, sv.z, wv.z), 0.f);
            u = make_float4(fmaf(-alpha, tn.x, u.x), fmaf(-alpha, tn.y, u.y), fmaf(-alpha, tn.z, u.z), 0.f);
            r = make_float4(fmaf(-alpha, sn.x, r.x), fmaf(-alpha, sn.y, r.y), fmaf(-alpha, sn.z, r.z), 0.f);
            x.x = fmaf(alpha, pn.x, x.x), x.y = fmaf(alpha, pn.y, x.y), x.z = fmaf(alpha, pn.z, x.z);
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] = au[c] - alpha * (am[c] + beta * at[c]);
            s.mb_t[cur][a] = tn, s.mb_p[a] = pn, s.mb_s[a] = sn, s.mb_x[a] = x, s.mb_r[a] = r, s.mb_u[nxt][a] = u;
        }
        s.mb_w[a]                     = make_float4(w[0], w[1], w[2], 0.f);
        s.mb_m[it >= 0 ? nxt : 0][a] = make_float4(minv * w[0], minv * w[1], minv * w[2], 0.f);
        gpart = fmaf(r.z, u.z, fmaf(r.y, u.y, r.x * u.x));
        dpart = fmaf(w[2], u.z, fmaf(w[1], u.y, w[0] * u.x));
    }
    gpart = wave_sum_all(gpart), dpart = wave_sum_all(dpart);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[0][threadIdx.x >> 6] = gpart, sh[1][threadIdx.x >> 6] = dpart;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int slot = it >= 0 ? ((it + 1) & 1) : 0;
        s.mb_gpart[slot][blockIdx.x] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        s.mb_dpart[slot][blockIdx.x] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    }
}

// t += delta and the counters the single-workgroup kernels keep
__global__ __launch_bounds__(256) void pcg_mb_finish_kernel(SolveView s, SolveState* __restrict__ st) {
    if (st->mb_skip) return;
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < s.D) {
        const float4 x = s.mb_x[a];
        s.t[3 * a] += x.x, s.t[3 * a + 1] += x.y, s.t[3 * a + 2] += x.z;
    }
    if (a == 0) pcg_book_launch(st, st->mb_rz0, st->mb_iters, false);  // (launch 0 has set the at-floor mark)
}

// The iteration count is only known on the device.  With a pinned host word the launches go out in chunks (16, 32,
// 64, ...) and the stop flag is read back between chunks — one stream synchronisation per chunk instead of up to
// max_iter launches that return at once (3 us each: 0.7 ms per Gauss-Newton iteration at the usual cap of 256).
void MbGraphCache::release() {
    for (int i = 0; i < used; ++i)
        if (e[i].exec) (void)hipGraphExecDestroy(e[i].exec);
    used = 0;
    if (capture) (void)hipStreamDestroy(capture), capture = nullptr;
}

// iterations [it0, it1): from the cache's graph of that range when there is (or can be) one, else launch by launch
static hipError_t launch_mb_range(const SolveView& s, SolveState* state, int it0, int it1, float pcg_tol,
                                  MbGraphCache* gc, hipStream_t st) {
    const int nb = solve_mb_blocks(s.D);
    auto direct = [&](hipStream_t q) {
        for (int it = it0; it < it1; ++it) pcg_mb_step_kernel<<<nb, 256, 0, q>>>(s, state, it, pcg_tol);
        return hipGetLastError();
    };
    if (!gc || gc->disabled || it1 - it0 < 4) return direct(st);
    MbGraphCache::Entry* hit = nullptr;
    for (int i = 0; i < gc->used && !hit; ++i) {
        MbGraphCache::Entry& c = gc->e[i];
        // (the plan's own buffers never move; the borrowed pointers of the view change from frame to frame but these
        // kernels read none of them)
        if (c.it0 == it0 && c.it1 == it1 && c.tol == pcg_tol && c.state == state && c.view.D == s.D && c.view.ell == s.ell)
            hit = &c;
    }
    if (!hit) {
        if (gc->used == (int)(sizeof(gc->e) / sizeof(gc->e[0]))) {  // other problem sizes / chunk sizes: start over
            for (int i = 0; i < gc->used; ++i)
                if (gc->e[i].exec) (void)hipGraphExecDestroy(gc->e[i].exec);
            gc->used = 0;
        }
        hipGraph_t g = nullptr;
        hipGraphExec_t exec = nullptr;
        bool ok = gc->capture || hipStreamCreateWithFlags(&gc->capture, hipStreamNonBlocking) == hipSuccess;
        ok      = ok && hipStreamBeginCapture(gc->capture, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            const hipError_t le = direct(gc->capture);
            const hipError_t ce = hipStreamEndCapture(gc->capture, &g);
            ok = le == hipSuccess && ce == hipSuccess && g && hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) == hipSuccess;
            if (g) (void)hipGraphDestroy(g);
        }
        if (!ok) {
            (void)hipGetLastError();  // clear the sticky error of the failed attempt
            gc->disabled = true;
            return direct(st);
        }
        hit        = &gc->e[gc->used++];
        hit->it0 = it0, hit->it1 = it1, hit->tol = pcg_tol, hit->view = s, hit->state = state, hit->exec = exec;
    }
    return hipGraphLaunch(hit->exec, st);
}

hipError_t launch_mb_pcg(const SolveView& s, SolveState* state, int max_iter, float pcg_tol, int* host_flag,
                         MbGraphCache* gc, hipStream_t st) {
    const int nb = solve_mb_blocks(s.D), nbu = (s.D + 255) / 256;
    pcg_mb_init_kernel<<<nbu, 256, 0, st>>>(s, state);
    pcg_mb_step_kernel<<<nb, 256, 0, st>>>(s, state, -1, pcg_tol);
    int chunk = 16;
    const int ci = gc ? std::min(gc->call++, 63) : 0;
    if (gc && host_flag && gc->pred[ci] > 0) chunk = std::max(8, (gc->pred[ci] + 4 + 7) & ~7);
    for (int it = 0; it < max_iter;) {
        const int end = host_flag ? std::min(max_iter, it + chunk) : max_iter;
        {
            const hipError_t e = launch_mb_range(s, state, it, end, pcg_tol, host_flag ? gc : nullptr, st);
            if (e != hipSuccess) return e;
            it = end;
        }
        if (host_flag && it < max_iter) {
            // step `it` first evaluates the stopping rule on the residual the chunk left, then iterates
            pcg_mb_step_kernel<<<nb, 256, 0, st>>>(s, state, it, pcg_tol);
            // mb_done, converged, mb_skip, mb_iters
            hipError_t e = hipMemcpyAsync(host_flag, &state->mb_done, 4 * sizeof(int), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
            if (gc) gc->pred[ci] = host_flag[3];  // (the total when the flag is set, a lower bound otherwise)
            if (*host_flag) break;
            ++it;
            chunk = 16;  // the prediction fell short: go on in small chunks
        }
    }
    pcg_mb_finish_kernel<<<nbu, 256, 0, st>>>(s, state);
    return hipGetLastError();
}

}  // namespace dfa
