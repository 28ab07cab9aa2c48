// solve6_pcg.hip — the block-Jacobi preconditioned CG of the north-star solve on the block rows the assembly left
// (solve6_assemble.hip, which also sets x = 0, r = g, u = M^-1 g): ONE launch per iteration, one wave per block row,
// replayed by the C ABI as a HIP graph.
#include <hip/hip_runtime.h>

#include "solve6.hpp"
#include "solve6_internal.hpp"

namespace dfa {

namespace {

// -------------------------------------------------------------------------------------- PCG
// Chronopoulos-Gear form of preconditioned CG: the two inner products of an iteration are taken
// together after the matrix product, so an iteration needs ONE grid-wide synchronisation — one
// kernel launch (the textbook form needs two: 22 us per iteration at 4 k nodes, launch-bound).
//   u = M^-1 r, w = A u, m = M^-1 w, t = M^-1 s (kept by the recurrence t_i = m_i + beta_i t_{i-1})
//   p_i = u_i + beta_i p_{i-1};  s_i = w_i + beta_i s_{i-1};  x += alpha_i p_i;  r -= alpha_i s_i
//   u_{i+1} = u_i - alpha_i t_i;  w_{i+1} = A u_{i+1};  gamma = (r, u), delta = (w, u)
//   beta_{i+1} = gamma_{i+1} / gamma_i;  alpha_{i+1} = gamma_{i+1} / (delta_{i+1} - beta_{i+1} gamma_{i+1} / alpha_i)
// The matrix product of launch i needs u_{i+1} of OTHER nodes, which their waves are only computing in
// the same launch: the gather rebuilds it from u_i, m_i, t_{i-1} and the two scalars (18 floats per
// neighbour block next to the block's own 36).  Same iterates as textbook PCG in exact arithmetic.
// launch `it` = -1: w_0 = A u_0, m_0, gamma_0, delta_0.   launch it >= 0: iteration `it` as above.
constexpr int S6_PCG_WAVES = 5;  // waves per SIMD the register allocation aims at
__global__ __launch_bounds__(64 * S6_NODES_PER_BLOCK, S6_PCG_WAVES) void s6_pcg_step_kernel(Solve6View s, Solve6State* st, int it) {
    __shared__ float stage[S6_NODES_PER_BLOCK][3][64];
    __shared__ float gd_sh[S6_NODES_PER_BLOCK][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a    = blockIdx.x * S6_NODES_PER_BLOCK + wave;
    const int cur = it >= 0 ? (it & 1) : 0, nxt = cur ^ 1;  // u, m: read [cur], write [nxt]; t: read [nxt], write [cur]
    const float* ucur  = s.u[cur];
    const float* mcur  = s.m[cur];
    const float* tprev = s.t[nxt];
    // The kernel is a chain of dependent memory round trips (~2 us each) and little else, so it is
    // written as two rounds of loads: (1) everything addressable from the launch arguments — the
    // stop flag, the partial inner products and scalars of the previous launch, this row's columns,
    // its M^-1 and its own vector entries — and (2) the gathers through the columns.  The three
    // products A u, A m, A t are gathered separately and w = A u - alpha (A m + beta A t) is formed at
    // the end, so round (2) does not wait for the scalars either.
    constexpr int MAXIT = 5;  // 10 slots per pass, plan capacity 48
    // The partial inner products of the previous launch (one pair per workgroup) are read ONCE per workgroup — thread t takes
    // partials t, t + 512, ... —, added over the wave, and the eight waves' sums go through LDS: the same value, in the same
    // order, in every wave of every workgroup.  (Every wave used to read all of them: 2 x 16 registers per lane, which kept
    // the kernel at 92 VGPRs — two of these 512-thread workgroups per CU.)
    constexpr int MAXP  = 4;  // partials per thread held in registers: 512 x 4 = 2048 workgroups = 16 384 nodes (more: a loop)
    constexpr int NT    = 64 * S6_NODES_PER_BLOCK;
    const int nb   = s6_matvec_blocks(s.D);
    const int done = st->pcg_done;
    float gp[MAXP], dp[MAXP];
    float gamma_prev = 1.f, alpha_prev = 1.f, rz0 = 0.f;
    float tol2 = st->tol2;
    if (it >= 0) {
#pragma unroll
        for (int q = 0; q < MAXP; ++q) {
            const int i = (int)threadIdx.x + NT * q;
            gp[q] = i < nb ? s.g_part[it & 1][i] : 0.f;
            dp[q] = i < nb ? s.d_part[it & 1][i] : 0.f;
        }
        for (int i = (int)threadIdx.x + NT * MAXP; i < nb; i += NT) gp[MAXP - 1] += s.g_part[it & 1][i], dp[MAXP - 1] += s.d_part[it & 1][i];
        if (it > 0) gamma_prev = st->gamma_prev[(it + 1) & 1], alpha_prev = st->alpha_prev[(it + 1) & 1], rz0 = st->rz0;
    }
    const int ss = lane / 6, c = lane - 6 * ss;
    int cols[MAXIT];
#pragma unroll
    for (int q = 0; q < MAXIT; ++q) {
        const int sl = ss + 10 * q;
        cols[q]      = (a < s.D && lane < 60 && sl < s.cap) ? s.bcols[(size_t)a * s.cap + sl] : -1;
    }
    float minv_row[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, own_u = 0.f, own_m = 0.f, own_t = 0.f, own_p = 0.f, own_s = 0.f,
          own_w = 0.f, own_r = 0.f, own_x = 0.f;
    if (a < s.D && lane < 6) {
        const size_t i = 6 * (size_t)a + lane;
#pragma unroll
        for (int d = 0; d < 6; ++d) minv_row[d] = s.minv[36 * (size_t)a + 6 * lane + d];
        own_u = ucur[i], own_r = s.r[i];
        if (it >= 0) own_m = mcur[i], own_t = tprev[i], own_p = s.p[i], own_s = s.s[i], own_w = s.w[i], own_x = s.x[i];
    }
    if (done) return;  // (uniform)
    // (the partials arrive with the first round of loads, before the columns the gathers need anyway)
    __shared__ float gd_wave[S6_NODES_PER_BLOCK][2];
    if (it >= 0) {
        float gsum = 0.f, dsum = 0.f;
#pragma unroll
        for (int q = 0; q < MAXP; ++q) gsum += gp[q], dsum += dp[q];
        gsum = wave_sum_all(gsum), dsum = wave_sum_all(dsum);
        if (lane == 0) gd_wave[wave][0] = gsum, gd_wave[wave][1] = dsum;
    }
    float au = 0.f, am = 0.f, at = 0.f;
#pragma unroll
    for (int q = 0; q < MAXIT; ++q) {
        if (cols[q] < 0) continue;
        const float2* H  = reinterpret_cast<const float2*>(s.bvals + ((size_t)a * s.cap + ss + 10 * q) * 36 + 6 * c);
        const size_t cb  = 6 * (size_t)cols[q];
        const float2* pu = reinterpret_cast<const float2*>(ucur + cb);
        const float2* pm = reinterpret_cast<const float2*>(mcur + cb);
        const float2* pt = reinterpret_cast<const float2*>(tprev + cb);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float2 h = H[d], uu = pu[d];
            au += h.x * uu.x, au += h.y * uu.y;
            if (it >= 0) {
                const float2 mm = pm[d], tt = pt[d];
                am += h.x * mm.x, am += h.y * mm.y;
                at += h.x * tt.x, at += h.y * tt.y;
            }
        }
    }
    // scalars of this iteration
    float alpha = 0.f, beta = 0.f;
    if (it >= 0) {
        __syncthreads();  // (uniform: `it` and `done` are the same everywhere)
        float gamma = 0.f, delta = 0.f;
#pragma unroll
        for (int w = 0; w < S6_NODES_PER_BLOCK; ++w) gamma += gd_wave[w][0], delta += gd_wave[w][1];
        float denom = delta;
        if (it > 0) {
            beta = gamma / gamma_prev;
            denom -= beta * gamma / alpha_prev;
        } else {
            rz0 = gamma;
            // Eisenstat-Walker forcing term (choice 2, alpha = 2): the tolerance of this PCG from the gradients of this and
            // of the previous linearisation — the same value in every workgroup; one thread records it for the launches
            // that follow
            const int slot   = st->ew_slot & 1;
            const float prev = st->rz0_gn[slot ^ 1];
            const float eg   = st->ew_gamma;
            if (eg > 0.f && prev > 0.f) {
                const float eta = eg * gamma / prev;
                tol2            = fminf(fmaxf(eta * eta, st->ew_min2), st->ew_max2);
            }
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                st->rz0_gn[slot] = gamma;
                if (eg > 0.f && prev > 0.f) {
                    st->tol2 = tol2;
                    const int h = st->cur;
                    if (h >= 0 && h < S6_HIST) st->pcg_tol_hist[h] = sqrtf(tol2);
                }
            }
        }
        // p^T H p, which the recurrence carries as denom, is positive in exact arithmetic; on an ill-conditioned system
        // (lambda = 0: the nearly free sliding modes) the float32 recurrence can drive it to <= 0 long before the
        // tolerance.  Such a PCG used to stop there (at T0 / C2 / C3 with lambda = 0 at a relative residual of 4e-3 to 3e-2,
        // asked for 1e-4); it now restarts its directions from the current residual: beta = 0, denominator (w, u) = u^T H u.
        if (gamma > tol2 * rz0 && !(denom > 0.f)) beta = 0.f, denom = delta;
        // converged, or breakdown: the same decision in every workgroup
        if (!(gamma > 0.f) || gamma <= tol2 * rz0 || !(denom > 0.f)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                st->pcg_done = 1;
                const int h = st->cur;
                if (h >= 0 && h < S6_HIST) st->pcg_rel_hist[h] = gamma > 0.f && rz0 > 0.f ? sqrtf(gamma / rz0) : 0.f;
            }
            return;
        }
        alpha = gamma / denom;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->gamma_prev[it & 1] = gamma, st->alpha_prev[it & 1] = alpha;
            if (it == 0) st->rz0 = gamma;
            st->pcg_iters += 1;
            st->pcg_last_it = it + 1;
            const int h = st->cur;
            if (h >= 0 && h < S6_HIST) st->pcg_it_hist[h] = it + 1;
        }
    }
    stage[wave][0][lane] = au, stage[wave][1][lane] = am, stage[wave][2][lane] = at;
    __syncthreads();
    float gpart = 0.f, dpart = 0.f;
    if (a < s.D) {
        float wn = 0.f;
        if (lane < 6) {
            float su = 0.f, sm = 0.f, stt = 0.f;
#pragma unroll
            for (int q = 0; q < 10; ++q)
                su += stage[wave][0][q * 6 + lane], sm += stage[wave][1][q * 6 + lane], stt += stage[wave][2][q * 6 + lane];
            wn = it >= 0 ? su - alpha * (sm + beta * stt) : su;
        }
        // m_new = M^-1 w_new needs the six components held by lanes 0..5
        float mn = 0.f;
#pragma unroll
        for (int d = 0; d < 6; ++d) mn += minv_row[d] * __shfl(wn, d, 64);
        if (lane < 6) {
            const size_t i = 6 * (size_t)a + lane;
            float un = own_u, rn = own_r;
            if (it >= 0) {
                const float tn = own_m + beta * own_t;
                const float pn = own_u + beta * own_p;
                const float sn = own_w + beta * own_s;
                un = own_u - alpha * tn;
                rn = own_r - alpha * sn;
                s.t[cur][i] = tn, s.p[i] = pn, s.s[i] = sn;
                s.x[i] = own_x + alpha * pn;
                s.r[i] = rn;
                s.u[nxt][i] = un;
            }
            s.w[i] = wn;
            s.m[it >= 0 ? nxt : 0][i] = mn;
            gpart = rn * un, dpart = wn * un;
        }
    }
    gpart = wave_sum_all(gpart), dpart = wave_sum_all(dpart);
    if (lane == 0) gd_sh[wave][0] = gpart, gd_sh[wave][1] = dpart;
    __syncthreads();
    if (threadIdx.x == 0) {
        float g = 0.f, d = 0.f;
        for (int w = 0; w < S6_NODES_PER_BLOCK; ++w) g += gd_sh[w][0], d += gd_sh[w][1];
        const int slot = it >= 0 ? ((it + 1) & 1) : 0;
        s.g_part[slot][blockIdx.x] = g, s.d_part[slot][blockIdx.x] = d;
    }
}

}  // namespace

hipError_t s6_pcg(const Solve6View& s, Solve6State* state, const Solve6Params& p, hipStream_t st) {
    const int mb = s6_matvec_blocks(s.D);
    // launch -1 forms w_0 = A u_0; launch it >= 0 is iteration it (x_{it+1} is complete when it returns); the stop test
    // reads the tolerance of this Gauss-Newton iteration from the state block (set by the assembly launch)
    for (int it = -1; it < p.linear_iter; ++it) s6_pcg_step_kernel<<<mb, 64 * S6_NODES_PER_BLOCK, 0, st>>>(s, state, it);
    return hipGetLastError();
}

hipError_t s6_pcg_n(const Solve6View& s, Solve6State* state, int launches, hipStream_t st) {
    Solve6Params p{};
    p.linear_iter = launches;
    return s6_pcg(s, state, p, st);
}

}  // namespace dfa
