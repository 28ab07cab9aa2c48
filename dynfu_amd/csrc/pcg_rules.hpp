// pcg_rules.hpp — what an iteration of the reference-mode block-Jacobi PCG IS, stated once: the preconditioner, the
// stopping rules, the Chronopoulos-Gear scalars, the row owner's vector update and the booking of a finished launch.
// The forms in solve_pcg.hip (register-resident, streaming), solve_pcg_launched.hip and solve_pcg_team.hip (team, guard) say only how they move the data and
// call these; the library is built with -ffp-contract=off, so an expression inlined from here is the arithmetic it
// spells (fmaf where it says fmaf, a product where it says a product).
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

#include "solve.hpp"

namespace dfa {

// Jacobi preconditioner: the inverse of a diagonal entry of the normal matrix (a node no row touches keeps M = 1)
__device__ __forceinline__ float jacobi_inv(float d) { return d > FLT_EPSILON ? 1.0f / d : 1.0f; }

// PCG targets never go below the round-off floor of the SOLVE: 1e-12 of the first linearisation's (r0, z0), the level
// at which a whole linearisation is skipped.  A late Gauss-Newton iteration starts from a small gradient, and 1e-12 of
// THAT is out of float's reach — its PCG would polish noise until the iteration cap (C2: the third iteration spent 108
// PCG iterations to move the translations by 2e-7 m).
constexpr double PCG_SOLVE_FLOOR = 1e-12;
__device__ __forceinline__ float solve_floor(const SolveState* st) { return (float)(PCG_SOLVE_FLOOR * st->grad_first); }

// Is the gradient of this linearisation — (r0, z0) of the joint system — at that floor already?  Then there is nothing
// to solve: the launch leaves t alone and marks the state (solve_mark_at_floor).  `floor_` is an argument because the
// launched form compares against the float constant (DESIGN_NOTES.md, "open differences between the PCG forms").
__device__ __forceinline__ bool pcg_at_floor(const SolveState* st, double rz0, double floor_ = PCG_SOLVE_FLOOR) {
    return st->grad_first > 0.0 && rz0 <= floor_ * st->grad_first;
}

// (r, z) at which the joint system counts as solved: pcg_tol^2 (not below float's squared-residual-ratio floor) of
// (r0, z0), never below the solve's floor.  A form that solves the coordinates apart gives each a third of it.
__device__ __forceinline__ float pcg_joint_target(const SolveState* st, float pcg_tol, float rz0) {
    const float floor_ = 1e-12f;
    const float tol2   = pcg_tol * pcg_tol > floor_ ? pcg_tol * pcg_tol : floor_;
    return fmaxf(tol2 * rz0, solve_floor(st));
}

// ---- Chronopoulos-Gear form (one reduction per iteration):  u = M^-1 r, w = A u, gamma = (r, u), delta = (w, u);
//   beta_i = gamma_i / gamma_(i-1);  alpha_i = gamma_i / (delta_i - beta_i gamma_i / alpha_(i-1));
//   p = u + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s
// and, where u is kept by recurrence instead of u = M^-1 r (m = M^-1 w):  t = m + beta t;  u -= alpha t.
// Same iterates as the textbook form in exact arithmetic; the stopping rule is evaluated on gamma = (r, M^-1 r) of the
// iterate in x.
// A form's loop reads:  stop if !(gamma > target) [converged];  beta, denom from here;  stop if !(denom > 0) [broke down];
// alpha = gamma / denom.  (The two tests stay in the loops: folded into one function here, the register-resident and the
// team kernel came out of the compiler with other spill counts — profiles/pcg_rules_refactor.md.)
__device__ __forceinline__ float cg_beta(bool first, float gamma, float gamma_old) { return first ? 0.f : gamma / gamma_old; }
__device__ __forceinline__ float cg_denom(bool first, float gamma, float delta, float beta, float alpha_old) {
    return first ? delta : delta - beta * gamma / alpha_old;
}

// the row owner's update, one row and one coordinate
__device__ __forceinline__ void cg_update_row(float alpha, float beta, float u, float w, float& p, float& s, float& x, float& r) {
    p = fmaf(beta, p, u), s = fmaf(beta, s, w);
    x = fmaf(alpha, p, x), r = fmaf(-alpha, s, r);
}
// ... and u by recurrence (the same arithmetic on the same numbers wherever a replica of u is kept)
__device__ __forceinline__ void cg_update_u(float alpha, float beta, float m, float& t, float& u) {
    t = fmaf(beta, t, m);
    u = fmaf(-alpha, t, u);
}

// ---- a finished launch goes into the solve's books: one Gauss-Newton iteration, its PCG iterations, the scale of the
// floor if this was the first linearisation, the at-floor mark.  By the one workgroup that ran it (one thread) ...
__device__ __forceinline__ void pcg_book_launch(SolveState* st, double rz0, int iters, bool at_floor) {
    if (st->grad_first == 0.0) st->grad_first = rz0;
    st->pcg_iters += iters;
    st->gn_iters += 1;
    if (at_floor) solve_mark_at_floor(st);
}
// ... or by the last to arrive of the three workgroups that solved a coordinate each (one thread of each calls this):
// iterations of the launch = those of its slowest coordinate; rz0 and at_floor are the same in all three
__device__ __forceinline__ void pcg_book_launch_of_three(SolveState* st, double rz0, int iters, bool at_floor) {
    atomicMax(&st->split_iters, iters);
    __threadfence();
    if (atomicAdd(&st->split_ticket, 1u) == 2u) {
        __threadfence();
        st->pcg_iters += atomicExch(&st->split_iters, 0);
        st->split_ticket = 0u;
        if (st->grad_first == 0.0) st->grad_first = rz0;
        st->gn_iters += 1;
        if (at_floor) solve_mark_at_floor(st);
    }
}

}  // namespace dfa
