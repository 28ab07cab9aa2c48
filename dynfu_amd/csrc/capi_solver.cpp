// capi_solver.cpp — C ABI (include/dynfu_amd.h), the reference-mode solver plan: its struct and field list, the per-frame
// launch sequence, the timing brackets and the stats.  What owns memory is in device_memory.hpp; the stages are
// solve_*.hip (solve.hpp).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "capi_internal.hpp"
#include "dev_switch.hpp"
#include "solve.hpp"

using namespace dfa::capi;

struct dfa_solver {
    int max_D, max_N, k;
    size_t max_R;
    int ell_cap;
    int asm_resident = 0;      // workgroups of the in-flight assembly the device holds at once (solve_assemble_resident_blocks)
    dfa::SolveView v;          // pointers into `mem`
    dfa::SolveState* state;    // device
    double* cost_partials;     // device
    unsigned int* ticket;      // device: arrival counter of the linearise kernel (self re-arming)
    dfa::PlanArena mem;         // every hipMalloc and pinned block of this plan
    GridScratch grid;           // node grid of the current problem
    bool has_problem;
    bool timing;
    dfa::EventPool ev;               // timing events, in begin / end pairs: they accumulate from enable_timing(1) on
    std::vector<int> ev_pcg, ev_asm; // indices of the begin events of each bracketed launch
    int timed_solves = 0;
    dfa::MbGraphCache mb_graphs;  // HIP graphs of the many-workgroup PCG's launch chunks
    dfa::TeamPcg team;            // host side of the team PCG (plans of 2 049 nodes up to solve_team_pcg_fits: 19 584;
                                  // rows longer than J x 20 entries make the first launch give up and the plan fall back)
    bool deterministic = false;  // order-stable variant (dfa_solver_set_deterministic), applied by the next set_problem
    bool just_reset = false;  // the unknowns and the state block were zeroed by set_problem and not touched since
    bool graph_rows = false;  // the last set_problem built graphs and rows with the fused launch (solve_build_graph_rows)
    long long* iters_total = nullptr;  // device: PCG iterations of all solves since enable_timing(1)
    dfa_overlap_fn overlap_fn = nullptr;  // called behind the first assembly launch of every solve
    void* overlap_user        = nullptr;
    int* host_flag = nullptr;        // pinned int[4]: stop flag of the many-workgroup PCG, the plan's converged flag, (skip), iterations;
                                     // read back between launch chunks
};

namespace {
// a begin / end pair of timing events: the begin event's index, recorded on st (-1: no events, the bracket is not taken)
int bracket_open(dfa_solver* s, hipStream_t st) {
    const int idx = s->timing ? s->ev.take(2) : -1;
    if (idx >= 0) (void)hipEventRecord(s->ev.events[idx], st);
    return idx;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------- solver seam

int dfa_solver_create(int max_D, int max_N, int k, dfa_solver** out) {
    REQUIRE(out, "null out");
    *out = nullptr;
    REQUIRE(max_D > 0 && max_N >= 0, "bad sizes");
    REQUIRE(k >= 1 && k <= DFA_MAX_KNN, "k out of range 1..16");
    REQUIRE(max_D <= dfa::solve_pcg_max_nodes(), "more nodes than a plan supports (32768)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DFA_ERR_NO_GPU, "no HIP device");
    dfa_solver* s = new (std::nothrow) dfa_solver();
    REQUIRE(s, "out of host memory");
    s->max_D = max_D, s->max_N = max_N, s->k = k;
    s->max_R       = (size_t)max_N + (size_t)max_D * k;
    s->ell_cap     = 256;
    s->asm_resident = dfa::solve_assemble_resident_blocks(k);
    s->has_problem = false;
    s->timing      = false;
    {
        // (the one environment variable of the product library, read once per plan: the order-stable assembly for a caller
        // that cannot reach dfa_solver_set_deterministic — include/dynfu_amd.h)
        const char* e    = getenv("DFA_ASSEMBLE_DETERMINISTIC");
        s->deterministic = e && atoi(e) != 0;
    }
    std::memset(&s->v, 0, sizeof(s->v));
    const size_t R = s->max_R, D = (size_t)max_D;
    dfa::PlanArena& mem = s->mem;
#define A(field, count) mem.alloc(&s->v.field, (count))
    A(ridx, R * k);
    A(rw, R * k);
    A(rtau, R);
    A(rb, R * 3);
    A(re, R * (size_t)dfa::solve_rec_words(k));
    A(reg_idx, D * k);
    A(blk_hist, D * (dfa::SOLVE_TG_BLOCKS + 1));
    A(node_ptr, D + 1);
    A(node_list, R * k);
    A(ell, D * s->ell_cap);
    A(ell_cnt, D);
    A(diag, D);
    A(g, D * 3);
    A(g_base, D * 3);
    A(t_base, D * 3);
    A(pk_perm, D);
    A(pk_perm2, D);
    A(pk_vals, D * s->ell_cap);
    A(pk_cols, D * s->ell_cap);
    A(mb_x, D);
    A(mb_r, D);
    A(mb_p, D);
    A(mb_s, D);
    A(mb_w, D);
    A(mb_u[0], D);
    A(mb_u[1], D);
    A(mb_m[0], D);
    A(mb_m[1], D);
    A(mb_t[0], D);
    A(mb_t[1], D);
    A(mb_gpart[0], (size_t)dfa::solve_mb_blocks(max_D));
    A(mb_gpart[1], (size_t)dfa::solve_mb_blocks(max_D));
    A(mb_dpart[0], (size_t)dfa::solve_mb_blocks(max_D));
    A(mb_dpart[1], (size_t)dfa::solve_mb_blocks(max_D));
    A(t, D * 3);
    A(huber, D);
    A(node_dq_out, D * 8);
#undef A
    int rc = plan_status(mem);
    if (rc == DFA_OK) rc = plan_grid(s->grid, max_D);
    // (plans of up to 2 048 nodes solve in the register-resident kernels: no team buffers for them outside development builds)
    if (rc == DFA_OK && dfa::solve_team_pcg_fits(max_D) && (max_D > 2048 || dfa::kDevAB)) {
        // team PCG: control block and flag words (zeroed once: barrier rounds grow; the words are cleared again only where
        // the rounds would wrap), exchange buffer, the pinned abort count
        s->v.team_stride = (max_D + 3) & ~3;
        const size_t areas = (size_t)3 * dfa::solve_team_pcg_rounds();  // an area per barrier round and coordinate (50 MB at 8 k nodes)
        mem.alloc(&s->v.team_ctl, 1, true);
        mem.alloc(&s->v.team_mt, areas * s->v.team_stride, true);
        mem.alloc(&s->v.team_words, dfa::solve_team_pcg_words(), true);
        s->team.host_abort = mem.pinned<int>(1);
        if ((rc = plan_status(mem)) == DFA_OK && !s->team.host_abort) rc = fail(DFA_ERR_HIP, "hipHostMalloc (team PCG abort count)");
        if (rc == DFA_OK) {
            s->team.ctl = s->v.team_ctl;
            // (development builds: DFA_MB_TEAM_EPOCH = the first barrier round, e.g. just below 2^32 for the wrap's test)
            if (const char* e0 = dfa::dev_env("DFA_MB_TEAM_EPOCH")) s->team.epoch = (unsigned)std::strtoul(e0, nullptr, 0);
        }
    }
    if (rc == DFA_OK) {
        mem.alloc(&s->state, 1);
        mem.alloc(&s->iters_total, 1, true);
        s->host_flag = mem.pinned<int>(4);  // (none: the solve does without the read-backs)
        // (per linearise workgroup, at most 1024 of them: its share of the energy; behind those its largest matrix addend,
        // as a double and once more as a float: solve_internal.hpp)
        mem.alloc(&s->cost_partials, dfa::solve_cost_partials_len());
        mem.alloc(&s->ticket, 64, true);
        rc = plan_status(mem);
    }
    if (rc != DFA_OK) {
        dfa_solver_destroy(s);
        return rc;
    }
    *out = s;
    return DFA_OK;
}

void dfa_solver_destroy(dfa_solver* s) {
    if (!s) return;
    s->grid.release();
    s->mb_graphs.release();
    delete s;  // (the arena frees the plan's memory, the pool its events)
}

int dfa_solver_set_problem(dfa_solver* s, const float* node_pos, const float* node_dq, const float* node_w, int D,
                           const float* canon_vertices, const float* canon_normals, const float* live_vertices,
                           const float* live_normals, int N, dfa_stream_t stream) {
    (void)canon_normals;
    (void)live_normals;  // declared by energy.t:28-31, never read by an Energy term
    REQUIRE(s, "null plan");
    REQUIRE(node_pos && node_dq && node_w && D > 0, "no nodes");
    REQUIRE(N >= 0 && (N == 0 || (canon_vertices && live_vertices)), "bad vertex arrays");
    if (D > s->max_D || N > s->max_N)
        return fail(DFA_ERR_CAPACITY, "dfa_solver_set_problem: D=%d N=%d exceed the plan (max_D=%d max_N=%d)", D, N,
                    s->max_D, s->max_N);
    dfa::SolveView& v = s->v;
    v.N = N, v.D = D, v.k = s->k, v.Dpad = (D + 3) & ~3, v.ell_cap = s->ell_cap;
    v.deterministic = s->deterministic ? 1 : 0;
    v.node_pos = node_pos, v.node_dq = node_dq, v.node_w = node_w;
    v.canon = canon_vertices, v.live = live_vertices;
    hipStream_t st = S(stream);
    // initializeDataGraph (opt_solver.cpp:56-72): rows [0, N) = k-NN of the canonical vertices + RBF weights
    const dfa::KnnGridView* grid = nullptr;
    // (development builds: DFA_GRAPH_GRID=1 puts the nodes of ANY problem in the grid — the tests of the fused graph build
    // reach its branches with a few dozen nodes)
    if (want_grid(D, (long)N + D) || dfa::dev_env_int("DFA_GRAPH_GRID", 0) != 0) {
        HIP_TRY(dfa::knn_grid_build(s->grid.v, node_pos, D, st));
        grid = &s->grid.v;
    }
    s->graph_rows = grid && dfa::solve_graph_rows_fits(v);
    if (s->graph_rows) {
        // both searches, the rows and the reset as one launch, then the transposition: the same bits as the sequence below
        HIP_TRY(dfa::solve_build_graph_rows(v, *grid, s->state, s->ticket, 64, st));
    } else {
        if (N > 0) HIP_TRY(dfa::launch_knn(node_pos, node_w, D, canon_vertices, N, s->k, v.ridx, v.rw, grid, st));
        // initializeRegGraph (:74-105): k-NN of every node among the nodes (itself included at distance 0)
        HIP_TRY(dfa::launch_knn(node_pos, node_w, D, node_pos, D, s->k, v.reg_idx, nullptr, grid, st));
        // rows + transposition; resetGPUMemory (:149-202): unknowns start at zero (same launch as the row set-up)
        HIP_TRY(dfa::solve_build_graph(v, s->state, s->ticket, 64, st));
    }
    s->has_problem = true;
    s->just_reset  = true;
    return DFA_OK;
}

int dfa_solver_set_deterministic(dfa_solver* s, int on) {
    REQUIRE(s, "null plan");
    s->deterministic = on != 0;
    return DFA_OK;
}

int dfa_solver_solve(dfa_solver* s, const dfa_solve_params* p, dfa_stream_t stream) {
    REQUIRE(s && p, "null plan / params");
    REQUIRE(s->has_problem, "set_problem has not been called");
    REQUIRE(p->num_iter >= 0 && p->nonlinear_iter >= 0 && p->linear_iter >= 0, "negative iteration count");
    REQUIRE(p->tukey_offset > 0.f && p->psi_data > 0.f, "tukey_offset / psi_data must be positive");
    REQUIRE(p->lambda >= 0.f && std::isfinite(p->lambda), "lambda must be non-negative and finite");
    const dfa::SolveView& v = s->v;
    hipStream_t st          = S(stream);
    if (!s->just_reset) HIP_TRY(dfa::solve_reset(v, s->state, s->ticket, 64, st));  // (set_problem has just done it)
    s->just_reset = false;
    // w_reg = sqrt(lambda / (D * KNN))  (opt_solver.cpp:30); rows carry tau = w_reg^2
    const double w_reg    = std::sqrt((double)p->lambda / ((double)v.D * (double)v.k));
    const float w_reg_f   = (float)w_reg;
    const float w_reg_sq  = w_reg_f * w_reg_f;
    if (s->timing) s->timed_solves += 1;
    if (s->host_flag) s->host_flag[0] = s->host_flag[1] = 0;
    s->mb_graphs.call = 0;
    int not_launched = 0;  // iterations after the host has seen the converged flag (many-workgroup path only)
    int gn_launched = 0;  // Gauss-Newton iterations whose assembly has been enqueued
    bool huber_done = false;
    const bool big_budget = (long)p->num_iter * p->nonlinear_iter > 8;
    const bool pcg_async  = dfa::solve_pcg_is_async(v, &s->team, p->linear_iter);  // (else the PCG itself reads the flags back)
    const bool no_regradient = dfa::dev_env("DFA_NO_REGRADIENT") != nullptr;  // (development builds: the tests compare both ways)
    // Behind the launch that left this iteration's system (the assembly, or the regradient that stands in for one) in the
    // bracket ev_asm: this iteration's PCG starts here — the caller's chip-wide work may run in its shadow
    auto run_pcg = [&](int ev_asm) -> int {
        if (ev_asm >= 0) {  // close that bracket and book it
            (void)hipEventRecord(s->ev.events[ev_asm + 1], st);
            s->ev_asm.push_back(ev_asm);
        }
        if (s->overlap_fn) s->overlap_fn(s->overlap_user, stream, gn_launched);
        ++gn_launched;
        const int ev = bracket_open(s, st);  // closed behind the solving kernel, before the fallback launch
        HIP_TRY(dfa::solve_pcg(v, s->state, p->linear_iter, p->pcg_tol, s->host_flag, &s->mb_graphs, &s->team,
                               ev >= 0 ? s->ev.events[ev + 1] : nullptr, st));
        if (ev >= 0) s->ev_pcg.push_back(ev);
        return DFA_OK;
    };
    for (int outer = 0; outer < p->num_iter; ++outer) {
        // preNonlinearSolve (opt_solver.cpp:135-140): the Huber weights are only observable after
        // the solve, so they are evaluated for the last outer iteration alone
        // (folded into that iteration's first linearisation; a launch of its own only if that one is never enqueued)
        // converged == 2 (gradient at the floor under stale weights) ended the inner iterations of the outer iteration
        // before only: this one re-weights, and its first linearisation clears the flag on the device
        if (s->host_flag && s->host_flag[1] == 2) s->host_flag[1] = 0;
        int gn_in_outer = 0;  // iterations of this outer iteration enqueued (the device's flag is current behind them)
        for (int gn = 0; gn < p->nonlinear_iter; ++gn) {
            // Iteration budgets like the reference's (24 x 16, dyn_fusion.cpp:183-189) are ~380 iterations of which a
            // handful do anything: behind a converged one the kernels return at entry, but 4 launches x 5 us x 380 is
            // still 8 ms of stream time.  Small budgets (<= 8 iterations: bench.py's 5) stay free of any host
            // synchronisation; larger ones read the `converged` flag back every 4th iteration (plans whose PCG does not
            // synchronise by itself: the register-resident kernels and the team form).
            if (big_budget && gn_in_outer >= 4 && gn_in_outer % 4 == 0 && s->host_flag && !s->host_flag[1] && pcg_async) {
                HIP_TRY(hipMemcpyAsync(&s->host_flag[1], &s->state->converged, sizeof(int), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            if (s->host_flag && s->host_flag[1]) {  // t can no longer change (in this outer iteration, when the flag is
                ++not_launched;                     // 2): every further iteration is a no-op
                continue;
            }
            ++gn_in_outer;
            // An inner iteration (frozen robust weights: linear least squares) restarts the PCG on the true residual of
            // the SAME matrix, g = g_base - A (t - t_base): one sparse product instead of a linearisation and an assembly
            // (the reference's budget is 16 inner iterations per re-weighting).  With a cost-decrease tolerance the cost
            // of every iteration is wanted: the long way.  Without the regulariser (lambda = 0: the reference's OptTests,
            // fewer vertices than nodes) the matrix is singular, and the cancellation in g_base - A (t - t_base) leaves
            // round-off in its null space, which CG then amplifies (a re-linearised gradient is J^T of something and has
            // none; measured: two of the eight OptTest scenes leave their 1e-3 tolerance): the long way as well.
            // DFA_NO_REGRADIENT=1: the long way always (A/B).
            if (gn > 0 && p->gn_tol == 0.f && p->lambda > 0.f && !no_regradient) {
                const int ev = bracket_open(s, st);  // booked with the assemblies: it stands in for one
                HIP_TRY(dfa::solve_regradient(v, s->state, st));
                if (int rc = run_pcg(ev)) return rc;
                continue;
            }
            const bool with_huber = gn == 0 && outer == p->num_iter - 1;
            // the re-weighting linearisation ends with its rows; the assembly launch forms amax and books the cost, so the
            // assembly's timing bracket contains that booking and the state block is complete behind the assembly, which
            // is where dfa_solver_get_stats reads it.  DFA_LIN_HANDOFF=0 (development builds): the linearisation's own tail.
            const bool handoff = dfa::solve_lin_handoff(gn == 0, gn == 0 ? 0 : 1, p->gn_tol) && dfa::dev_env_int("DFA_LIN_HANDOFF", 1) != 0;
            HIP_TRY(dfa::solve_linearise(v, s->state, s->cost_partials, s->ticket, gn == 0, gn == 0 ? 0 : 1, p->gn_tol,
                                         p->tukey_offset, p->psi_data, w_reg_sq, with_huber ? p->psi_reg : 0.f, nullptr, handoff, st));
            huber_done |= with_huber;
            const int ev = bracket_open(s, st);
            HIP_TRY(dfa::solve_assemble(v, s->state, gn == 0 && p->nonlinear_iter > 1, w_reg_sq, s->asm_resident,
                                        handoff ? s->cost_partials : nullptr, st));
            if (int rc = run_pcg(ev)) return rc;
        }
    }
    if (s->overlap_fn && gn_launched == 0) s->overlap_fn(s->overlap_user, stream, -1);  // no iteration ran: the caller's work still goes out
    if (not_launched) HIP_TRY(dfa::solve_count_noop(s->state, not_launched, st));
    // final cost at the solved t; weights re-evaluated only if no iteration ever did
    const bool no_weights = p->num_iter == 0 || p->nonlinear_iter == 0;
    if (!huber_done) HIP_TRY(dfa::solve_huber(v, p->psi_reg, st));  // no outer iteration, or the host stopped launching before the last
    HIP_TRY(dfa::solve_linearise(v, s->state, s->cost_partials, s->ticket, no_weights ? 1 : 0, 2, 0.f,
                                 p->tukey_offset, p->psi_data, w_reg_sq, 0.f, s->timing ? s->iters_total : nullptr, false, st));
    // (postSingleSolve -> copyResultToCPUFromFloat3, opt_solver.cpp:133,270-285: composed once, by that same launch)
    return DFA_OK;
}

int dfa_solver_set_overlap_callback(dfa_solver* s, dfa_overlap_fn fn, void* user) {
    REQUIRE(s, "null plan");
    s->overlap_fn = fn, s->overlap_user = user;
    return DFA_OK;
}

const float* dfa_solver_translations(const dfa_solver* s) { return s ? s->v.t : nullptr; }
const float* dfa_solver_node_dq(const dfa_solver* s) { return s ? s->v.node_dq_out : nullptr; }
const float* dfa_solver_tukey_weights(const dfa_solver* s) { return s ? s->v.rtau : nullptr; }
const float* dfa_solver_huber_weights(const dfa_solver* s) { return s ? s->v.huber : nullptr; }
const int32_t* dfa_solver_data_graph(const dfa_solver* s) { return s ? s->v.ridx : nullptr; }
const int32_t* dfa_solver_reg_graph(const dfa_solver* s) { return s ? s->v.reg_idx : nullptr; }
const float* dfa_solver_matrix_entries(const dfa_solver* s) { return s ? (const float*)s->v.ell : nullptr; }
const int32_t* dfa_solver_matrix_row_lengths(const dfa_solver* s) { return s ? s->v.ell_cnt : nullptr; }
const float* dfa_solver_gradient(const dfa_solver* s) { return s ? s->v.g : nullptr; }

int dfa_solver_warp_to_live(dfa_solver* s, const float* normals, float* out_vertices, float* out_normals,
                            dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(out_vertices || s->v.N == 0, "null output");
    HIP_TRY(dfa::launch_warp_graph(s->v.node_pos, s->v.node_dq_out, s->v.node_w, s->k, s->v.ridx, s->v.canon, normals,
                                   s->v.N, out_vertices, out_normals, S(stream)));
    return DFA_OK;
}

int dfa_solver_get_stats(dfa_solver* s, dfa_solve_stats* host_out, dfa_stream_t stream) {
    REQUIRE(s && host_out, "null plan / out");
    dfa::SolveState h;
    HIP_TRY(hipMemcpyAsync(&h, s->state, sizeof(h), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    host_out->initial_cost = h.initial_cost;
    host_out->final_cost   = h.final_cost;
    host_out->gn_iters     = h.gn_iters;
    host_out->pcg_iters    = h.pcg_iters;
    host_out->max_row_nnz  = h.max_row_nnz;
    host_out->gn_noop      = h.gn_noop;
    if (dfa::dev_env("DFA_PCG_PROFILE_PRINT")) {
        fprintf(stderr, "pcg phase cycles: spmv %lld  red_pAp %lld  update %lld  red_rz %lld  p_update+barrier %lld  loop %lld  (iters %d)\n",
                h.prof[0], h.prof[1], h.prof[2], h.prof[3], h.prof[4], h.prof[5], h.pcg_iters);
        fprintf(stderr, "assemble block 7 cycles: init %lld  list+hash %lld  reduce+barrier %lld  compact %lld   (raw prof[6] %lld prof[7] %lld)\n",
                h.prof[6] / 1000000, h.prof[6] % 1000000, h.prof[7] / 1000000, h.prof[7] % 1000000, h.prof[6], h.prof[7]);
    }
    if (h.overflow)
        return fail(DFA_ERR_CAPACITY, "normal-matrix row wider than the plan's ELL capacity (%d > %d)", h.max_row_nnz,
                    s->ell_cap);
    return DFA_OK;
}

int dfa_solver_enable_timing(dfa_solver* s, int enable) {
    REQUIRE(s, "null plan");
    s->timing = enable != 0;
    if (enable == 1) {  // a new measurement: forget the brackets collected so far (2 = resume, keeps them)
        s->ev.rewind(), s->timed_solves = 0;
        s->ev_pcg.clear(), s->ev_asm.clear();
        if (s->iters_total) HIP_TRY(hipMemset(s->iters_total, 0, sizeof(long long)));
    }
    return DFA_OK;
}

int dfa_solver_team_pcg_info(dfa_solver* s, int* launches, int* aborts, int* disabled) {
    REQUIRE(s, "null plan");
    if (launches) *launches = (int)std::min<long>(s->team.launches, 0x7fffffffL);
    if (aborts) *aborts = s->team.host_abort ? *(volatile int*)s->team.host_abort : 0;
    if (disabled) *disabled = (!s->team.ctl || s->team.disabled) ? 1 : 0;
    return DFA_OK;
}

int dfa_solver_get_timing(dfa_solver* s, dfa_solve_timing* out, dfa_stream_t stream) {
    REQUIRE(s && out, "null plan / out");
    HIP_TRY(hipStreamSynchronize(S(stream)));
    std::memset(out, 0, sizeof(*out));
    for (const std::vector<int>* brackets : {&s->ev_pcg, &s->ev_asm})
        for (int idx : *brackets) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, s->ev.events[idx], s->ev.events[idx + 1]));
            (brackets == &s->ev_pcg ? out->pcg_ms : out->assemble_ms) += ms;
        }
    out->pcg_launches      = (int)s->ev_pcg.size();
    out->assemble_launches = (int)s->ev_asm.size();
    out->solves            = s->timed_solves;
    if (s->iters_total) HIP_TRY(hipMemcpy(&out->pcg_iters, s->iters_total, sizeof(long long), hipMemcpyDeviceToHost));
    if (s->has_problem && s->v.D > 0)
        HIP_TRY_AS(row_count_sum(s->v.ell_cnt, s->v.D, &out->matrix_nnz),
                   "hipMemcpy(cnt.data(), s->v.ell_cnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost)");
    return DFA_OK;
}

}  // extern "C"

#ifdef DFA_DEV_AB  // development flavour only: the plan's graph-build outputs, for the tests that compare the two launch sequences
// out[0..10] = ridx, rw, rb, re, reg_idx, node_ptr, node_list, t, state block, tickets, (size_t) bytes of the state block;
// returns 1 if the last set_problem took the fused graph build
extern "C" __attribute__((visibility("default"))) int dfa_dev_solver_graph_ptrs(dfa_solver* s, void** out) {
    const dfa::SolveView& v = s->v;
    void* p[] = {v.ridx, v.rw, v.rb, v.re, v.reg_idx, v.node_ptr, v.node_list, v.t, s->state, s->ticket, (void*)sizeof(dfa::SolveState)};
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i) out[i] = p[i];
    return s->graph_rows ? 1 : 0;
}
#endif
