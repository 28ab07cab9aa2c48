// capi_solver6.cpp — C ABI (include/dynfu_amd.h), the north-star (6-DoF) solver plan: its struct and field list, the
// per-frame launch sequence with its captured PCG graphs, the timing marks and the stats.  What owns memory is in
// device_memory.hpp, the launch budget in launch_budget.hpp; the stages are solve6_*.hip (solve6.hpp).
#include <cstring>
#include <map>
#include <new>

#include "capi_internal.hpp"
#include "launch_budget.hpp"
#include "solve.hpp"  // SOLVE_TG_BLOCKS (blk_hist: solve_transpose_graph builds the node lists)
#include "solve6.hpp"

using namespace dfa::capi;

struct dfa_solver6 {
    int max_D, max_N, k;
    dfa::Solve6View v;
    dfa::Solve6State* state;
    float* raw_w;       // N x k un-normalised weights of the k-NN pass
    int32_t* raw_reg;   // D x (k + 1)
    const float* node_dq;  // borrowed: transforms at set_problem time
    dfa::PlanArena mem;
    GridScratch grid;
    bool has_problem;
    // the PCG of one Gauss-Newton iteration (linear_iter + 2 dependent launches) captured as a HIP graph:
    // re-captured when the problem size or the iteration parameters change
    std::map<int, hipGraphExec_t> pcg_graphs;  // by the number of step launches
    int last_launches = 0;  // step launches enqueued by the last solve
    dfa::LaunchBudget budget;                  // dfa_solve6_params.adaptive_launch (launch_budget.hpp)
    int* mirror = nullptr;                     // pinned int[S6_RING][S6_HIST]: the device's counts, solve n in slot n % S6_RING
    hipEvent_t done_ev[dfa::S6_RING] = {};     // end of solve n, n % S6_RING
    bool graph_disabled = false;
    hipStream_t capture_stream = nullptr;  // capture is not allowed on the legacy default stream
    bool timing = false;  // hipEvent brackets around linearise / assemble / PCG of every Gauss-Newton iteration
    dfa::EventPool ev;  // 4 per Gauss-Newton iteration
    int pcg_key_D = -1;  // node count the captured PCG graphs were recorded for
    // dfa_solver6_set_vertex_mask: the plan's copy of the caller's mask in its sorted order (max_N bytes, allocated on first
    // use); has_mask: the linearisations read it
    uint8_t* vmask = nullptr;
    bool has_mask  = false;
    // dfa_solver6_set_reg_hierarchy: the configuration and its buffers (max_D levels, a table for S6_REG_LEVELS levels,
    // allocated by the first call that asks for a hierarchy); hierarchical: the set_problem calls that follow build it
    dfa::S6RegHierarchy hier{};
    bool hierarchical = false;
    bool graph_levels = false;  // the graph of the last set_problem is a hierarchy: hier.level holds its D levels
};

namespace {
// The PCG launches of one Gauss-Newton iteration are replayed as a HIP graph (one per launch count): the graph of `launches`
// step launches, captured the first time it is asked for.  Null once capture has been given up (it is never possible on some
// stream configurations): the launches are then issued one by one.
hipGraphExec_t pcg_graph(dfa_solver6* s, int launches) {
    if (s->graph_disabled) return nullptr;
    const auto it = s->pcg_graphs.find(launches);
    if (it != s->pcg_graphs.end()) return it->second;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    bool ok = s->capture_stream || hipStreamCreateWithFlags(&s->capture_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipStreamBeginCapture(s->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        const hipError_t le = dfa::s6_pcg_n(s->v, s->state, launches, s->capture_stream);
        const hipError_t ce = hipStreamEndCapture(s->capture_stream, &g);
        ok = le == hipSuccess && ce == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
    }
    if (ok) {
        s->pcg_graphs.emplace(launches, ge);
        return ge;
    }
    (void)hipGetLastError();  // clear the sticky error of the failed attempt
    s->graph_disabled = true;
    return nullptr;
}
}  // namespace

extern "C" {

// -------------------------------------------------------------------- north-star solver seam

int dfa_solver6_create(int max_D, int max_N, int k, dfa_solver6** out) {
    REQUIRE(out, "null out");
    *out = nullptr;
    REQUIRE(max_D > 0 && max_N >= 0, "bad sizes");
    REQUIRE(k >= 1 && k <= 8, "k out of range 1..8");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(DFA_ERR_NO_GPU, "no HIP device");
    dfa_solver6* s = new (std::nothrow) dfa_solver6();
    REQUIRE(s, "out of host memory");
    s->max_D = max_D, s->max_N = max_N, s->k = k, s->has_problem = false, s->node_dq = nullptr;
    std::memset(&s->v, 0, sizeof(s->v));
    s->v.cap = DFA_SOLVE6_ROW_BLOCKS;  // = S6_MAXSLOT of solve6_internal.hpp
    const size_t N = (size_t)max_N, D = (size_t)max_D, cap = (size_t)s->v.cap;
    dfa::PlanArena& mem = s->mem;
#define A(field, count) mem.alloc(&s->v.field, (count))
    A(idx, N * k);
    A(wn, N * k);
    A(idx_nat, N * k);
    A(near, N);
    A(vptr, D + 1);
    A(vlist, N);
    A(vperm, N);
    A(canon_own, N * 3);
    A(canon_n_own, N * 3);
    A(reg_idx, D * k);
    A(blk_hist, D * (dfa::SOLVE_TG_BLOCKS + 1));
    A(node_ptr, D + 1);
    A(node_list, N * k + 1);  // (+ 1: the assembly reads one entry even of an empty list)
    A(rnode_ptr, D + 1);
    A(rnode_list, D * k + 1);  // (+ 1: the assembly reads one entry even of an empty list)
    A(dq, D * 8);
    A(dq_prev, D * 8);
    A(ghat, D * 3);
    A(rec, N * (12 + (k <= 4 ? 4 : 8)));
    A(cost_part, (N + 255) / 256 + (D * k + 255) / 256 + 1);
    A(valid_part, (N + 255) / 256 + (D * k + 255) / 256 + 1);
    A(mnode, D * 48);
    A(rho, N);
    A(rres, D * k * 3);
    A(rvec, D * k * 18);
    A(rhub, D * k);
    A(bcols, D * cap);
    A(bcnt, D);
    A(bfu, D);
    A(rslot, D * cap);
    A(utab, D * 256);
    A(eslot, N * k * k);
    A(pair_list, N * k * k);
    A(pair_ptr, D * (cap + 1));
    A(bvals, D * cap * 36);
    A(minv, D * 36);
    A(g, D * 6);
    A(x, D * 6);
    A(r, D * 6);
    A(p, D * 6);
    A(s, D * 6);
    A(w, D * 6);
    A(u[0], D * 6);
    A(u[1], D * 6);
    A(t[0], D * 6);
    A(t[1], D * 6);
    A(m[0], D * 6);
    A(m[1], D * 6);
    A(g_part[0], (size_t)dfa::s6_matvec_blocks(max_D));
    A(g_part[1], (size_t)dfa::s6_matvec_blocks(max_D));
    A(d_part[0], (size_t)dfa::s6_matvec_blocks(max_D));
    A(d_part[1], (size_t)dfa::s6_matvec_blocks(max_D));
#undef A
    mem.alloc(&s->raw_w, N * k);
    mem.alloc(&s->raw_reg, D * (k + 1));
    mem.alloc(&s->state, 1);
    int rc = plan_status(mem);
    if (rc == DFA_OK) {  // the launch budget's mirror and completion events (none: every PCG gets its full budget)
        bool ok = true;
        for (int i = 0; ok && i < dfa::S6_RING; ++i)
            ok = hipEventCreateWithFlags(&s->done_ev[i], hipEventDisableTiming) == hipSuccess;
        if (ok) s->mirror = mem.pinned<int>(dfa::S6_RING * dfa::S6_HIST);
        else (void)hipGetLastError();
        rc = plan_grid(s->grid, max_D);
    }
    if (rc != DFA_OK) {
        dfa_solver6_destroy(s);
        return rc;
    }
    *out = s;
    return DFA_OK;
}

void dfa_solver6_destroy(dfa_solver6* s) {
    if (!s) return;
    for (auto& g : s->pcg_graphs) (void)hipGraphExecDestroy(g.second);
    for (hipEvent_t e : s->done_ev)
        if (e) (void)hipEventDestroy(e);
    if (s->capture_stream) (void)hipStreamDestroy(s->capture_stream);
    s->grid.release();
    delete s;  // (the arena frees the plan's memory, the pool its events)
}

int dfa_solver6_set_problem(dfa_solver6* s, const float* node_pos, const float* node_dq, const float* node_w, int D,
                            const float* canon_vertices, const float* canon_normals, int N, dfa_stream_t stream) {
    REQUIRE(s, "null plan");
    REQUIRE(node_pos && node_dq && node_w && D > 0, "no nodes");
    REQUIRE(N >= 0 && (N == 0 || canon_vertices), "bad vertex arrays");
    if (D > s->max_D || N > s->max_N) return fail(DFA_ERR_CAPACITY, "problem larger than the plan");
    dfa::Solve6View& v = s->v;
    v.N = N, v.D = D, v.k = s->k;
    // (the solver reads its own, sorted copies of the vertices: s6_build_graph)
    v.node_pos = node_pos, v.node_w = node_w, v.canon = v.canon_own, v.canon_n = canon_normals ? v.canon_n_own : nullptr;
    s->node_dq = node_dq;
    const dfa::KnnGridView* grid = nullptr;
    if (want_grid(D, N)) {
        HIP_TRY(dfa::knn_grid_build(s->grid.v, node_pos, D, S(stream)));
        grid = &s->grid.v;
    }
    HIP_TRY(dfa::launch_knn(node_pos, node_w, D, canon_vertices, N, s->k, v.idx_nat, s->raw_w, grid, S(stream)));
    const int kreg = s->k + 1;
    HIP_TRY(dfa::launch_knn(node_pos, node_w, D, node_pos, D, kreg, s->raw_reg, nullptr, grid, S(stream)));
    HIP_TRY(dfa::s6_build_graph(v, s->state, canon_vertices, canon_normals, s->raw_w, s->raw_reg, kreg, S(stream),
                                s->hierarchical ? &s->hier : nullptr));
    s->has_problem  = true;
    s->graph_levels = s->hierarchical;
    s->has_mask     = false;  // a mask belongs to the vertex order it was given in
    return DFA_OK;
}

namespace {
// scratch of dfa_node_levels, which has no plan to keep it in
struct LevelScratch {
    dfa::DeviceBuffer<unsigned long long> table;
    dfa::DeviceBuffer<unsigned int> rep;
};
}  // namespace

int dfa_node_levels(const float* node_pos, int D, float epsilon, int beta, int levels, int32_t* out_level, dfa_stream_t stream) {
    REQUIRE(D >= 0 && (D == 0 || (node_pos && out_level)), "bad node arrays");
    REQUIRE(levels >= 1 && levels <= dfa::S6_REG_LEVELS, "levels out of range 1..8");
    REQUIRE(epsilon > 0.f && epsilon <= 3.0e38f, "epsilon must be positive");  // (false for NaN)
    REQUIRE(beta >= 2, "beta must be at least 2");
    if (D == 0) return DFA_OK;
    LevelScratch& sc = dfa::stream_scratch<LevelScratch>(S(stream));
    const size_t cap = dfa::reg_hierarchy_table(D, levels);
    HIP_TRY(sc.table.reserve(cap));
    HIP_TRY(sc.rep.reserve(cap));
    HIP_TRY(dfa::reg_hierarchy_levels(node_pos, D, epsilon, beta, levels, out_level, sc.table.data, sc.rep.data, S(stream)));
    return DFA_OK;
}

int dfa_solver6_set_reg_hierarchy(dfa_solver6* s, int levels, const int* slots, float epsilon, int beta) {
    if (levels > 1 && slots) {  // (the configuration before the plan: what is wrong with it does not depend on one)
        REQUIRE(levels <= dfa::S6_REG_LEVELS, "levels out of range 1..8");
        REQUIRE(epsilon > 0.f && epsilon <= 3.0e38f, "epsilon must be positive");
        REQUIRE(beta >= 2, "beta must be at least 2");
        REQUIRE(slots[0] >= 1, "level 0 needs at least one slot");
        for (int l = 1; l < levels; ++l) REQUIRE(slots[l] >= 0, "negative slot count");
    }
    REQUIRE(s, "null plan");
    if (levels <= 1 || !slots) {
        s->hierarchical = false;
        return DFA_OK;
    }
    long sum = 0;
    for (int l = 0; l < levels; ++l) sum += slots[l];
    REQUIRE(sum <= s->k, "more slots than the plan's k");
    if (!s->hier.level) {
        s->mem.alloc(&s->hier.level, (size_t)s->max_D);
        s->mem.alloc(&s->hier.table, dfa::reg_hierarchy_table(s->max_D, dfa::S6_REG_LEVELS));
        s->mem.alloc(&s->hier.rep, dfa::reg_hierarchy_table(s->max_D, dfa::S6_REG_LEVELS));
        const int rc = plan_status(s->mem);
        if (rc != DFA_OK) {
            s->hier.level = nullptr;
            return rc;
        }
    }
    s->hier.levels = levels, s->hier.epsilon = epsilon, s->hier.beta = beta;
    for (int l = 0; l < dfa::S6_REG_LEVELS; ++l) s->hier.slots[l] = l < levels ? slots[l] : 0;
    s->hierarchical = true;
    return DFA_OK;
}

int dfa_solver6_set_vertex_mask(dfa_solver6* s, const uint8_t* mask, dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    s->has_mask = false;
    if (!mask) return DFA_OK;
    if (!s->vmask) {
        s->mem.alloc(&s->vmask, (size_t)s->max_N);
        const int rc = plan_status(s->mem);
        if (rc != DFA_OK) return rc;
    }
    HIP_TRY(dfa::s6_gather_mask(s->v, mask, s->vmask, S(stream)));
    s->has_mask = true;
    return DFA_OK;
}

int dfa_solver6_set_node_transforms(dfa_solver6* s, const float* node_dq) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(node_dq, "null transforms");
    s->node_dq = node_dq;
    return DFA_OK;
}

int dfa_solver6_solve(dfa_solver6* s, const float* live_vertex_map, int vertex_step, const float* live_normal_map,
                      int normal_step, int cols, int rows, float fx, float fy, float cx, float cy,
                      const dfa_solve6_params* prm, dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(prm, "null params");
    REQUIRE(live_vertex_map && live_normal_map && cols > 0 && rows > 0, "bad live maps");
    REQUIRE(vertex_step >= cols * 16 && normal_step >= cols * 16, "row step smaller than a row");
    REQUIRE(prm->num_iter >= 0 && prm->gn_iter >= 0 && prm->linear_iter >= 0, "negative iteration count");
    REQUIRE(prm->tukey_offset > 0.f && prm->psi_data > 0.f && prm->psi_reg > 0.f, "non-positive robust parameter");
    REQUIRE(prm->damping >= 0.f && prm->lambda >= 0.f, "negative damping / lambda");
    REQUIRE(prm->pcg_tol_first <= 0.f || prm->pcg_tol_adapt > 0.f || (prm->pcg_tol_decay > 0.f && prm->pcg_tol_decay <= 1.f),
            "forcing decay outside (0, 1]");
    REQUIRE(prm->pcg_tol_adapt >= 0.f, "negative adaptive forcing factor");
    REQUIRE(prm->gn_tol >= 0.f && prm->gn_tol < 1.f, "gn_tol outside [0, 1)");
    dfa::Solve6Params p{prm->num_iter, prm->gn_iter, prm->linear_iter, prm->tukey_offset, prm->psi_data, prm->lambda,
                        prm->psi_reg, prm->dist_thresh, prm->cos_thresh, prm->damping, prm->pcg_tol, prm->pcg_tol_first,
                        prm->pcg_tol_decay, prm->pcg_tol_adapt, prm->gn_tol};
    const bool early = p.gn_tol > 0.f;
    dfa::Solve6Image img{live_vertex_map, live_normal_map, vertex_step, normal_step, cols, rows, fx, fy, cx, cy};
    hipStream_t st = S(stream);
    const uint8_t* vmask = s->has_mask ? s->vmask : nullptr;
    s->ev.rewind();
    HIP_TRY(dfa::s6_begin(s->v, s->state, s->node_dq, early ? p.num_iter * p.gn_iter : 0, st));
    s->last_launches = 0;
    // ---- launch budget (launch_budget.hpp): the solves up to n - 2 enter the history, in order, each behind its completion event
    dfa::LaunchBudget& budget = s->budget;
    const auto b = budget.start(prm->adaptive_launch && s->mirror,
                                dfa::BudgetKey{s->v.D, s->v.N, p.num_iter, p.gn_iter, p.linear_iter, p.pcg_tol, p.pcg_tol_first,
                                               p.pcg_tol_decay, p.pcg_tol_adapt, p.gn_tol});
    for (unsigned long long f = b.fold_from; f < b.fold_to; ++f) {
        const int fs = (int)(f % dfa::S6_RING);
        HIP_TRY(hipEventSynchronize(s->done_ev[fs]));  // two solves back: complete long ago unless the caller is far ahead
        budget.fold(s->mirror + fs * dfa::S6_HIST);
    }
    if (b.reset) budget.forget(b.n);
    int* mirror_slot = s->mirror ? s->mirror + b.slot * dfa::S6_HIST : nullptr;
    if (mirror_slot) {
        // the slot's previous owner, solve n - S6_RING, must have finished writing it (it has, unless the caller runs more
        // than S6_RING - 1 solves ahead of the device)
        if (b.slot_reused) HIP_TRY(hipEventSynchronize(s->done_ev[b.slot]));
        std::memset(mirror_slot, 0, dfa::S6_HIST * sizeof(int));
        budget.slot_gn[b.slot] = p.num_iter * p.gn_iter;
    }
    // the graphs replay launches over the plan's own buffers: only the node count is part of what they captured
    if (s->pcg_key_D != s->v.D) {
        for (auto& g : s->pcg_graphs) (void)hipGraphExecDestroy(g.second);
        s->pcg_graphs.clear();
        s->pcg_key_D = s->v.D;
    }
    for (int outer = 0; outer < p.num_iter; ++outer)
        for (int gn = 0; gn < p.gn_iter; ++gn) {
            auto mark = [&]() { if (s->timing) (void)s->ev.record(st); };  // 4 per Gauss-Newton iteration: | linearise | assemble | pcg |
            const int gi = outer * p.gn_iter + gn;
            mark();
            // gn_tol > 0: the launch's last workgroup applies the stopping rule on the device — launches behind the end of an
            // outer iteration return at entry (nothing comes back to the host: the launches of the whole solve are enqueued
            // regardless)
            HIP_TRY(dfa::s6_linearise(s->v, s->state, img, p, gn == 0, gi, gn, 0, vmask, st));
            mark();
            HIP_TRY(dfa::s6_assemble(s->v, s->state, p, gn, st));
            mark();
            int launches = budget.launches(gi, p.linear_iter);  // the caller's cap, or what this iteration has needed
            if (hipGraphExec_t replay = pcg_graph(s, launches))
                HIP_TRY_AS(hipGraphLaunch(replay, st), "hipGraphLaunch(it->second, st)");
            else
                HIP_TRY(dfa::s6_pcg_n(s->v, s->state, launches, st));
            s->last_launches += launches + 1;
            mark();
            HIP_TRY(dfa::s6_update(s->v, s->state, launches, p.linear_iter, gi < dfa::S6_HIST ? mirror_slot : nullptr, gi, 1, st));
        }
    if (early && p.num_iter * p.gn_iter > 0) {
        // the last step of the solve, if its outer iteration ran to the cap: one closing linearisation decides whether it stays
        const int gi = p.num_iter * p.gn_iter;
        HIP_TRY(dfa::s6_linearise(s->v, s->state, img, p, 0, gi, p.gn_iter, 1, vmask, st));
        HIP_TRY(dfa::s6_update(s->v, s->state, 0, p.linear_iter, nullptr, gi, 0, st));
    }
    if (mirror_slot) HIP_TRY(hipEventRecord(s->done_ev[b.slot], st));
    return DFA_OK;
}

int dfa_solver6_enable_timing(dfa_solver6* s, int enable) {
    REQUIRE(s, "null plan");
    s->timing = enable != 0;
    return DFA_OK;
}

int dfa_solver6_get_timing(dfa_solver6* s, dfa_solve6_timing* out, dfa_stream_t stream) {
    REQUIRE(s && out, "null plan / out");
    HIP_TRY(hipStreamSynchronize(S(stream)));
    std::memset(out, 0, sizeof(*out));
    const std::vector<hipEvent_t>& ev = s->ev.events;
    for (size_t i = 0; i + 3 < s->ev.used; i += 4) {
        float a = 0.f, b = 0.f, c = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, ev[i], ev[i + 1]));
        HIP_TRY(hipEventElapsedTime(&b, ev[i + 1], ev[i + 2]));
        HIP_TRY(hipEventElapsedTime(&c, ev[i + 2], ev[i + 3]));
        out->linearise_ms += a, out->assemble_ms += b, out->pcg_ms += c;
        out->gn_iterations += 1;
    }
    if (s->has_problem && s->v.D > 0)
        HIP_TRY_AS(row_count_sum(s->v.bcnt, s->v.D, &out->matrix_blocks),
                   "hipMemcpy(cnt.data(), s->v.bcnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost)");
    return DFA_OK;
}

const float* dfa_solver6_node_dq(const dfa_solver6* s) { return s ? s->v.dq : nullptr; }
static_assert(DFA_SOLVE6_ROW_BLOCKS == dfa::S6_ROW_BLOCKS, "row capacity of the C ABI and of the plan (S6_MAXSLOT of solve6_internal.hpp)");
const float* dfa_solver6_matrix_blocks(const dfa_solver6* s) { return s ? s->v.bvals : nullptr; }
const int32_t* dfa_solver6_matrix_columns(const dfa_solver6* s) { return s ? s->v.bcols : nullptr; }
const int32_t* dfa_solver6_matrix_row_blocks(const dfa_solver6* s) { return s ? s->v.bcnt : nullptr; }
const float* dfa_solver6_gradient(const dfa_solver6* s) { return s ? s->v.g : nullptr; }
const float* dfa_solver6_step(const dfa_solver6* s) { return s ? s->v.x : nullptr; }
const int32_t* dfa_solver6_data_graph(const dfa_solver6* s) { return s ? s->v.idx_nat : nullptr; }
const int32_t* dfa_solver6_reg_graph(const dfa_solver6* s) { return s ? s->v.reg_idx : nullptr; }
const int32_t* dfa_solver6_node_levels(const dfa_solver6* s) { return s && s->graph_levels ? s->hier.level : nullptr; }

int dfa_solver6_warp(dfa_solver6* s, float* out_vertices, float* out_normals, dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(out_vertices, "null output");
    HIP_TRY(dfa::s6_warp(s->v, s->v.dq, out_vertices, out_normals, S(stream)));
    return DFA_OK;
}

int dfa_solver6_warp_with(dfa_solver6* s, const float* node_dq, float* out_vertices, float* out_normals, dfa_stream_t stream) {
    REQUIRE(s && s->has_problem, "no problem set");
    REQUIRE(node_dq && out_vertices, "null transforms / output");
    HIP_TRY(dfa::s6_warp(s->v, node_dq, out_vertices, out_normals, S(stream)));
    return DFA_OK;
}

int dfa_solver6_get_stats(dfa_solver6* s, dfa_solve6_stats* out, dfa_stream_t stream) {
    REQUIRE(s && out, "null argument");
    dfa::Solve6State h;
    HIP_TRY(hipMemcpyAsync(&h, s->state, sizeof(h), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    out->initial_cost = h.initial_cost, out->final_cost = h.final_cost;
    out->gn_iters = h.gn_iters, out->pcg_iters = h.pcg_iters;
    out->gn_solves = h.gn_solves, out->gn_rejected = h.gn_rejected, out->gn_converged = h.gn_converged, out->hist_n = h.hist_n;
    out->valid_first = (long long)h.valid_first, out->valid_last = (long long)h.valid_last;
    out->max_row_blocks = h.max_row_blocks, out->overflow = h.overflow;
    out->pcg_short = h.pcg_short, out->pcg_launches = s->last_launches;
    static_assert(DFA_SOLVE6_HIST == dfa::S6_HIST, "history length of the C ABI and of the state block");
    for (int i = 0; i < DFA_SOLVE6_HIST; ++i) {
        const bool in = i < h.hist_n;
        out->valid_hist[i] = in ? (long long)h.valid_hist[i] : 0ll;
        out->stop_hist[i] = in ? h.stop_hist[i] : 0;
        out->cost_hist[i] = in ? h.cost_hist[i] : 0.0;
        out->pcg_rel_hist[i] = in ? h.pcg_rel_hist[i] : 0.f;
        out->pcg_tol_hist[i] = in ? h.pcg_tol_hist[i] : 0.f;
        out->pcg_it_hist[i] = in ? h.pcg_it_hist[i] : 0;
    }
    return h.overflow ? fail(DFA_ERR_CAPACITY, "a block row of the normal matrix exceeded the plan's capacity") : DFA_OK;
}

}  // extern "C"

#ifdef DFA_S6_DEBUG  // development builds only: device pointers of the north-star plan (tools/ns_plan_check.py)
extern "C" __attribute__((visibility("default"))) int dfa_dev_solver6_ptrs(dfa_solver6* s, void** out) {
    const dfa::Solve6View& v = s->v;
    void* p[] = {v.utab, v.pair_ptr, v.pair_list, v.bcnt, v.bfu, (void*)v.node_ptr, (void*)v.node_list, v.bcols, v.bvals, v.g,
                 (void*)v.idx, v.rec, nullptr, v.mnode, v.rslot};
    out[18] = v.minv;
    for (size_t i = 0; i < sizeof(p) / sizeof(p[0]); ++i) out[i] = p[i];
    out[15] = (void*)(size_t)v.cap, out[16] = (void*)(size_t)v.D, out[17] = (void*)(size_t)v.N;
    return 0;
}
#endif
