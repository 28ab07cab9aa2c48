// northstar_solver.cpp — NorthStarSolver on the dfa_solver6 plan (see dynfu/utils/northstar_solver.hpp).
#include <cstdio>
#include <dynfu/utils/northstar_solver.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include <dfa_host/plan_cache.hpp>
#include <kfusion/cuda/icp_update.hpp>
#include <kfusion/cuda/imgproc.hpp>

#include "../../../include/dynfu_amd.h"

extern void dfa_host_copy_from_device(void*, const void*, size_t);

namespace {
// What the graphs of a plan were built from.  A DynFusion solves frame after frame over the SAME canonical cloud and —
// until the field grows — the same nodes: k-NN, transposition and pair lists of the frame before are then still right and
// only the starting transforms change (dfa_solver6_set_node_transforms).  The arrays are kept alive here: the plan
// borrows them.
struct Built {
    dfa::DeviceArray<float> node_pos, node_w, canon, canon_n;
    int D = 0, N = 0, k = 0;
    uint64_t nodes_hash = 0;
    std::vector<int> reg_slots;  // the regularisation hierarchy the graph was built with (empty: flat)
    float reg_epsilon = 0.f;
    int reg_beta      = 0;
};
std::mutex g_built_mu;
std::map<dfa_solver6*, Built> g_built;

void destroy_plan6(dfa_solver6* p) {
    {
        std::lock_guard<std::mutex> lock(g_built_mu);
        g_built.erase(p);
    }
    dfa_solver6_destroy(p);
}
dfa::PlanCache<dfa_solver6, destroy_plan6>& plan_cache() {
    static dfa::PlanCache<dfa_solver6, destroy_plan6> c;
    return c;
}
uint64_t fnv1a(const std::vector<float>& a, uint64_t h) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(a.data());
    for (size_t i = 0; i < a.size() * sizeof(float); ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
}  // namespace

struct NorthStarSolver::Impl {
    dfa_solver6* plan = nullptr;
    int plan_D = 0, plan_N = 0, plan_k = 0;
    dfa::DeviceArray<float> node_pos, node_dq, node_w, canon, canon_n;  // borrowed by the plan until the next set_problem
    kfusion::cuda::Cloud vmap;
    kfusion::cuda::Normals nmap;
    std::vector<float> host_dq;  // the start transforms as uploaded to node_dq
    int D = 0, N = 0;
    ~Impl() { plan_cache().park(plan, plan_D, plan_N, plan_k); }
};

NorthStarSolver::NorthStarSolver(Warpfield warpfield, NorthStarParameters params, float tukeyOffset_, float psi_data_,
                                 float lambda_, float psi_reg_)
    : m_warpfield(std::move(warpfield)), m_params(params), tukeyOffset(tukeyOffset_), psi_data(psi_data_), lambda(lambda_),
      psi_reg(psi_reg_), impl(std::make_shared<Impl>()) {}
NorthStarSolver::~NorthStarSolver() = default;

void NorthStarSolver::initializeProblemInstance(const std::shared_ptr<dynfu::Frame> canonicalFrame) {
    const int D = (int)m_warpfield.nodesRef().size(), N = (int)canonicalFrame->size();
    if (D == 0) throw dfa::Error(DFA_ERR_INVALID, "NorthStarSolver: the warp field has no nodes");
    std::vector<float> pos, w, dq;
    m_warpfield.hostArrays(pos, w, dq);
    Impl& I = *impl;
    I.D = D, I.N = N;
    canonicalFrame->deviceArrays(I.canon, I.canon_n);
    const int k = northStarKnn(m_warpfield.getKnn());
    if (I.plan && !(I.plan_k == k && I.plan_D >= D && I.plan_N >= N)) {
        plan_cache().park(I.plan, I.plan_D, I.plan_N, I.plan_k);
        I.plan = nullptr;
    }
    if (!I.plan) {
        I.plan   = plan_cache().take(D, N, k, I.plan_D, I.plan_N);
        I.plan_k = k;
    }
    if (!I.plan) {
        I.plan_D = dfa::grown_node_capacity(D), I.plan_N = dfa::grown_vertex_capacity(N);
        dfa::check(dfa_solver6_create(I.plan_D, I.plan_N, k, &I.plan), "NorthStarSolver: dfa_solver6_create");
    }
    // (a plan from the cache may have served a solver with another hierarchy, or none)
    const bool hierarchy = reg_slots_.size() > 1;
    dfa::check(dfa_solver6_set_reg_hierarchy(I.plan, hierarchy ? (int)reg_slots_.size() : 0, hierarchy ? reg_slots_.data() : nullptr,
                                             reg_epsilon_, reg_beta_),
               "NorthStarSolver: set_reg_hierarchy");
    const std::vector<int> slots_now = hierarchy ? reg_slots_ : std::vector<int>();
    I.node_dq.upload(dq);
    I.host_dq = dq;
    const uint64_t nodes_hash = fnv1a(w, fnv1a(pos, 1469598103934665603ull));
    {
        std::lock_guard<std::mutex> lock(g_built_mu);
        auto it = g_built.find(I.plan);
        if (it != g_built.end() && !dfa::host_switch("DFA_HOST_NO_GRAPH_REUSE")) {
            const Built& b = it->second;
            if (b.D == D && b.N == N && b.k == k && b.nodes_hash == nodes_hash && b.canon.ptr() == I.canon.ptr() &&
                b.canon_n.ptr() == I.canon_n.ptr() && b.reg_slots == slots_now &&
                (!hierarchy || (b.reg_epsilon == reg_epsilon_ && b.reg_beta == reg_beta_))) {
                I.node_pos = b.node_pos, I.node_w = b.node_w;  // shared: the plan reads them
                dfa::check(dfa_solver6_set_node_transforms(I.plan, I.node_dq.ptr()), "NorthStarSolver: set_node_transforms");
                // a mask stays across set_node_transforms, and the plan may have served another solver: a frame starts without
                dfa::check(dfa_solver6_set_vertex_mask(I.plan, nullptr, nullptr), "NorthStarSolver: set_vertex_mask");
                return;
            }
        }
    }
    I.node_pos = dfa::DeviceArray<float>(), I.node_w = dfa::DeviceArray<float>();  // fresh arrays: older ones may be shared
    I.node_pos.upload(pos), I.node_w.upload(w);
    dfa::check(dfa_solver6_set_problem(I.plan, I.node_pos.ptr(), I.node_dq.ptr(), I.node_w.ptr(), D, I.canon.ptr(),
                                       I.canon_n.ptr(), N, nullptr),
               "NorthStarSolver::initializeProblemInstance");
    std::lock_guard<std::mutex> lock(g_built_mu);
    Built& b = g_built[I.plan];
    b.node_pos = I.node_pos, b.node_w = I.node_w, b.canon = I.canon, b.canon_n = I.canon_n;
    b.D = D, b.N = N, b.k = k, b.nodes_hash = nodes_hash;
    b.reg_slots = slots_now, b.reg_epsilon = reg_epsilon_, b.reg_beta = reg_beta_;
}

void NorthStarSolver::setRegHierarchy(std::vector<int> slots, float epsilon, int beta) {
    // the plan's own checks, on no plan: a configuration it refuses is refused here, before a frame is under way
    if (slots.size() > 1 && !regHierarchyAccepted(slots, epsilon, beta, northStarKnn(m_warpfield.getKnn())))
        throw dfa::Error(DFA_ERR_INVALID, "NorthStarSolver::setRegHierarchy: at most 8 levels, slots[0] >= 1, no negative slot, "
                                          "a slot sum of at most the field's k, epsilon > 0, beta >= 2");
    reg_slots_ = std::move(slots), reg_epsilon_ = epsilon, reg_beta_ = beta;
}

bool NorthStarSolver::regHierarchyAccepted(const std::vector<int>& slots, float epsilon, int beta, int k) {
    long sum = 0;
    bool ok  = !slots.empty() && slots.size() <= 8 && slots[0] >= 1 && epsilon > 0.f && beta >= 2;
    for (int v : slots) ok = ok && v >= 0, sum += v;
    return ok && sum <= k;
}

std::vector<int> NorthStarSolver::nodeLevels() const {
    const Impl& I = *impl;
    const int32_t* lv = I.plan ? dfa_solver6_node_levels(I.plan) : nullptr;
    std::vector<int> out;
    if (lv && I.D > 0) {
        out.resize((size_t)I.D);
        dfa_host_copy_from_device(out.data(), lv, out.size() * sizeof(int));
    }
    return out;
}

void NorthStarSolver::solveAll(const kfusion::cuda::Depth& liveDepth, const kfusion::Intr& intr) {
    Impl& I = *impl;
    kfusion::cuda::computePointNormals(intr, liveDepth, I.vmap, I.nmap);  // imgproc.cu:187-226
    solveAll(I.vmap, I.nmap, intr);
}

void NorthStarSolver::solveAll(const kfusion::cuda::Cloud& vmap, const kfusion::cuda::Normals& nmap, const kfusion::Intr& intr) {
    Impl& I = *impl;
    if (!I.plan) throw dfa::Error(DFA_ERR_INVALID, "solveAll before initializeProblemInstance");
    if (vmap.rows() != nmap.rows() || vmap.cols() != nmap.cols() || vmap.empty())
        throw dfa::Error(DFA_ERR_INVALID, "NorthStarSolver: vertex / normal maps differ in size or are empty");
    dfa_solve6_params p;
    p.num_iter     = m_params.numIter;
    p.gn_iter      = m_params.gnIter;
    p.linear_iter  = m_params.linearIter;
    p.tukey_offset = tukeyOffset;
    p.psi_data     = psi_data;
    p.lambda       = lambda;
    p.psi_reg      = psi_reg;
    p.dist_thresh  = m_params.distThresh;
    p.cos_thresh   = m_params.cosThresh;
    p.damping      = m_params.damping;
    p.pcg_tol      = m_params.pcgTol;
    p.pcg_tol_first = m_params.pcgTolFirst;
    p.pcg_tol_decay = m_params.pcgTolDecay;
    p.pcg_tol_adapt = m_params.pcgTolAdapt;
    p.adaptive_launch = m_params.adaptiveLaunch ? 1 : 0;
    p.gn_tol          = m_params.gnTol;
    dfa::check(dfa_solver6_solve(I.plan, (const float*)vmap.ptr(), (int)vmap.step(), (const float*)nmap.ptr(), (int)nmap.step(),
                                 vmap.cols(), vmap.rows(), intr.fx, intr.fy, intr.cx, intr.cy, &p, nullptr),
               "NorthStarSolver::solveAll");
    dfa_solve6_stats st;
    dfa::check(dfa_solver6_get_stats(I.plan, &st, nullptr), "NorthStarSolver::solveAll (stats)");  // synchronises
    initial_cost_ = st.initial_cost, final_cost_ = st.final_cost, valid_rows_ = st.valid_last, pcg_iters_ = st.pcg_iters;
    pcg_short_ = st.pcg_short, gn_solves_ = st.gn_solves, gn_rejected_ = st.gn_rejected;
    if (st.pcg_short > 0) {  // a PCG stopped where its launch budget ended (still a descent step); the plan doubles that budget
        static bool told = false;
        if (!told)
            std::fprintf(stderr, "NorthStarSolver: %d PCG(s) of this solve were cut short by the adaptive launch budget "
                                 "(pcgsCutShort(); NorthStarParameters::adaptiveLaunch = false enqueues the full budget)\n",
                         st.pcg_short);
        told = true;
    }
    // the solved transforms replace dg_se3 of the shared Nodes (the reference's solver composes a translation onto it,
    // opt_solver.cpp:270-285; here the unknown IS the transform)
    std::vector<float> dq(8 * (size_t)I.D);
    dfa_host_copy_from_device(dq.data(), dfa_solver6_node_dq(I.plan), dq.size() * sizeof(float));
    const auto& nodes = m_warpfield.nodesRef();
    for (int i = 0; i < I.D; ++i) {
        const float* q = &dq[8 * (size_t)i];
        nodes[i]->setTransformation(std::make_shared<DualQuaternion<float>>(dfa::quaternion<float>(q[0], q[1], q[2], q[3]),
                                                                            dfa::quaternion<float>(q[4], q[5], q[6], q[7])));
    }
}

bool NorthStarSolver::beginAlignRigid(const kfusion::cuda::Cloud& vmap, const kfusion::cuda::Normals& nmap, const RigidSchedule* schedule,
                                      int iters, dfa::Affine3f& T, dfa::DeviceArray<float>& wv, dfa::DeviceArray<float>& wn) {
    Impl& I = *impl;
    T = dfa::Affine3f();
    rigid_matched_first_ = rigid_matched_last_ = 0;
    rigid_iters_run_.assign(schedule ? schedule->steps.size() : 0, 0);
    if (!I.plan) throw dfa::Error(DFA_ERR_INVALID, "alignRigid before initializeProblemInstance");
    if (vmap.rows() != nmap.rows() || vmap.cols() != nmap.cols() || vmap.empty())
        throw dfa::Error(DFA_ERR_INVALID, "NorthStarSolver: vertex / normal maps differ in size or are empty");
    if (schedule) {
        if (schedule->steps.size() != schedule->iters.size())
            throw dfa::Error(DFA_ERR_INVALID, "NorthStarSolver::alignRigid: one step and one iteration count per level");
        iters = 0;
        for (int n : schedule->iters) iters += n > 0 ? n : 0;
    }
    if (iters <= 0) return false;
    wv = dfa::DeviceArray<float>(3 * (size_t)I.N), wn = dfa::DeviceArray<float>(3 * (size_t)I.N);
    if (I.N) dfa::check(dfa_solver6_warp_with(I.plan, I.node_dq.ptr(), wv.ptr(), wn.ptr(), nullptr), "NorthStarSolver::alignRigid (warp)");
    return true;
}

void NorthStarSolver::commitAlignRigid(const dfa::Affine3f& T) {
    Impl& I = *impl;
    Warpfield::composeRigid(T, I.host_dq.data(), (size_t)I.D);
    I.node_dq.upload(I.host_dq);
    dfa::check(dfa_solver6_set_node_transforms(I.plan, I.node_dq.ptr()), "NorthStarSolver::alignRigid (set_node_transforms)");
    m_warpfield.composeRigid(T);
}

bool NorthStarSolver::alignRigid(const kfusion::cuda::Cloud& vmap, const kfusion::cuda::Normals& nmap, const kfusion::Intr& intr,
                                 int iters, dfa::Affine3f& T) {
    Impl& I = *impl;
    dfa::DeviceArray<float> wv, wn;
    if (!beginAlignRigid(vmap, nmap, nullptr, iters, T, wv, wn)) return true;
    dfa::DeviceArray<float> out(28);  // the 27 sums, then the matched count: one read-back per iteration
    float h[28];
    for (int it = 0; it < iters; ++it) {
        float aff[12];
        T.to12(aff);
        dfa::check(dfa_rigid_sums_cloud(wv.ptr(), wn.ptr(), 3, I.N, aff, (const float*)vmap.ptr(), (int)vmap.step(),
                                        (const float*)nmap.ptr(), (int)nmap.step(), vmap.cols(), vmap.rows(), intr.fx, intr.fy,
                                        intr.cx, intr.cy, m_params.distThresh, m_params.cosThresh, out.ptr(),
                                        reinterpret_cast<unsigned int*>(out.ptr() + 27), nullptr),
                   "NorthStarSolver::alignRigid");
        dfa_host_copy_from_device(h, out.ptr(), sizeof(h));
        unsigned int matched;
        std::memcpy(&matched, &h[27], sizeof(matched));
        if (it == 0) rigid_matched_first_ = matched;
        rigid_matched_last_ = matched;
        if (!kfusion::cuda::icp_update(h, T)) {
            T = dfa::Affine3f();
            return false;
        }
    }
    commitAlignRigid(T);
    return true;
}

bool NorthStarSolver::alignRigid(const kfusion::cuda::Cloud& vmap, const kfusion::cuda::Normals& nmap, const kfusion::Intr& intr,
                                 const RigidSchedule& schedule, dfa::Affine3f& T) {
    Impl& I = *impl;
    dfa::DeviceArray<float> wv, wn;
    if (!beginAlignRigid(vmap, nmap, &schedule, 0, T, wv, wn)) return true;  // as iters <= 0 of the host loop
    static_assert(sizeof(dfa_rigid_align_report) % sizeof(float) == 0, "the report travels as words");
    dfa::DeviceArray<float> out(sizeof(dfa_rigid_align_report) / sizeof(float));
    float aff0[12];
    T.to12(aff0);
    dfa::check(dfa_rigid_align_cloud(wv.ptr(), wn.ptr(), 3, I.N, aff0, (const float*)vmap.ptr(), (int)vmap.step(),
                                     (const float*)nmap.ptr(), (int)nmap.step(), vmap.cols(), vmap.rows(), intr.fx, intr.fy, intr.cx,
                                     intr.cy, m_params.distThresh, m_params.cosThresh, schedule.steps.data(), schedule.iters.data(),
                                     (int)schedule.steps.size(), schedule.stopRot, schedule.stopTrans,
                                     reinterpret_cast<dfa_rigid_align_report*>(out.ptr()), nullptr, nullptr),
               "NorthStarSolver::alignRigid (device loop)");
    dfa_rigid_align_report rep;
    dfa_host_copy_from_device(&rep, out.ptr(), sizeof(rep));  // the one read-back
    rigid_matched_first_ = rep.matched_first, rigid_matched_last_ = rep.matched_last;
    for (size_t l = 0; l < rigid_iters_run_.size(); ++l) rigid_iters_run_[l] = rep.iters_run[l];
    if (rep.status != 0) return false;
    for (int i = 0; i < 9; ++i) T.R[i] = rep.aff[i];
    for (int i = 0; i < 3; ++i) T.t[i] = rep.aff[9 + i];
    commitAlignRigid(T);
    return true;
}

dfa::DeviceArray<float> NorthStarSolver::warpCanonicalByStart() {
    Impl& I = *impl;
    if (!I.plan) throw dfa::Error(DFA_ERR_INVALID, "warpCanonicalByStart before initializeProblemInstance");
    dfa::DeviceArray<float> ov(3 * (size_t)I.N);
    if (I.N) dfa::check(dfa_solver6_warp_with(I.plan, I.node_dq.ptr(), ov.ptr(), nullptr, nullptr), "NorthStarSolver::warpCanonicalByStart");
    return ov;
}

void NorthStarSolver::setVertexMask(const dfa::DeviceArray<unsigned char>& mask) {
    Impl& I = *impl;
    if (!I.plan) throw dfa::Error(DFA_ERR_INVALID, "setVertexMask before initializeProblemInstance");
    if (mask.size() != (size_t)I.N) throw dfa::Error(DFA_ERR_INVALID, "NorthStarSolver::setVertexMask: one byte per canonical vertex");
    if (I.N) dfa::check(dfa_solver6_set_vertex_mask(I.plan, mask.ptr(), nullptr), "NorthStarSolver::setVertexMask");
}

void NorthStarSolver::clearVertexMask() {
    Impl& I = *impl;
    if (!I.plan) throw dfa::Error(DFA_ERR_INVALID, "clearVertexMask before initializeProblemInstance");
    dfa::check(dfa_solver6_set_vertex_mask(I.plan, nullptr, nullptr), "NorthStarSolver::clearVertexMask");
}

std::shared_ptr<dynfu::Frame> NorthStarSolver::warpCanonicalToLive() {
    Impl& I = *impl;
    if (!I.plan) throw dfa::Error(DFA_ERR_INVALID, "warpCanonicalToLive before initializeProblemInstance");
    dfa::DeviceArray<float> ov(3 * (size_t)I.N), on(3 * (size_t)I.N);
    if (I.N) dfa::check(dfa_solver6_warp(I.plan, ov.ptr(), on.ptr(), nullptr), "NorthStarSolver::warpCanonicalToLive");
    return dynfu::Frame::fromDevice(0, ov, on, (size_t)I.N);
}
