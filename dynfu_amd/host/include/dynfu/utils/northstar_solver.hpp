// dynfu/utils/northstar_solver.hpp — the 6-DoF solve of BASELINE.json's north star behind an interface shaped like
// CombinedSolver's (include/dynfu/utils/opt_solver.hpp:19-110).  NOT in the reference: its energy.t moves node
// TRANSLATIONS towards matched live VERTICES; this solver moves full node transforms (a twist per node) towards the live
// DEPTH FRAME — dual-quaternion blend of the k nearest nodes, projective association into the live vertex / normal maps,
// point-to-plane data term (Tukey), ARAP regulariser (Huber), Gauss-Newton with a block-Jacobi PCG (DESIGN.md §4.5,
// dfa_solver6_* in include/dynfu_amd.h).  Same life cycle as CombinedSolver:
//     NorthStarSolver solver(*warpfield, params, tukeyOffset, psi_data, lambda, psi_reg);
//     solver.initializeProblemInstance(canonicalFrame);      // graphs of the frame (canonical cloud WITH normals)
//     solver.solveAll(liveDepth, intr);                      // vertex / normal maps of the depth frame, solve, write-back
// and the shared Nodes come out with their dg_se3 REPLACED by the solved transforms.  The canonical cloud, the nodes and
// the depth frame must be in ONE frame: the camera's.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include <dynfu/utils/frame.hpp>
#include <dynfu/warp_field.hpp>
#include <kfusion/types.hpp>

struct NorthStarParameters {
    int numIter      = 2;   // outer iterations: robust weights re-evaluated
    int gnIter       = 3;   // Gauss-Newton iterations per outer iteration
    int linearIter   = 64;  // PCG iterations per Gauss-Newton iteration, at most
    float distThresh = 0.1f;   // association gate |p - l| (metres)         (KinFuParams::icp_dist_thres)
    float cosThresh  = 0.5f;   // association gate n_warped . n_live
    float damping    = 1e-4f;  // added to the diagonal of the normal matrix
    // PCG stop test: relative residual max(pcgTol, pcgTolFirst * pcgTolDecay^i) at Gauss-Newton iteration i of an outer
    // iteration (inexact Newton: early linearisations are solved loosely); pcgTolFirst <= 0: constant pcgTol
    float pcgTol      = 1e-3f;
    float pcgTolFirst = 0.1f;
    float pcgTolDecay = 0.5f;
    // > 0: the Eisenstat-Walker forcing term instead of the geometric schedule (dfa_solve6_params.pcg_tol_adapt)
    float pcgTolAdapt = 0.9f;
    // enqueue only as many PCG launches per Gauss-Newton iteration as the previous frames needed (+ a quarter): see
    // dfa_solve6_params.adaptive_launch in dynfu_amd.h
    bool adaptiveLaunch = true;
    // Gauss-Newton stopping rule + step acceptance (dfa_solve6_params.gn_tol): gnIter is a cap, as nonLinearIter is for the
    // reference, which runs Opt with earlyOut = true (src/dynfu/dyn_fusion.cpp:183-189).  0: every iteration runs.
    float gnTol = 1e-3f;
};

// the k the north-star blend reads, of a warp field with `field_knn` neighbours: a dfa_solver6 plan blends at most 8 nodes
// (the reference's KNN)
inline int northStarKnn(int field_knn) { return std::min(field_knn, 8); }

class NorthStarSolver {
public:
    NorthStarSolver(Warpfield warpfield, NorthStarParameters params, float tukeyOffset, float psi_data, float lambda,
                    float psi_reg);
    ~NorthStarSolver();

    void initializeProblemInstance(const std::shared_ptr<dynfu::Frame> canonicalFrame);
    void solveAll(const kfusion::cuda::Depth& liveDepth, const kfusion::Intr& intr);
    // ... or against maps the caller already has (kfusion::cuda::computePointNormals, TsdfVolume::raycast)
    void solveAll(const kfusion::cuda::Cloud& liveVertexMap, const kfusion::cuda::Normals& liveNormalMap,
                  const kfusion::Intr& intr);

    // Rigid pre-alignment (call it after initializeProblemInstance, before solveAll): the rigid Gauss-Newton
    // of the solve's own data term.  The canonical cloud and its normals are warped once by the transforms the solve starts
    // from (dfa_solver6_warp_with); then, `iters` times, dfa_rigid_sums_cloud with distThresh / cosThresh against the live
    // maps, one read-back of the 27 sums and kfusion::cuda::icp_update: T <- exp(x) T, from the identity.  T maps the
    // start-warped model into the live camera's frame.  On success T is composed onto the start transforms of the plan
    // (dfa_solver6_set_node_transforms) and onto the shared Nodes (Warpfield::composeRigid): the north-star blend is
    // left-invariant, so the solve starts from the same field moved by T — as do the model view, the visibility test, the
    // fusion and the node insertion that read the Nodes.  A singular update ends the loop: T goes back to the identity,
    // nothing is composed, the call returns false.  iters <= 0: nothing is enqueued, T is the identity, true.
    bool alignRigid(const kfusion::cuda::Cloud& liveVertexMap, const kfusion::cuda::Normals& liveNormalMap,
                    const kfusion::Intr& intr, int iters, dfa::Affine3f& T);
    // The same estimate with the whole Gauss-Newton loop on the device (dfa_rigid_align_cloud): one warp, one call that
    // enqueues every iteration of the schedule — level l over every steps[l]-th vertex of the warped cloud for at most
    // iters[l] iterations, a level ended early by an accepted step with |rvec| < stopRot and |tvec| < stopTrans (0: never) —
    // and ONE read-back, of the report.  T is then composed as above.  A singular system: T is the identity, nothing is
    // composed, false.  A schedule without iterations: nothing is enqueued, T is the identity, true.
    struct RigidSchedule {
        std::vector<int> steps, iters;  // one entry per level, in the order they run (coarsest first); 1 to 4 levels
        float stopRot = 0.f, stopTrans = 0.f;  // radians, metres
    };
    bool alignRigid(const kfusion::cuda::Cloud& liveVertexMap, const kfusion::cuda::Normals& liveNormalMap,
                    const kfusion::Intr& intr, const RigidSchedule& schedule, dfa::Affine3f& T);
    // iterations (accepted or refused) each level of the last schedule ran; empty after the host-loop overload
    const std::vector<int>& rigidIterationsRun() const { return rigid_iters_run_; }
    // vertices that took a row in the first / the last iteration of the last alignRigid (0 before it)
    long long rigidMatchedFirst() const { return rigid_matched_first_; }
    long long rigidMatchedLast() const { return rigid_matched_last_; }

    // the canonical frame of the problem warped by the solved transforms (dual-quaternion blend, as the solve models
    // it); stays in HBM
    std::shared_ptr<dynfu::Frame> warpCanonicalToLive();
    // ... warped by the transforms the solve STARTS from (the nodes' as initializeProblemInstance found them): the same
    // blend, no solve needed (dfa_solver6_warp_with).  Vertices only, packed N x 3
    dfa::DeviceArray<float> warpCanonicalByStart();

    // Which canonical vertices may take a data row in the solveAll calls that follow (dfa_solver6_set_vertex_mask): one byte
    // per vertex of the canonical frame, in its order, non-zero = may.  Every initializeProblemInstance starts without a
    // mask; the bytes are copied by the work the call enqueues.
    void setVertexMask(const dfa::DeviceArray<unsigned char>& mask);
    void clearVertexMask();

    // The multi-level regularisation graph (dfa_solver6_set_reg_hierarchy in include/dynfu_amd.h states the rule) for the
    // initializeProblemInstance calls that follow: slots[l] columns of a node's row for level l, cells of epsilon beta^l.
    // One level or none: the flat graph.  Throws dfa::Error for what that call refuses — more than 8 levels, slots[0] < 1, a
    // negative slot, a slot sum above the k the plan blends (the warp field's, at most 8), epsilon <= 0, beta < 2.
    void setRegHierarchy(std::vector<int> slots, float epsilon, int beta);
    // that rule on the host, for a plan that blends k nodes: 1 to 8 levels, slots[0] >= 1, no negative slot, a slot sum of at
    // most k, epsilon > 0, beta >= 2.  (setRegHierarchy asks it of two levels or more, DynFuParams::validate of any.)
    static bool regHierarchyAccepted(const std::vector<int>& slots, float epsilon, int beta, int k);
    // the level of every node of the last initializeProblemInstance's graph (one read from the device); empty while it is flat
    std::vector<int> nodeLevels() const;

    double initialCost() const { return initial_cost_; }
    double finalCost() const { return final_cost_; }
    long long validRows() const { return valid_rows_; }  // data rows with an association at the last linearisation
    int pcgIterations() const { return pcg_iters_; }
    /* PCGs of the last solveAll that stopped at the end of their adaptive launch budget instead of at their tolerance */
    int pcgsCutShort() const { return pcg_short_; }
    /* normal equations solved / steps undone by the acceptance test in the last solveAll (gnTol > 0) */
    int gnSolves() const { return gn_solves_; }
    int gnRejected() const { return gn_rejected_; }

private:
    Warpfield m_warpfield;  // copied by value, Nodes shared (as CombinedSolver, opt_solver.cpp:5)
    NorthStarParameters m_params;
    float tukeyOffset, psi_data, lambda, psi_reg;
    struct Impl;
    std::shared_ptr<Impl> impl;
    // alignRigid's frame around its two loops.  begin: T and the report reset, the checks (`schedule`, or null and the host
    // loop's `iters`), and — with iterations to run — cloud and normals warped by the start transforms; false: nothing to
    // run.  commit: T composed onto the start transforms, host and device, and onto the shared Nodes
    bool beginAlignRigid(const kfusion::cuda::Cloud& vmap, const kfusion::cuda::Normals& nmap, const RigidSchedule* schedule, int iters,
                         dfa::Affine3f& T, dfa::DeviceArray<float>& warped, dfa::DeviceArray<float>& warped_normals);
    void commitAlignRigid(const dfa::Affine3f& T);
    double initial_cost_ = 0.0, final_cost_ = 0.0;
    long long valid_rows_ = 0;
    int pcg_iters_        = 0;
    int pcg_short_        = 0;
    int gn_solves_ = 0, gn_rejected_ = 0;
    long long rigid_matched_first_ = 0, rigid_matched_last_ = 0;
    std::vector<int> rigid_iters_run_;
    std::vector<int> reg_slots_;  // setRegHierarchy (empty: flat)
    float reg_epsilon_ = 0.f;
    int reg_beta_      = 0;
};
