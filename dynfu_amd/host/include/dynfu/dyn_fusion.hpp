// dynfu/dyn_fusion.hpp — class DynFusion with the reference's interface (include/dynfu/dyn_fusion.hpp:25-90,
// src/dynfu/dyn_fusion.cpp).  As in the reference (:45) it IS-A kfusion::KinFu: the volume, the marching-cubes
// object, the frame counter, the pose chain and the inherited accessors (tsdf(), mc(), icp(), getCameraPose(),
// KinFu::params()) are the base class's; DynFusion::params() returns the DynFuParams and operator() replaces the
// rigid loop by the per-frame warp-field sequence of dyn_fusion.cpp:48-242 on the dynfu_amd C ABI:
//   init                    node seeding, every 128th canonical vertex            (:147-168)
//   addLiveFrame            store the live cloud                                  (:177-180)
//   warpCanonicalToLiveOpt  warp -> correspond -> build -> solve -> write-back    (:182-210)
//   findCorrespondingFrame  nearest warped-canonical vertex of every live vertex  (:212-242)
// plus fuse(): the TSDF steps of operator() (:58,:108-115 — dists, clear, integrate) on a caller-
// owned kfusion::cuda::TsdfVolume.  Vertices come from the caller (marching cubes is a later row).
#pragma once
#include <cstddef>
#include <memory>
#include <vector>

#include <dfa_host/io.hpp>
#include <dynfu/utils/frame.hpp>
#include <dynfu/utils/northstar_solver.hpp>
#include <dynfu/utils/opt_solver.hpp>
#include <dynfu/warp_field.hpp>
#include <kfusion/cuda/imgproc.hpp>
#include <kfusion/cuda/marching_cubes.hpp>
#include <kfusion/cuda/mesh_render.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>
#include <kfusion/kinfu.hpp>

struct DynFuParams {  // dyn_fusion.hpp:25-42
    static DynFuParams defaultParams();  // dyn_fusion.cpp:6-31
    kfusion::KinFuParams kinfuParams;
    kfusion::Intr intr;  // = kinfuParams.intr (kept for callers of fuse())
    float tukeyOffset;
    float lambda;
    float psi_data;
    float psi_reg;
    int L;
    int beta;
    float epsilon;
    // Extension (off = the reference's behaviour: default-constructed normals, dyn_fusion.cpp:80-88): normals of the
    // extracted vertices from the TSDF gradient (MarchingCubes::computeNormals)
    bool mesh_normals = false;
    // Extension — the north-star mode (BASELINE.json): operator() solves full 6-DoF node transforms
    // against the live DEPTH FRAME (NorthStarSolver: dual-quaternion blend, projective point-to-plane, ARAP) instead of
    // the reference's translations against the nearest live marching-cubes vertices.  The canonical cloud (with normals
    // from the TSDF gradient), the nodes and getCanonicalWarpedToLive() are then in the CAMERA frame (the frame of the
    // depth maps); getLiveFrame() / getMesh() stay the volume-frame marching-cubes output.
    bool north_star = false;
    NorthStarParameters northStarParams;
    // Extension — the view of the canonical model: frame 0 also extracts the fused volume as a welded mesh
    // with normals (MarchingCubes::runIndexed / computeNormals) and keeps it in HBM, in the frame of the canonical cloud;
    // DynFusion::renderWarpedModel carries it through the warp field and rasterises it from the live camera.  Off: nothing
    // of this runs.  On or off, everything else a frame produces is the same, bit for bit.  The warp is the one the mode's
    // solve fitted: Warpfield::warpToLive (the reference's blend) in reference mode, the dual-quaternion blend of the
    // north-star solve (dfa_solver6_warp_with on a plan of the view's own) in north-star mode — the two differ as soon as
    // a transform is not the identity, and the model has to move as getCanonicalWarpedToLive() does.
    bool model_view = false;
    float model_view_z_near = 0.05f;  // metres: triangles with a vertex nearer to the camera are not drawn
    // Extension — dense non-rigid surface fusion (step 4 of the reference's pipeline, dyn_fusion.cpp:39-47, which it never
    // does); reference mode only.  Frame 0 copies the integrated volume into a second TsdfVolume, the CANONICAL volume
    // (DynFusion::canonicalVolume()); every later frame, once the warp field is solved and before it grows, integrates that
    // frame's depth into it through the warp field (TsdfVolume::integrateWarped, voxels no node supports left alone).  The
    // per-frame live volume, the live cloud, the solve and the node insertion are untouched — the canonical cloud stays
    // frame 0's —: off, nothing of this runs, and on or off every other output of a frame is the same, bit for bit.  With
    // north_star the constructor throws dfa::Error: that mode has another blend and keeps its nodes in the camera frame —
    // its switch is north_star_fuse_canonical.
    bool fuse_canonical = false;
    // Extension — the same fusion in north-star mode (north_star only: without it the constructor throws dfa::Error).  Frame 0
    // creates the canonical volume as fuse_canonical does; every later frame, once the solve has written its transforms into
    // the nodes and before the warp field grows, integrates that frame's depth into it through the north-star blend
    // (TsdfVolume::integrateWarped6; the node frame is frame 0's camera).  Off, nothing of this runs; on or off every other
    // output of a frame is the same, bit for bit.
    bool north_star_fuse_canonical = false;
    // Extension — the COLOURED canonical model (DESIGN.md §4.1 "Colour fusion"; needs north_star_fuse_canonical: otherwise
    // validate() throws).  Frames come with a registered colour image: operator()(depth, color) — the depth-only overload
    // throws dfa::Error while the switch is on.  Frame 0: the canonical volume gets a colour volume (TsdfVolume::createColors)
    // and frame 0's colours by one colours-only call (no nodes, every voxel where it stands: frame 0's geometry stays the
    // copied volume, bit for bit).  Every later frame: the warped integration is TsdfVolume::integrateWarped6Color instead of
    // integrateWarped6 — the same voxels, and the frame's colours fused in the same sweep, colour weights capped at
    // canonical_max_color_weight (1..255).  DynFusion::canonicalColors() samples the result at the canonical vertices.  Off,
    // nothing of this runs; on, every other output of a frame is what north_star_fuse_canonical alone gives, bit for bit.
    bool north_star_fuse_color     = false;
    int canonical_max_color_weight = 255;
    // Extension — the canonical fusion without its per-voxel search.  With fuse_canonical or north_star_fuse_canonical (alone
    // it means nothing: the constructor throws dfa::Error) the canonical volume gets a k-NN field when it is created
    // (TsdfVolume::buildKnnField over frame 0's nodes), and before every warped integrate the field is brought up to date when
    // the warp field holds more nodes than it does (TsdfVolume::appendKnnField: Warpfield::update only ever appends).  The
    // canonical volume is the one the searching calls fuse, bit for bit.  fuse_knn_field_max_bytes bounds the field's rows
    // (0: no cap): when a build or append would exceed it the field is dropped and the sequence goes on searching.  Off,
    // nothing of this runs.
    bool fuse_knn_field = false;
    size_t fuse_knn_field_max_bytes = 0;
    // Extension — the north-star data term over the visible surface of the model only (needs north_star AND model_view:
    // otherwise the constructor throws dfa::Error).  Every frame after the first, between initializeProblemInstance and the
    // solve: the canonical mesh is warped by the node transforms the solve starts from and rasterised from the frame's camera
    // (renderWarpedModel's path without the shading: getWarpedModelMaps() holds the maps afterwards), the canonical cloud is
    // warped by the same transforms on the solver's plan, and the vertices the model's surface hides
    // (kfusion::cuda::visibleVertices) take no data row in that frame's solve (NorthStarSolver::setVertexMask).
    // visibility_z_tol: how far behind the rasterised surface a vertex may lie and still count as seen, in metres; 0 = two
    // voxels of the volume's largest voxel edge — the cloud's vertices are vertices of the rasterised mesh, and the depth
    // interpolated under a vertex's pixel differs from the vertex's own by at most one cell's extent, sqrt(3) voxels.
    // Off, nothing of this runs and a frame's outputs are what they were, bit for bit.
    bool north_star_visible_only = false;
    float visibility_z_tol       = 0.f;
    // Extension — voxels no node supports are integrated where they stand (TsdfVolume::UnsupportedMode::Rigid) instead of left
    // alone, in fuse_canonical's and north_star_fuse_canonical's warped integrations, with or without fuse_knn_field (without
    // one of the two fusion switches the constructor throws dfa::Error).  Without it the canonical volume only ever changes
    // inside the support of the nodes it already has.  Off, the integrations are what they were.
    bool fuse_unsupported_rigid = false;
    // Extension — the GROWING canonical model (needs north_star AND north_star_fuse_canonical: otherwise the
    // constructor throws dfa::Error; reference mode keeps frame 0's cloud).  Frame 0: the canonical cloud is the welded vertex
    // set of the volume (MarchingCubes::runIndexed, gradient normals) instead of the triangle soup.  Every later frame, after
    // the solve and the warped integration: getCanonicalWarpedToLive() is the cloud the solve used, warped; then the cloud is
    // re-extracted from the canonical volume — runIndexed with the weight floor canonical_min_weight, normals from the
    // canonical volume, to the camera frame as frame 0's — and replaces getCanonicalFrame() (an empty extraction keeps the old
    // cloud: regrowSkippedFrames() counts those); Warpfield::update then seeds nodes where the NEW cloud, in canonical space,
    // has no support (instead of where the warped old one has none), and the nodes it appends start from the north-star blend
    // of the nodes before them, not from update's calcDQB (which composes its k neighbours' transforms: fine at the edge of
    // the support, a metre off for a seed half a model away).  With model_view the kept mesh is replaced by the same
    // extraction — getCanonicalMesh()'s views then hold until the next frame —, so north_star_visible_only tests the regrown
    // cloud against the regrown surface.  The next frame's solve, node insertion, model view and visibility test see what the
    // fusion added.  canonical_min_weight (1..65535): what one frame touched once (weight 1) stays out at the default, 2.
    // Off, nothing of this runs and a frame's outputs are what they were, bit for bit.
    bool north_star_regrow_canonical = false;
    int canonical_min_weight         = 2;
    // Extension — rigid pre-alignment of the warp field (needs north_star: otherwise the constructor throws
    // dfa::Error).  Every frame after the first, between initializeProblemInstance / the live maps and the visibility test /
    // the solve: NorthStarSolver::alignRigid estimates the rigid motion T of the model as the solve would start from it
    // against the live depth frame — rigid_prealign_iters Gauss-Newton iterations of the solve's own data term (its pixel rule,
    // its gates; 10 is KinFu's count at full resolution) — and composes T onto every node (Warpfield::composeRigid).  The
    // north-star blend is left-invariant, so the solve starts from the same field moved by T, an exact warm start of the same
    // energy, and the model view, the visibility test, the fusion and the node insertion see the aligned model.  A singular
    // system (no overlap, an empty depth frame) skips the step for that frame: rigidSkippedFrames() counts those.  Off, or
    // with rigid_prealign_iters = 0, nothing of this runs and a frame's outputs are what they were, bit for bit.
    bool north_star_rigid_prealign = false;
    int rigid_prealign_iters       = 10;
    // Extension — the same step with its whole Gauss-Newton loop on the device (dfa_rigid_align_cloud; needs
    // north_star_rigid_prealign: otherwise the constructor throws dfa::Error): a coarse-to-fine schedule over every
    // rigid_prealign_steps[l]-th vertex of the warped cloud, at most rigid_prealign_level_iters[l] iterations per level
    // (KinFu's {10, 5, 4}, coarsest first; rigid_prealign_iters is not used), a level ended early by an accepted step of
    // less than rigid_prealign_stop_rot radians AND rigid_prealign_stop_trans metres — two decades under the 1 mm depth
    // quantum, two decades above the converged step noise of the float32 loop (at most 1.5e-7 on the 80 x 60 scene of
    // tests/rigid_loop_cases.py) —, everything enqueued at once, one read-back per frame instead of one per iteration.
    // DynFusion::northStarRigidIterations() reports what ran.  Off, nothing of this runs and a frame keeps its bits.
    bool rigid_prealign_device                  = false;
    std::vector<int> rigid_prealign_steps       = {16, 4, 1};
    std::vector<int> rigid_prealign_level_iters = {4, 5, 10};
    float rigid_prealign_stop_rot               = 1e-5f;
    float rigid_prealign_stop_trans             = 1e-5f;
    // Extension — the regularisation hierarchy of DynamicFusion, which L, beta and epsilon above were declared for and the
    // reference never reads (needs north_star: otherwise the constructor throws dfa::Error).  The north-star solve's
    // regularisation graph becomes multi-level (NorthStarSolver::setRegHierarchy; the rule: dfa_solver6_set_reg_hierarchy in
    // include/dynfu_amd.h): min(L + 1, reg_level_slots.size()) levels, reg_level_slots[l] of a node's k columns for level l,
    // cells of epsilon beta^l — a node reaches a few far nodes besides its nearest ones, so a PCG iteration carries a step
    // further than one node spacing.  A slot sum above the k the solve blends (the warp field's KNN, at most 8), slots[0] < 1,
    // a negative slot, more than 8 levels, beta < 2 or epsilon <= 0 throw.  DynFusion::northStarNodeLevels() reports the
    // levels' sizes.  Off, nothing of this runs and a frame's outputs are what they were, bit for bit.
    bool north_star_reg_hierarchy    = false;
    std::vector<int> reg_level_slots = {4, 2, 2};
    int regLevels() const;  // ... min(L + 1, reg_level_slots.size())
    // every rule stated above, each switch with its prerequisites and ranges: throws dfa::Error (DFA_ERR_INVALID) naming the
    // switch at fault.  DynFusion's constructor calls it first.
    void validate() const;
};

namespace dfa {
struct StageClock;  // src/stage_clock.hpp
}

class DynFusion : public kfusion::KinFu {  // include/dynfu/dyn_fusion.hpp:45
public:
    explicit DynFusion(const DynFuParams& params);
    ~DynFusion();

    DynFuParams& params();

    // the whole per-frame sequence of the reference (dyn_fusion.cpp:48-145): pre-process the depth frame, fuse it,
    // extract the zero level set by marching cubes; frame 0 seeds the canonical frame and the warp field, later
    // frames become the live frame, the warp field is solved against it and grown.  Returns as the reference
    // does: false for the first frame, true afterwards.  The volume, its dimensions and the case tables come from
    // params().kinfuParams / the MarchingCubes passed to useMarchingCubes() (default: the library's tables).
    bool operator()(const kfusion::cuda::Depth& depth);
    // the same frame with its colour image (b, g, r, x pixels, registered to the depth frame: the same size).  With
    // north_star_fuse_color the image is fused into the canonical volume's colours; without it the image is not read.
    bool operator()(const kfusion::cuda::Depth& depth, const kfusion::cuda::Image& color);
    void useMarchingCubes(std::shared_ptr<kfusion::cuda::MarchingCubes> mc) { mc_ = mc; }
    std::shared_ptr<dynfu::Frame> getLiveFrame() { return liveFrame; }
    // reference mode: what the last frame's solve took as its canonical cloud — for every live vertex the nearest vertex of
    // the warped canonical cloud, with that vertex's normal (findCorrespondingFrame's result itself, not a copy; null before
    // the first solved frame) — and CombinedSolver::initialCost() / finalCost() of that solve
    std::shared_ptr<dynfu::Frame> getCorrespondingFrame() { return correspondingFrame; }
    double solveInitialCost() const { return solve_initial_cost_; }
    double solveFinalCost() const { return solve_final_cost_; }
    // KinFu::getMesh (kinfu.cpp:262): the marching-cubes triangles of the last frame, KinFu::convertToMesh's layout
    // (built on first use: one small vector per triangle is not something every frame should pay for)
    std::shared_ptr<dfa::PolygonMesh> getMesh();
    // lets go of the mesh getMesh() built (one small vector per triangle: freeing them takes milliseconds, which a
    // caller may want outside its timed region; the next frame would do it otherwise)
    void dropMesh() { mesh_.reset(); }
    // model_view: the canonical model, warped to the live frame and seen from the current camera (getCameraPose(), the
    // model being in the volume's frame; the origin in north-star mode, where the model already is in the camera frame), shaded with
    // params().kinfuParams.light_pose.  Flags and image sizes are KinFu::renderImage's: 2 the normal colours, 3 the Phong
    // view and the normal colours side by side (2 * cols wide), anything else the Phong view.  Throws dfa::Error when
    // model_view is off or before frame 0.
    void renderWarpedModel(kfusion::cuda::Image& image, int flag = 0);
    // what renderWarpedModel rasterises: the canonical mesh's vertices and normals (one per vertex of getCanonicalMesh())
    // carried through the current warp field by the mode's blend.  Throws as renderWarpedModel does.
    std::shared_ptr<dynfu::Frame> warpCanonicalMesh();
    // the point and normal maps of the last renderWarpedModel: the visible surface of the warped model, camera frame,
    // NaN where nothing is seen (empty before the first call)
    struct ModelMaps {
        kfusion::cuda::Cloud points;
        kfusion::cuda::Normals normals;
    };
    ModelMaps getWarpedModelMaps() const { return ModelMaps{model_points_, model_normals_}; }
    // the canonical mesh kept by frame 0 (empty before it, or with model_view off): float4 vertices in the frame of the
    // canonical cloud, three indices per triangle; views that stay valid while this object lives
    kfusion::cuda::MarchingCubes::IndexedMesh getCanonicalMesh() const { return canonical_mesh_; }
    // north-star mode: energy before / after the last frame's solve and the data rows that found an association
    double northStarInitialCost() const { return report_.initial_cost; }
    double northStarFinalCost() const { return report_.final_cost; }
    long long northStarValidRows() const { return report_.valid_rows; }
    // ... the PCG iterations of that solve, over all its Gauss-Newton iterations, and the normal equations it solved
    int northStarPcgIterations() const { return report_.pcg_iters; }
    int northStarGnSolves() const { return report_.gn_solves; }
    // north_star_rigid_prealign: the last frame's rigid estimate — it maps the model, warped by the transforms that frame's
    // solve would have started from, into the live camera's frame (the identity when the step was skipped, or is off) —, the
    // vertices that took a row in its first and its last iteration, and the frames whose system was singular
    dfa::Affine3f northStarRigidPose() const { return report_.rigid_pose; }
    struct RigidMatched {
        long long first, last;
    };
    RigidMatched northStarRigidMatched() const { return RigidMatched{report_.rigid_matched_first, report_.rigid_matched_last}; }
    int rigidSkippedFrames() const { return report_.rigid_skipped; }
    // rigid_prealign_device: the iterations each level of the schedule ran in the last frame (empty before it, or with the
    // switch off)
    std::vector<int> northStarRigidIterations() const { return report_.rigid_iters_run; }
    // north_star_reg_hierarchy: how many nodes of the last frame's graph have level 0, 1, ... (one entry per level used;
    // empty before the first solved frame, or with the switch off), and the levels themselves, one per node
    std::vector<int> northStarNodeLevels() const { return report_.reg_level_counts; }
    std::vector<int> northStarNodeLevelOfEach() const { return report_.reg_node_levels; }
    // north_star_visible_only: canonical vertices the last frame's solve could take data rows from (one small read from the
    // device); -1 before the first such frame, or with the switch off
    long long northStarVisibleVertices() const;
    // ... and that frame's flags themselves, on the device: one byte per vertex of the canonical cloud that frame's solve
    // ran over, non-zero = seen (empty before the first such frame, or with the switch off)
    dfa::DeviceArray<unsigned char> northStarVisibleFlags() const { return visible_flags_; }
    // north-star mode: the live vertex and normal maps the last solved frame's solve (and pre-alignment) read, camera frame
    // (empty before the first such frame).  What a test needs to state the pre-alignment and the solve's initial cost from the
    // frame's own inputs (tests/cpp/test_host_northstar_frames.cpp)
    struct LiveMaps {
        kfusion::cuda::Cloud points;
        kfusion::cuda::Normals normals;
    };
    LiveMaps northStarLiveMaps() const { return LiveMaps{live_points_, live_normals_}; }

    void init(dfa::PointCloud<dfa::PointXYZ>& canonicalVertices, dfa::PointCloud<dfa::Normal>& canonicalNormals);
    void initCanonicalFrame(dfa::PointCloud<dfa::PointXYZ>& vertices, dfa::PointCloud<dfa::Normal>& normals);
    void addLiveFrame(int frameID, dfa::PointCloud<dfa::PointXYZ>& vertices, dfa::PointCloud<dfa::Normal>& normals);
    // the same two steps on frames that may live in HBM (what operator() uses: nothing is staged through the host)
    void initFromFrame(std::shared_ptr<dynfu::Frame> frame);
    void addLiveFrame(int frameID, std::shared_ptr<dynfu::Frame> frame);
    void warpCanonicalToLiveOpt(dfa::Affine3f affine);
    std::shared_ptr<dynfu::Frame> getCanonicalWarpedToLive();
    // the canonical cloud the NEXT frame's solve starts from (frame 0's; with north_star_regrow_canonical the last
    // re-extraction), and its size
    std::shared_ptr<dynfu::Frame> getCanonicalFrame() { return canonicalFrame; }
    size_t canonicalVertexCount() const { return canonicalFrame ? canonicalFrame->size() : 0; }
    // north_star_fuse_color: one b, g, r, a per vertex of getCanonicalFrame() (a = 0: the colour volume holds nothing around
    // the vertex), on the device — sampled after the frame's regrow when north_star_regrow_canonical is on, else when asked
    // for.  With model_view, canonicalMeshColors() is the same for the vertices of getCanonicalMesh().  Both throw
    // dfa::Error with the switch off or before frame 0.
    dfa::DeviceArray<kfusion::RGB> canonicalColors();
    dfa::DeviceArray<kfusion::RGB> canonicalMeshColors();
    // north_star_regrow_canonical: frames whose re-extraction was empty (the cloud before it was kept)
    int regrowSkippedFrames() const { return report_.regrow_skipped; }

    // private in the reference (dyn_fusion.hpp:86-89); public here so that it can be tested alone
    std::shared_ptr<dynfu::Frame> findCorrespondingFrame(dfa::PointCloud<dfa::PointXYZ> canonicalVertices,
                                                         dfa::PointCloud<dfa::Normal> canonicalNormals,
                                                         dfa::PointCloud<dfa::PointXYZ> liveVertices);
    std::shared_ptr<dynfu::Frame> findCorrespondingFrame(std::shared_ptr<dynfu::Frame> canonical,
                                                         std::shared_ptr<dynfu::Frame> live);

    // dists -> clear -> integrate of operator() (dyn_fusion.cpp:58, :108-115) as one fused sweep
    void fuse(const kfusion::cuda::Depth& depth, kfusion::cuda::TsdfVolume& volume, const dfa::Affine3f& camera_pose);

    // the iteration budget warpCanonicalToLiveOpt hands to the solver (dyn_fusion.cpp:183-189)
    CombinedSolverParameters solverParams;
    // vertices per deformation node at seeding (dyn_fusion.cpp:151)
    int nodeStep = 128;

    std::shared_ptr<Warpfield> getWarpfield() { return warpfield; }
    // fuse_canonical / north_star_fuse_canonical: the canonical volume (null before frame 0, or with the switch off)
    std::shared_ptr<kfusion::cuda::TsdfVolume> canonicalVolume() { return canonical_volume_; }

private:
    DynFuParams dynfuParams;
    std::shared_ptr<dynfu::Frame> canonicalFrame;
    std::shared_ptr<dynfu::Frame> canonicalFrameWarpedToLive;
    std::shared_ptr<dynfu::Frame> liveFrame;
    std::shared_ptr<dynfu::Frame> correspondingFrame;  // kept for getCorrespondingFrame(): the next solved frame replaces it
    double solve_initial_cost_ = 0.0, solve_final_cost_ = 0.0;
    std::shared_ptr<Warpfield> warpfield;
    std::shared_ptr<dfa::PolygonMesh> mesh_;
    // the last frame's marching-cubes output (:76 / :122): in HBM (a view of mc_buffer_, valid until the next frame),
    // downloaded when getMesh() asks for it
    dfa::DeviceArray<kfusion::cuda::MarchingCubes::PointType> mc_buffer_, mesh_source_;
    std::vector<dfa::PointXYZ> mesh_triangles_;
    bool mesh_downloaded_ = false;
    // what the northStar* / *SkippedFrames accessors read: the numbers of the last north-star frame that ran the stage (a
    // frame resets nothing it does not write), the skip counters over all frames
    struct FrameReport {
        double initial_cost = 0.0, final_cost = 0.0;
        long long valid_rows = 0;
        int pcg_iters = 0, gn_solves = 0;
        dfa::Affine3f rigid_pose;  // north_star_rigid_prealign
        long long rigid_matched_first = 0, rigid_matched_last = 0;
        int rigid_skipped = 0;
        std::vector<int> rigid_iters_run;
        std::vector<int> reg_level_counts, reg_node_levels;  // north_star_reg_hierarchy
        dfa::DeviceArray<int> visible_count;                 // north_star_visible_only: on the device
        bool visible_counted = false;
        int regrow_skipped = 0;  // north_star_regrow_canonical
    } report_;
    void seedNodes(const std::vector<dfa::PointXYZ>& canonicalVertices);
    // vertices of the volume's zero level set as a point cloud (dyn_fusion.cpp:73-88 / :119-134), device-resident
    std::shared_ptr<dynfu::Frame> extractSurface(int frame_id, bool with_normals);
    // operator() in north-star mode, and its stages in the order they run (dyn_fusion_northstar.cpp): each
    // reads its switch and returns at once when it is off
    bool frame(const kfusion::cuda::Depth& depth);  // operator()'s body, either overload
    const kfusion::cuda::Image* frame_color_ = nullptr;  // north_star_fuse_color: this frame's colour image, while the frame runs
    void fuseFirstFrameColors();                         // ... frame 0: the canonical volume's colours, by one colours-only call
    void sampleModelColors();                            // ... after a regrow: the new cloud's (and mesh's) colours
    dfa::DeviceArray<kfusion::RGB> cloud_colors_, mesh_colors_;
    bool model_colors_current_ = false;
    bool northStarFrame(const kfusion::cuda::Depth& depth);
    bool northStarFirstFrame();
    void buildNorthStarProblem(NorthStarSolver& solver, dfa::StageClock& clk);
    bool prealignRigid(NorthStarSolver& solver, dfa::StageClock& clk);  // true: it ran, and live_points_ / live_normals_ are this frame's
    void maskHiddenVertices(NorthStarSolver& solver, dfa::StageClock& clk);
    void solveNorthStar(NorthStarSolver& solver, dfa::StageClock& clk);
    void fuseThroughSolvedField(dfa::StageClock& clk);
    void growModelAndField(dfa::StageClock& clk);
    void volumeToCamera(float aff[12]);  // camera_pose^-1 * volume_pose, the camera at the origin: the inverse of what integrate() applies
    std::shared_ptr<kfusion::cuda::TsdfVolume> canonical_volume_;  // fuse_canonical, north_star_fuse_canonical
    bool knn_field_dropped_ = false;  // fuse_knn_field: the field exceeded fuse_knn_field_max_bytes and is not tried again
    void createCanonicalVolume();  // frame 0: a copy of the live volume
    void syncKnnField();           // fuse_knn_field: the canonical volume's field built, or appended to, for the nodes as they are
    kfusion::cuda::Cloud live_points_;
    kfusion::cuda::Normals live_normals_;
    // model_view: the canonical mesh (frame 0) as a frame for Warpfield::warpToLive and as float4 vertices + indices, the
    // buffers behind them, and what the last renderWarpedModel made
    void keepCanonicalMesh(const float* to_canonical_frame /* 12 floats, or null: the volume's frame */);
    // ... the kept mesh and its frame replaced (frame 0 and every frame of north_star_regrow_canonical): the view's plan rebuilds
    void setCanonicalMesh(std::shared_ptr<dynfu::Frame> frame, const kfusion::cuda::MarchingCubes::IndexedMesh& mesh);
    // the welded mesh of a volume at a weight floor (in mesh_vertex_buffer_ / mesh_index_buffer_) and its vertices with
    // gradient normals as a frame; null when there is no surface.  keepCanonicalMesh's extraction, and the regrown model's
    std::shared_ptr<dynfu::Frame> extractWeldedModel(const kfusion::cuda::TsdfVolume& volume, int min_weight, const float* to_frame,
                                                     kfusion::cuda::MarchingCubes::IndexedMesh& mesh);
    kfusion::cuda::TsdfVolume::UnsupportedMode unsupportedMode() const;  // fuse_unsupported_rigid
    // north_star_regrow_canonical: the nodes appended since there were `nodes_before` start from the north-star blend of the
    // nodes before them (Warpfield::update's calcDQB composes its k neighbours' transforms: see dyn_fusion_northstar.cpp)
    void startNewNodesFromBlend(size_t nodes_before);
    std::shared_ptr<dynfu::Frame> canonical_mesh_frame_;
    kfusion::cuda::MarchingCubes::IndexedMesh canonical_mesh_;
    dfa::DeviceArray<kfusion::cuda::MarchingCubes::PointType> mesh_vertex_buffer_, warped_vertices_;
    dfa::DeviceArray<int> mesh_index_buffer_;
    dfa::DeviceArray<dfa::Normal> warped_normals_;
    dfa::DeviceArray<uint64_t> model_zbuffer_;
    // north-star mode: a dfa_solver6 plan over (nodes, mesh vertices) that only ever warps (dyn_fusion_model_view.cpp)
    class MeshWarpPlan;
    std::shared_ptr<MeshWarpPlan> mesh_warp_;
    kfusion::cuda::Cloud model_points_;
    kfusion::cuda::Normals model_normals_;
    // the warped mesh as float4 vertices / normals rasterised into model_points_ / model_normals_ / model_zbuffer_
    // (renderWarpedModel's first half; north_star_visible_only runs it alone)
    void rasterizeWarpedModel();
    // north_star_visible_only: the frame's flags (one per canonical vertex), on the device
    dfa::DeviceArray<unsigned char> visible_flags_;
};

// DynFuApp::execute of the reference's demo (src/apps/demo.cpp:68-124) without its windows and command line: every
// depth PNG of <dir>/depth in lexicographic order is uploaded and handed to DynFusion::operator(); whenever that
// returns true, <dir>/out/pcl_canonical_to_live<i>.pcd and <dir>/out/<i>_tsdf_mesh.vtk are written (demo.cpp:21-37).
// <dir>/color must exist and hold at least as many files (the demo reads them for display only; they are not decoded
// here).  max_frames < 0: all.
struct SequenceReport {
    int frames = 0, saved = 0;
    double dynfu_ms = 0;  // time inside DynFusion::operator() (the demo's SampledScopeTime)
    std::vector<double> frame_ms;  // ... per frame
};
SequenceReport runSequence(DynFusion& dynfu, const std::string& dir, int max_frames = -1);
