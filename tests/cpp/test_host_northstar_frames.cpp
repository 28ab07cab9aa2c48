// test_host_northstar_frames.cpp — DynFusion::operator() in north-star mode (DynFuParams::north_star), observed
// frame by frame.
//   test_host_northstar_frames            the tests below (no GPU: the parameter file and the frame files)
//   test_host_northstar_frames dump DIR   GPU: run DynFusion over the frames the pytest wrapper wrote into DIR and write what every
//                                         frame left behind, unpitched (tests/test_gpu_northstar_frames.py compares it stage by
//                                         stage with tests/northstar_statement.py).  The mode observes only: it reads the public
//                                         accessors and KinFu's protected members and computes nothing of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <dynfu/dyn_fusion.hpp>

#include "minitest.hpp"

using namespace kfusion;

namespace {
// what a case sets: DynFuParams, and the public knobs beside it
struct Case {
    DynFuParams p = DynFuParams::defaultParams();
    int frames    = 0;
    int nodeStep  = 128;
    int warp_knn  = KNN;  // Warpfield::setKnn, once frame 0 has created the field
};

std::string g9(float v) {  // nine significant digits carry a float32 exactly
    char buf[32];
    std::snprintf(buf, sizeof buf, "%.9g", v);
    return buf;
}

void read_ints(std::istream& in, std::vector<int>& v) {
    int n = 0;
    in >> n;
    if (n < 0 || n > 64) throw dfa::Error(1, "params: bad list length");
    v.assign((size_t)n, 0);
    for (int& x : v) in >> x;
}
std::string ints(const std::vector<int>& v) {
    std::string s = std::to_string(v.size());
    for (int x : v) s += " " + std::to_string(x);
    return s;
}

// params.txt: `key value ...` per line, keys as the members of KinFuParams / DynFuParams / NorthStarParameters (and frames,
// nodeStep, warp_knn); an unknown key is an error
Case parse_params(std::istream& in) {
    Case c;
    KinFuParams& k          = c.p.kinfuParams;
    DynFuParams& d          = c.p;
    NorthStarParameters& ns = c.p.northStarParams;
    std::string key;
    while (in >> key) {
        if (key == "cols") in >> k.cols;
        else if (key == "rows") in >> k.rows;
        else if (key == "intr") in >> k.intr.fx >> k.intr.fy >> k.intr.cx >> k.intr.cy;
        else if (key == "volume_dims") in >> k.volume_dims[0] >> k.volume_dims[1] >> k.volume_dims[2];
        else if (key == "volume_size") in >> k.volume_size[0] >> k.volume_size[1] >> k.volume_size[2];
        else if (key == "volume_pose") {
            for (float& v : k.volume_pose.R) in >> v;
            for (float& v : k.volume_pose.t) in >> v;
        } else if (key == "bilateral") in >> k.bilateral_sigma_depth >> k.bilateral_sigma_spatial >> k.bilateral_kernel_size;
        else if (key == "icp_truncate_depth_dist") in >> k.icp_truncate_depth_dist;
        else if (key == "tsdf_trunc_dist") in >> k.tsdf_trunc_dist;
        else if (key == "tsdf_max_weight") in >> k.tsdf_max_weight;
        else if (key == "gradient_delta_factor") in >> k.gradient_delta_factor;
        else if (key == "tukeyOffset") in >> d.tukeyOffset;
        else if (key == "lambda") in >> d.lambda;
        else if (key == "psi_data") in >> d.psi_data;
        else if (key == "psi_reg") in >> d.psi_reg;
        else if (key == "L") in >> d.L;
        else if (key == "beta") in >> d.beta;
        else if (key == "epsilon") in >> d.epsilon;
        else if (key == "mesh_normals") in >> d.mesh_normals;
        else if (key == "north_star") in >> d.north_star;
        else if (key == "model_view") in >> d.model_view;
        else if (key == "north_star_fuse_canonical") in >> d.north_star_fuse_canonical;
        else if (key == "north_star_fuse_color") in >> d.north_star_fuse_color;
        else if (key == "canonical_max_color_weight") in >> d.canonical_max_color_weight;
        else if (key == "fuse_knn_field") in >> d.fuse_knn_field;
        else if (key == "north_star_visible_only") in >> d.north_star_visible_only;
        else if (key == "fuse_unsupported_rigid") in >> d.fuse_unsupported_rigid;
        else if (key == "north_star_regrow_canonical") in >> d.north_star_regrow_canonical;
        else if (key == "canonical_min_weight") in >> d.canonical_min_weight;
        else if (key == "north_star_rigid_prealign") in >> d.north_star_rigid_prealign;
        else if (key == "rigid_prealign_iters") in >> d.rigid_prealign_iters;
        else if (key == "rigid_prealign_device") in >> d.rigid_prealign_device;
        else if (key == "rigid_prealign_steps") read_ints(in, d.rigid_prealign_steps);
        else if (key == "rigid_prealign_level_iters") read_ints(in, d.rigid_prealign_level_iters);
        else if (key == "rigid_prealign_stop") in >> d.rigid_prealign_stop_rot >> d.rigid_prealign_stop_trans;
        else if (key == "north_star_reg_hierarchy") in >> d.north_star_reg_hierarchy;
        else if (key == "reg_level_slots") read_ints(in, d.reg_level_slots);
        else if (key == "numIter") in >> ns.numIter;
        else if (key == "gnIter") in >> ns.gnIter;
        else if (key == "linearIter") in >> ns.linearIter;
        else if (key == "distThresh") in >> ns.distThresh;
        else if (key == "cosThresh") in >> ns.cosThresh;
        else if (key == "damping") in >> ns.damping;
        else if (key == "gnTol") in >> ns.gnTol;
        else if (key == "frames") in >> c.frames;
        else if (key == "nodeStep") in >> c.nodeStep;
        else if (key == "warp_knn") in >> c.warp_knn;
        else throw dfa::Error(1, "params: unknown key " + key);
        if (!in) throw dfa::Error(1, "params: bad value of " + key);
    }
    d.intr = k.intr;
    return c;
}

std::string format_params(const Case& c) {
    const KinFuParams& k          = c.p.kinfuParams;
    const DynFuParams& d          = c.p;
    const NorthStarParameters& ns = c.p.northStarParams;
    std::ostringstream o;
    o << "cols " << k.cols << "\nrows " << k.rows << "\nintr " << g9(k.intr.fx) << " " << g9(k.intr.fy) << " " << g9(k.intr.cx) << " "
      << g9(k.intr.cy) << "\nvolume_dims " << k.volume_dims[0] << " " << k.volume_dims[1] << " " << k.volume_dims[2] << "\nvolume_size "
      << g9(k.volume_size[0]) << " " << g9(k.volume_size[1]) << " " << g9(k.volume_size[2]) << "\nvolume_pose";
    for (float v : k.volume_pose.R) o << " " << g9(v);
    for (float v : k.volume_pose.t) o << " " << g9(v);
    o << "\nbilateral " << g9(k.bilateral_sigma_depth) << " " << g9(k.bilateral_sigma_spatial) << " " << k.bilateral_kernel_size
      << "\nicp_truncate_depth_dist " << g9(k.icp_truncate_depth_dist) << "\ntsdf_trunc_dist " << g9(k.tsdf_trunc_dist)
      << "\ntsdf_max_weight " << k.tsdf_max_weight << "\ngradient_delta_factor " << g9(k.gradient_delta_factor) << "\ntukeyOffset "
      << g9(d.tukeyOffset) << "\nlambda " << g9(d.lambda) << "\npsi_data " << g9(d.psi_data) << "\npsi_reg " << g9(d.psi_reg) << "\nL " << d.L
      << "\nbeta " << d.beta << "\nepsilon " << g9(d.epsilon) << "\nmesh_normals " << d.mesh_normals << "\nnorth_star " << d.north_star
      << "\nmodel_view " << d.model_view << "\nnorth_star_fuse_canonical " << d.north_star_fuse_canonical << "\nnorth_star_fuse_color "
      << d.north_star_fuse_color << "\ncanonical_max_color_weight " << d.canonical_max_color_weight << "\nfuse_knn_field " << d.fuse_knn_field
      << "\nnorth_star_visible_only " << d.north_star_visible_only << "\nfuse_unsupported_rigid " << d.fuse_unsupported_rigid
      << "\nnorth_star_regrow_canonical " << d.north_star_regrow_canonical << "\ncanonical_min_weight " << d.canonical_min_weight
      << "\nnorth_star_rigid_prealign " << d.north_star_rigid_prealign << "\nrigid_prealign_iters " << d.rigid_prealign_iters
      << "\nrigid_prealign_device " << d.rigid_prealign_device << "\nrigid_prealign_steps " << ints(d.rigid_prealign_steps)
      << "\nrigid_prealign_level_iters " << ints(d.rigid_prealign_level_iters) << "\nrigid_prealign_stop " << g9(d.rigid_prealign_stop_rot)
      << " " << g9(d.rigid_prealign_stop_trans) << "\nnorth_star_reg_hierarchy " << d.north_star_reg_hierarchy << "\nreg_level_slots "
      << ints(d.reg_level_slots) << "\nnumIter " << ns.numIter << "\ngnIter " << ns.gnIter << "\nlinearIter " << ns.linearIter
      << "\ndistThresh " << g9(ns.distThresh) << "\ncosThresh " << g9(ns.cosThresh) << "\ndamping " << g9(ns.damping) << "\ngnTol "
      << g9(ns.gnTol) << "\nframes " << c.frames << "\nnodeStep " << c.nodeStep << "\nwarp_knn " << c.warp_knn << "\n";
    return o.str();
}

// a raw frame file of exactly n elements
template <class T>
std::vector<T> read_frame(const std::string& path, size_t n) {
    std::vector<T> px(n);
    std::ifstream f(path, std::ios::binary);
    if (!f) throw dfa::Error(1, "no frame file " + path);
    f.read((char*)px.data(), (std::streamsize)(n * sizeof(T)));
    if (!f || f.peek() != std::ifstream::traits_type::eof()) throw dfa::Error(1, "frame file " + path + " has the wrong size");
    return px;
}
}  // namespace

TEST(NorthStarFramesTest, AParamsFileRoundTrips) {
    Case c;
    c.p.kinfuParams.cols = 96, c.p.kinfuParams.rows = 72;
    c.p.kinfuParams.intr        = Intr(78.75f, 78.75f, 47.5f, 35.5f);
    c.p.kinfuParams.volume_dims = Vec3i::all(64);
    c.p.kinfuParams.volume_pose.t[0] = -1.1f, c.p.kinfuParams.volume_pose.R[1] = 0.1f;
    c.p.epsilon = 0.123456789f, c.p.north_star = true, c.p.north_star_reg_hierarchy = true, c.p.reg_level_slots = {3, 1};
    c.p.rigid_prealign_steps = {8, 1}, c.p.rigid_prealign_level_iters = {3, 7}, c.p.canonical_max_color_weight = 3;
    c.p.northStarParams.cosThresh = 0.3f, c.frames = 4, c.nodeStep = 37, c.warp_knn = 4;
    const std::string text = format_params(c);
    std::istringstream in(text);
    const Case back = parse_params(in);
    ASSERT_EQ(format_params(back), text);
    ASSERT_EQ(back.p.kinfuParams.cols, 96);
    ASSERT_TRUE(back.p.epsilon == 0.123456789f && back.p.kinfuParams.volume_pose.t[0] == -1.1f && back.p.intr.fx == 78.75f);
    ASSERT_TRUE((back.p.reg_level_slots == std::vector<int>{3, 1}) && (back.p.rigid_prealign_level_iters == std::vector<int>{3, 7}));
    ASSERT_TRUE(back.p.north_star && back.p.north_star_reg_hierarchy && !back.p.north_star_fuse_color && back.warp_knn == 4 && back.nodeStep == 37);
    bool threw = false;
    try {
        std::istringstream bad("cols 96\nno_such_key 1\n");
        parse_params(bad);
    } catch (const dfa::Error&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
}

TEST(NorthStarFramesTest, AMissingOrShortFrameFileIsAnError) {
    const char* tmp = std::getenv("TMPDIR");
    const std::string path = std::string(tmp ? tmp : "/tmp") + "/northstar_frames_test_" + std::to_string((long)std::rand()) + ".bin";
    bool threw = false;
    try {
        read_frame<unsigned short>(path, 12);
    } catch (const dfa::Error&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
    const unsigned short px[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    std::ofstream(path, std::ios::binary).write((const char*)px, sizeof px);
    ASSERT_TRUE(read_frame<unsigned short>(path, 12)[11] == 12);
    threw = false;
    try {
        read_frame<unsigned short>(path, 11);  // longer than asked for
    } catch (const dfa::Error&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
    threw = false;
    try {
        read_frame<unsigned short>(path, 13);  // shorter
    } catch (const dfa::Error&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
    std::remove(path.c_str());
}

// ---- dump mode
namespace {
template <class T>
void write_raw(const std::string& path, const T* data, size_t n) {
    std::ofstream f(path, std::ios::binary);
    if (n) f.write((const char*)data, (std::streamsize)(n * sizeof(T)));
    if (!f) throw dfa::Error(1, "dump: cannot write " + path);
}
template <class T>
void write_image(const std::string& path, const dfa::DeviceArray2D<T>& img) {
    std::vector<T> host;
    int cols = 0;
    if (!img.empty()) img.download(host, cols);
    write_raw(path, host.data(), host.size());
}
template <class T>
void write_array(const std::string& path, const dfa::DeviceArray<T>& a) {
    std::vector<T> host;
    if (a.size()) a.download(host);
    write_raw(path, host.data(), host.size());
}
void write_frame_cloud(const std::string& prefix, const std::shared_ptr<dynfu::Frame>& frame) {
    dfa::DeviceArray<float> v3, n3;
    size_t n = 0;
    if (frame && frame->size()) frame->deviceArrays(v3, n3), n = frame->size();
    std::vector<float> v, nn;
    if (n) v3.download(v), n3.download(nn);
    write_raw(prefix + "_v.bin", v.data(), std::min(v.size(), 3 * n));
    write_raw(prefix + "_n.bin", nn.data(), std::min(nn.size(), 3 * n));
}

// reads the protected members of KinFu, as DynFusion does
struct Probe : DynFusion {
    using DynFusion::DynFusion;
    void write_frame(const std::string& dir, int i, bool result) {
        const std::string f  = dir + "/f" + std::to_string(i) + "_";
        const DynFuParams& d = params();
        write_image(f + "dists.bin", dists_);
        write_image(f + "depth0.bin", curr_.depth_pyr[0]);
        const LiveMaps live = northStarLiveMaps();
        write_image(f + "live_points.bin", live.points);
        write_image(f + "live_normals.bin", live.normals);
        std::vector<uint32_t> voxels((size_t)tsdf().getDims()[0] * tsdf().getDims()[1] * tsdf().getDims()[2]);
        const cuda::TsdfVolume& live_volume = tsdf();  // (the const handle: the volume's occupancy map stays trusted)
        live_volume.data().download(voxels.data(), voxels.size() * sizeof(uint32_t));
        write_raw(f + "live_volume.bin", voxels.data(), voxels.size());
        // the nodes
        std::vector<float> pos, w, dq;
        getWarpfield()->hostArrays(pos, w, dq);
        write_raw(f + "node_pos.bin", pos.data(), pos.size());
        write_raw(f + "node_w.bin", w.data(), w.size());
        write_raw(f + "node_dq.bin", dq.data(), dq.size());
        const std::vector<int> levels = northStarNodeLevelOfEach(), level_counts = northStarNodeLevels(), iters = northStarRigidIterations();
        write_raw(f + "node_levels.bin", levels.data(), levels.size());
        // the rigid step
        float pose[12];
        northStarRigidPose().to12(pose);
        write_raw(f + "rigid_pose.bin", pose, 12);
        write_raw(f + "rigid_iters.bin", iters.data(), iters.size());
        // visibility
        write_array(f + "visible_flags.bin", northStarVisibleFlags());
        const ModelMaps maps = getWarpedModelMaps();
        write_image(f + "model_points.bin", maps.points);
        write_image(f + "model_normals.bin", maps.normals);
        // the clouds and the mesh
        write_frame_cloud(f + "warped", getCanonicalWarpedToLive());
        write_frame_cloud(f + "canonical", getCanonicalFrame());
        const cuda::MarchingCubes::IndexedMesh mesh = getCanonicalMesh();
        write_array(f + "mesh_v.bin", mesh.vertices);
        write_array(f + "mesh_i.bin", mesh.indices);
        // the canonical volume, its colours and its field
        int field_nodes = -1;
        std::vector<uint32_t> canon, colors;
        if (const std::shared_ptr<const cuda::TsdfVolume> cv = canonicalVolume()) {
            canon.resize(voxels.size());
            cv->data().download(canon.data(), canon.size() * sizeof(uint32_t));
            if (cv->colors()) {
                colors.resize(voxels.size());
                dfa::DeviceMemory((void*)cv->colors(), colors.size() * sizeof(uint32_t)).download(colors.data(), colors.size() * sizeof(uint32_t));
            }
            field_nodes = cv->knnFieldNodes();
        }
        write_raw(f + "canonical_volume.bin", canon.data(), canon.size());
        write_raw(f + "color_volume.bin", colors.data(), colors.size());
        if (d.north_star_fuse_color) {
            write_array(f + "canonical_colors.bin", canonicalColors());
            write_array(f + "mesh_colors.bin", d.model_view ? canonicalMeshColors() : dfa::DeviceArray<RGB>());
        } else {
            write_raw(f + "canonical_colors.bin", (const RGB*)nullptr, 0);
            write_raw(f + "mesh_colors.bin", (const RGB*)nullptr, 0);
        }
        const RigidMatched m = northStarRigidMatched();
        char buf[512];
        std::snprintf(buf, sizeof buf,
                      "result %d\ncounter %d\nnodes %zu\nknn %d\nrigid_matched_first %lld\nrigid_matched_last %lld\nrigid_skipped %d\n"
                      "visible_count %lld\ninitial_cost %.17g\nfinal_cost %.17g\nvalid_rows %lld\npcg_iters %d\ngn_solves %d\n"
                      "knn_field_nodes %d\nregrow_skipped %d\ncanonical_vertices %zu\n",
                      result ? 1 : 0, frame_counter_, w.size(), northStarKnn(getWarpfield()->getKnn()), m.first, m.last, rigidSkippedFrames(),
                      northStarVisibleVertices(), northStarInitialCost(), northStarFinalCost(), northStarValidRows(), northStarPcgIterations(),
                      northStarGnSolves(), field_nodes, regrowSkippedFrames(), canonicalVertexCount());
        std::ofstream status(f + "status.txt");
        status << buf << "level_counts " << ints(level_counts) << "\n";
        if (!status) throw dfa::Error(1, "dump: cannot write " + f + "status.txt");
    }
    void write_derived(const std::string& dir) {
        const Vec3f v = tsdf().getVoxelSize();
        std::ofstream(dir + "/derived.txt") << g9(tsdf().getTruncDist()) << " " << g9(v[0]) << " " << g9(v[1]) << " " << g9(v[2]) << " "
                                            << tsdf().getMaxWeight() << "\n";
    }
};

int dump(const std::string& dir) {
    std::ifstream in(dir + "/params.txt");
    if (!in) throw dfa::Error(1, "dump: no params.txt in " + dir);
    const Case c          = parse_params(in);
    const KinFuParams& k  = c.p.kinfuParams;
    const size_t pixels   = (size_t)k.cols * k.rows;
    Probe dynfu(c.p);
    dynfu.nodeStep = c.nodeStep;
    dynfu.write_derived(dir);
    for (int i = 0; i < c.frames; ++i) {
        cuda::Depth depth;
        depth.upload(read_frame<unsigned short>(dir + "/depth_" + std::to_string(i) + ".bin", pixels), k.cols);
        bool result;
        if (c.p.north_star_fuse_color) {
            cuda::Image color;
            color.upload(read_frame<RGB>(dir + "/color_" + std::to_string(i) + ".bin", pixels), k.cols);
            result = dynfu(depth, color);
        } else {
            result = dynfu(depth);
        }
        if (i == 0) dynfu.getWarpfield()->setKnn(c.warp_knn);  // frame 0 created the field
        dynfu.write_frame(dir, i, result);
    }
    std::printf("dumped %d frames\n", c.frames);
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "dump")) {
        try {
            return dump(argv[2]);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "dump: %s\n", e.what());
            return 2;
        }
    }
    return mt::run_all(argc, argv);
}
