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

#include "frames_io.hpp"
#include "minitest.hpp"

using namespace kfusion;
using namespace frames_io;  // the parameter file and the raw files: frames_io.hpp, shared with test_host_dynfusion_frames.cpp

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
