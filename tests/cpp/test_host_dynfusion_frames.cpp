// test_host_dynfusion_frames.cpp — DynFusion::operator() in reference mode (north_star = 0: the port of the reference's
// dyn_fusion.cpp:48-145), observed frame by frame.
//   test_host_dynfusion_frames            the tests below (no GPU: the parameter file with the reference-mode keys)
//   test_host_dynfusion_frames params DIR no GPU: read DIR/params.txt as `dump` does and print it back (the writer of
//                                         tests/dynfusion_cases.py against this reader)
//   test_host_dynfusion_frames dump DIR   GPU: run DynFusion over the frames the pytest wrapper wrote into DIR and write what every
//                                         frame left behind, unpitched (tests/test_gpu_dynfusion_frames.py compares it stage by
//                                         stage with tests/dynfusion_statement.py).  The mode observes only: it reads the public
//                                         accessors and KinFu's protected members and computes nothing of its own.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <dynfu/dyn_fusion.hpp>

#include "frames_io.hpp"
#include "minitest.hpp"

using namespace kfusion;
using namespace frames_io;

TEST(DynFusionFramesTest, AParamsFileWithTheReferenceModeKeysRoundTrips) {
    Case c;
    c.p.kinfuParams.cols = 96, c.p.kinfuParams.rows = 72;
    c.p.kinfuParams.intr        = Intr(78.75f, 78.75f, 47.5f, 35.5f);
    c.p.kinfuParams.volume_dims = Vec3i::all(64);
    c.p.kinfuParams.volume_pose.t[2] = 0.8f;
    c.p.epsilon = 0.0625f, c.p.fuse_canonical = true, c.p.fuse_knn_field = true, c.p.fuse_unsupported_rigid = true, c.p.mesh_normals = true;
    c.frames = 4, c.nodeStep = 41, c.warp_knn = 4;
    c.solver_numIter = 1, c.solver_nonLinearIter = 3, c.solver_linearIter = 64;
    const std::string text = format_params(c, Keys::Reference);
    std::istringstream in(text);
    const Case back = parse_params(in, Keys::Reference);
    ASSERT_EQ(format_params(back, Keys::Reference), text);
    ASSERT_TRUE(back.p.fuse_canonical && back.p.fuse_knn_field && back.p.fuse_unsupported_rigid && !back.p.north_star);
    ASSERT_TRUE(back.solver_numIter == 1 && back.solver_nonLinearIter == 3 && back.solver_linearIter == 64);
    ASSERT_TRUE(back.p.epsilon == 0.0625f && back.nodeStep == 41 && back.warp_knn == 4 && back.p.intr.cy == 35.5f);
    // the constructor's budgets where the file names none
    std::istringstream none("cols 96\n");
    const Case dflt = parse_params(none, Keys::Reference);
    ASSERT_TRUE(dflt.solver_numIter == 24 && dflt.solver_nonLinearIter == 16 && dflt.solver_linearIter == 256 && !dflt.p.fuse_canonical);
}

TEST(DynFusionFramesTest, AnUnknownKeyIsAnErrorAndTheNorthStarFileKeepsItsKeys) {
    const char* texts[] = {"cols 96\nno_such_key 1\n", "solver_numIter x\n"};
    for (const char* t : texts) {
        bool threw = false;
        try {
            std::istringstream bad(t);
            parse_params(bad, Keys::Reference);
        } catch (const dfa::Error&) {
            threw = true;
        }
        ASSERT_TRUE(threw);
    }
    // the four keys belong to the reference-mode file alone
    const char* keys[] = {"fuse_canonical 1\n", "solver_numIter 1\n", "solver_nonLinearIter 1\n", "solver_linearIter 1\n"};
    for (const char* t : keys) {
        bool threw = false;
        try {
            std::istringstream bad(t);
            parse_params(bad, Keys::NorthStar);
        } catch (const dfa::Error&) {
            threw = true;
        }
        ASSERT_TRUE(threw);
        std::istringstream good(t);
        parse_params(good, Keys::Reference);
    }
    Case c;
    ASSERT_TRUE(format_params(c, Keys::Reference).find(format_params(c, Keys::NorthStar)) == 0);
}

// ---- dump mode
namespace {
// reads the protected members of KinFu, as DynFusion does
struct Probe : DynFusion {
    using DynFusion::DynFusion;
    void write_frame(const std::string& dir, int i, bool result) {
        const std::string f = dir + "/f" + std::to_string(i) + "_";
        write_image(f + "dists.bin", dists_);
        write_image(f + "depth0.bin", curr_.depth_pyr[0]);
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
        // the clouds
        write_frame_cloud(f + "live", getLiveFrame());
        write_frame_cloud(f + "warped", getCanonicalWarpedToLive());
        write_frame_cloud(f + "corresponding", getCorrespondingFrame());
        write_frame_cloud(f + "canonical", getCanonicalFrame());
        // the canonical volume and its field
        int field_nodes = -1, field_k = -1;
        std::vector<uint32_t> canon;
        if (const std::shared_ptr<const cuda::TsdfVolume> cv = canonicalVolume()) {
            canon.resize(voxels.size());
            cv->data().download(canon.data(), canon.size() * sizeof(uint32_t));
            field_nodes = cv->knnFieldNodes(), field_k = cv->knnFieldK();
        }
        write_raw(f + "canonical_volume.bin", canon.data(), canon.size());
        char buf[256];
        std::snprintf(buf, sizeof buf, "result %d\ncounter %d\nnodes %zu\nknn %d\ninitial_cost %.17g\nfinal_cost %.17g\nknn_field_nodes %d\nknn_field_k %d\nwarp_graph_searches %d\n",
                      result ? 1 : 0, frame_counter_, w.size(), getWarpfield()->getKnn(), solveInitialCost(), solveFinalCost(), field_nodes, field_k,
                      getWarpfield()->warpGraphSearches());
        std::ofstream status(f + "status.txt");
        status << buf;
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
    const Case c         = parse_params(in, Keys::Reference);
    const KinFuParams& k = c.p.kinfuParams;
    const size_t pixels  = (size_t)k.cols * k.rows;
    if (c.p.north_star) throw dfa::Error(1, "dump: north_star is on (the north-star sequence: test_host_northstar_frames)");
    Probe dynfu(c.p);
    dynfu.nodeStep                   = c.nodeStep;
    dynfu.solverParams.numIter       = c.solver_numIter;
    dynfu.solverParams.nonLinearIter = c.solver_nonLinearIter;
    dynfu.solverParams.linearIter    = c.solver_linearIter;
    dynfu.write_derived(dir);
    for (int i = 0; i < c.frames; ++i) {
        cuda::Depth depth;
        depth.upload(read_frame<unsigned short>(dir + "/depth_" + std::to_string(i) + ".bin", pixels), k.cols);
        const bool result = dynfu(depth);
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
    if (argc >= 3 && !std::strcmp(argv[1], "params")) {
        try {
            std::ifstream in(std::string(argv[2]) + "/params.txt");
            if (!in) throw dfa::Error(1, "no params.txt in " + std::string(argv[2]));
            std::fputs(format_params(parse_params(in, Keys::Reference), Keys::Reference).c_str(), stdout);
            return 0;
        } catch (const std::exception& e) {
            std::fprintf(stderr, "params: %s\n", e.what());
            return 2;
        }
    }
    return mt::run_all(argc, argv);
}
