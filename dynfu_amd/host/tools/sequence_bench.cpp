// sequence_bench — the reference's own timed region on the adaptor classes: time inside DynFusion::operator()
// (src/apps/demo.cpp:90-95: upload outside, operator() inside), frame by frame, over a sequence of raw depth frames.
//
//   sequence_bench FRAMES.u16 W H N DIM ref|northstar [epsilon] [node_step]
//   sequence_bench FRAMES.u16 W H N DIM northstar+fuse|northstar+fuse+rigid|northstar+regrow [epsilon] [node_step]
//
// The second form (tools/regrow_timing.py): the north-star sequence with north_star_fuse_canonical, with
// fuse_unsupported_rigid added, and with north_star_regrow_canonical added to both (canonical_min_weight 2); the JSON then
// also holds the canonical cloud's size per frame.  "+prealign" on any northstar mode adds north_star_rigid_prealign
// (tools/rigid_align_timing.py): the JSON then holds the frames whose alignment was skipped and the last frame's matched counts.
// "+prealign+device" runs that step's loop on the device with the default schedule (rigid_prealign_device), "+prealign+device10"
// with ten iterations at full resolution and no stop, the host loop's work; the JSON then also holds the last frame's iterations.
//
// "+hier" on any northstar mode adds north_star_reg_hierarchy with the default slots (tools/reg_hierarchy_timing.py): the JSON
// then holds, per frame, the PCG iterations, the normal equations solved, the final energy and the valid rows, and the last
// frame's level sizes.
//
// FRAMES.u16: N frames of W x H little-endian uint16 millimetres, back to back (bench.py writes its synthetic
// sequence there).  Prints one JSON object: per-frame milliseconds (the device is synchronised inside the timed region,
// so nothing of a frame hides behind the next one), node / vertex counts, the north-star energies.  No files are
// written: the demo's PCD / VTK output sits outside its timed call (demo.cpp:115-118).
#include <dynfu/dyn_fusion.hpp>

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s FRAMES.u16 W H N DIM ref|northstar [epsilon] [node_step]\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), N = std::atoi(argv[4]), dim = std::atoi(argv[5]);
    const bool ns = !std::strncmp(argv[6], "northstar", 9);
    const bool fuse = ns && std::strstr(argv[6], "+fuse"), regrow = ns && std::strstr(argv[6], "+regrow");
    const bool rigid = regrow || (ns && std::strstr(argv[6], "+rigid"));
    const bool prealign = ns && std::strstr(argv[6], "+prealign");
    const bool device = prealign && std::strstr(argv[6], "+device"), device10 = prealign && std::strstr(argv[6], "+device10");
    const bool hier = ns && std::strstr(argv[6], "+hier");
    std::vector<uint16_t> all((size_t)W * H * N);
    std::ifstream f(argv[1], std::ios::binary);
    if (!f.read((char*)all.data(), (std::streamsize)(all.size() * 2))) {
        std::fprintf(stderr, "cannot read %zu bytes from %s\n", all.size() * 2, argv[1]);
        return 2;
    }
    try {
        DynFuParams p = DynFuParams::defaultParams();  // dyn_fusion.cpp:6-31
        auto& k       = p.kinfuParams;
        k.cols = W, k.rows = H;
        k.intr        = kfusion::Intr(k.intr.fx * W / 640.f, k.intr.fy * H / 480.f, W / 2 - 0.5f, H / 2 - 0.5f);
        p.intr        = k.intr;
        k.volume_dims = dfa::Vec3i(dim, dim, dim);
        p.north_star  = ns;
        p.north_star_fuse_canonical = fuse || regrow, p.fuse_unsupported_rigid = rigid, p.north_star_regrow_canonical = regrow;
        p.north_star_rigid_prealign = prealign;
        p.rigid_prealign_device     = device;
        if (device10) p.rigid_prealign_steps = {1}, p.rigid_prealign_level_iters = {10}, p.rigid_prealign_stop_rot = p.rigid_prealign_stop_trans = 0.f;
        p.north_star_reg_hierarchy = hier;
        if (argc > 7) p.epsilon = (float)std::atof(argv[7]);
        else if (ns) p.epsilon = 0.05f;
        DynFusion dynfu(p);
        dynfu.nodeStep = argc > 8 ? std::atoi(argv[8]) : 128;  // dyn_fusion.cpp:151
        kfusion::cuda::Depth depth;
        std::vector<double> ms;
        std::vector<size_t> nodes, cloud;
        std::vector<int> pcg_iters, gn_solves;
        std::vector<double> final_cost;
        std::vector<long long> valid;
        for (int i = 0; i < N; ++i) {
            depth.upload(all.data() + (size_t)i * W * H, (size_t)W * sizeof(uint16_t), H, W);  // demo.cpp:90
            (void)hipDeviceSynchronize();
            const auto t0 = std::chrono::steady_clock::now();
            dynfu(depth);  // demo.cpp:92-95
            (void)hipDeviceSynchronize();
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            nodes.push_back(dynfu.getWarpfield()->getNodes().size());
            cloud.push_back(dynfu.canonicalVertexCount());
            if (ns) {
                pcg_iters.push_back(dynfu.northStarPcgIterations()), gn_solves.push_back(dynfu.northStarGnSolves());
                final_cost.push_back(dynfu.northStarFinalCost()), valid.push_back(dynfu.northStarValidRows());
            }
        }
        std::printf("{\"mode\": \"%s\", \"dim\": %d, \"width\": %d, \"height\": %d, \"frames\": %d, \"canonical_vertices\": %zu, "
                    "\"live_vertices_last\": %zu, \"nodes_first\": %zu, \"nodes_last\": %zu, \"epsilon\": %g, \"node_step\": %d",
                    ns ? argv[6] : "ref", dim, W, H, N, dynfu.getCanonicalWarpedToLive()->size(),
                    dynfu.getLiveFrame() ? dynfu.getLiveFrame()->size() : (size_t)0, nodes.front(), nodes.back(), p.epsilon,
                    dynfu.nodeStep);
        if (ns)
            std::printf(", \"cost_first\": %.6g, \"cost_last\": %.6g, \"valid_rows\": %lld", dynfu.northStarInitialCost(),
                        dynfu.northStarFinalCost(), dynfu.northStarValidRows());
        if (prealign)
            std::printf(", \"rigid_skipped\": %d, \"rigid_matched_first\": %lld, \"rigid_matched_last\": %lld", dynfu.rigidSkippedFrames(),
                        dynfu.northStarRigidMatched().first, dynfu.northStarRigidMatched().last);
        if (device) {
            std::printf(", \"rigid_iterations\": [");
            const std::vector<int> ran = dynfu.northStarRigidIterations();
            for (size_t i = 0; i < ran.size(); ++i) std::printf("%s%d", i ? ", " : "", ran[i]);
            std::printf("]");
        }
        if (fuse || regrow) {
            std::printf(", \"regrow_skipped\": %d, \"canonical_vertices_by_frame\": [", dynfu.regrowSkippedFrames());
            for (size_t i = 0; i < cloud.size(); ++i) std::printf("%s%zu", i ? ", " : "", cloud[i]);
            std::printf("]");
        }
        if (ns) {
            std::printf(", \"pcg_iters_by_frame\": [");
            for (size_t i = 0; i < pcg_iters.size(); ++i) std::printf("%s%d", i ? ", " : "", pcg_iters[i]);
            std::printf("], \"gn_solves_by_frame\": [");
            for (size_t i = 0; i < gn_solves.size(); ++i) std::printf("%s%d", i ? ", " : "", gn_solves[i]);
            std::printf("], \"final_cost_by_frame\": [");
            for (size_t i = 0; i < final_cost.size(); ++i) std::printf("%s%.6g", i ? ", " : "", final_cost[i]);
            std::printf("], \"valid_rows_by_frame\": [");
            for (size_t i = 0; i < valid.size(); ++i) std::printf("%s%lld", i ? ", " : "", valid[i]);
            std::printf("]");
        }
        if (hier) {
            std::printf(", \"node_levels\": [");
            const std::vector<int> lv = dynfu.northStarNodeLevels();
            for (size_t i = 0; i < lv.size(); ++i) std::printf("%s%d", i ? ", " : "", lv[i]);
            std::printf("]");
        }
        std::printf(", \"frame_ms\": [");
        for (size_t i = 0; i < ms.size(); ++i) std::printf("%s%.4f", i ? ", " : "", ms[i]);
        std::printf("]}\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sequence_bench: %s\n", e.what());
        return 1;
    }
    return 0;
}
