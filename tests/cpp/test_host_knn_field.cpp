// test_host_knn_field.cpp — the k-NN field through the host adaptors: TsdfVolume::buildKnnField / appendKnnField and
// DynFuParams::fuse_knn_field.  The cached canonical fusion is the searching one bit for bit — a short DynFusion sequence run
// with the switch off and on, in reference mode (fuse_canonical) and in north-star mode (north_star_fuse_canonical), the
// canonical volumes compared after every frame — over a sequence in which Warpfield::update inserts nodes, so that the
// field is appended to; the switch alone is refused; beyond its cap the field is dropped and the sequence goes on searching.
// (dfa_knn_field_* themselves: tests/test_gpu_knn_field.py.)  The sizes are those of test_host_tsdf_warped.cpp /
// test_host_tsdf_warped6.cpp.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <dynfu/dyn_fusion.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>

#include "../../include/dynfu_amd.h"
#include "dynfu_fixtures.hpp"
#include "minitest.hpp"

using namespace kfusion;
using namespace dynfu_fixtures;
using namespace dynfu_fixtures::sphere_scene;

namespace {
const int DIM = 64;

DynFuParams small_params(bool north_star, bool fuse, bool field, size_t max_bytes = 0) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(DIM);
    p.epsilon = 0.05f;
    p.north_star = north_star;
    (north_star ? p.north_star_fuse_canonical : p.fuse_canonical) = fuse;
    p.fuse_knn_field = field, p.fuse_knn_field_max_bytes = max_bytes;
    return p;
}

// the sequence of test_host_tsdf_warped.cpp / test_host_tsdf_warped6.cpp (the sphere comes 1 cm closer per frame) run with the
// searching fusion and with the field: the canonical volumes after every frame, and everything else the frames produce
void run_sequence(bool north_star, size_t max_bytes, bool expect_field) {
    cuda::Depth d[4];
    for (int f = 0; f < 4; ++f) d[f].upload(sphere_depth(1.5f - 0.01f * f), W);
    DynFusion off(small_params(north_star, true, false)), on(small_params(north_star, true, true, max_bytes));
    // (nodeStep stays at its default in both modes: frame 0's nodes then leave part of the surface unsupported, and
    // Warpfield::update inserts nodes there — with a node at every 16th vertex, as test_host_tsdf_warped6.cpp has them, it never does)
    if (!north_star)
        for (DynFusion* df : {&off, &on}) df->solverParams.numIter = 2, df->solverParams.nonLinearIter = 2, df->solverParams.linearIter = 64;
    size_t nodes_prev = 0, appended_frames = 0, inserting_frames = 0;
    int field_prev = 0;
    for (int f = 0; f < 4; ++f) {
        const bool fa = off(d[f]), fb = on(d[f]);
        ASSERT_TRUE(fa == (f > 0) && fb == fa);
        std::vector<float> pa, wa, qa, pb, wb, qb;
        off.getWarpfield()->hostArrays(pa, wa, qa), on.getWarpfield()->hostArrays(pb, wb, qb);
        ASSERT_TRUE(!pa.empty() && same(pa, pb) && same(wa, wb) && same(qa, qb));
        ASSERT_TRUE(same(off.getCanonicalWarpedToLive()->vertices().points, on.getCanonicalWarpedToLive()->vertices().points));
        ASSERT_TRUE(off.canonicalVolume() != nullptr && on.canonicalVolume() != nullptr);
        const std::vector<uint32_t> want = voxels(*off.canonicalVolume()), got = voxels(*on.canonicalVolume());
        size_t differ = 0;
        for (size_t i = 0; i < got.size(); ++i) differ += got[i] != want[i];
        const cuda::TsdfVolume& vol = *on.canonicalVolume();
        std::printf("%s frame %d: %zu nodes, field over %d, %zu voxels differ\n", north_star ? "north-star" : "reference", f, wa.size(),
                    vol.knnFieldNodes(), differ);
        ASSERT_EQ(differ, (size_t)0);
        ASSERT_TRUE(off.canonicalVolume()->knnField() == nullptr);
        ASSERT_TRUE((vol.knnField() != nullptr) == expect_field);
        // the field holds the nodes the last integrate saw: the warp field may have grown since (Warpfield::update runs last)
        if (expect_field) ASSERT_EQ((size_t)vol.knnFieldNodes(), f == 0 ? wa.size() : nodes_prev);
        if (f > 0 && wa.size() > nodes_prev) ++inserting_frames;
        if (f > 0 && vol.knnFieldNodes() > field_prev) ++appended_frames;
        nodes_prev = wa.size(), field_prev = vol.knnFieldNodes();
    }
    // Warpfield::update inserted nodes in some frame before the last, and the integrate of the frame after it appended them
    std::printf("frames whose update inserted nodes: %zu, frames that appended to the field: %zu\n", inserting_frames, appended_frames);
    ASSERT_TRUE(inserting_frames >= 1);
    if (expect_field) ASSERT_TRUE(appended_frames >= 1);
}
}  // namespace

TEST(HostKnnFieldTest, TheSwitchNeedsAFusionSwitch) {
    ASSERT_TRUE(construction_throws(small_params(false, false, true)));
    ASSERT_TRUE(construction_throws(small_params(true, false, true)));
    ASSERT_TRUE(!construction_throws(small_params(false, true, true)));
    ASSERT_TRUE(!construction_throws(small_params(true, true, true)));
}

TEST(HostKnnFieldTest, ReferenceModeSequenceIsTheSearchingOne) {
    // two runs are compared bit for bit: the reference-mode solve assembles with float atomics unless asked for its
    // order-stable form (read once per solver plan)
    ::setenv("DFA_ASSEMBLE_DETERMINISTIC", "1", 1);
    run_sequence(false, 0, true);
}

TEST(HostKnnFieldTest, NorthStarSequenceIsTheSearchingOne) { run_sequence(true, 0, true); }

TEST(HostKnnFieldTest, BeyondItsCapTheFieldIsDroppedAndTheSequenceSearches) {
    ::setenv("DFA_ASSEMBLE_DETERMINISTIC", "1", 1);
    run_sequence(false, 4096, false);  // less than one record of k = 8
}

TEST(HostKnnFieldTest, VolumeUsesTheFieldOnlyWhereItMatches) {
    // 9 x 9 nodes on a plane through the sphere's front, as test_host_tsdf_warped.cpp
    cuda::TsdfVolume vol{Vec3i::all(DIM)}, plain{Vec3i::all(DIM)};
    Intr intr{F, F, W / 2 - 0.5f, H / 2 - 0.5f};
    for (cuda::TsdfVolume* v : {&vol, &plain}) {
        v->setTruncDist(0.1f), v->setMaxWeight(64), v->setSize(Vec3f::all(3.f));
        v->setPose(Affine3f().translate(Vec3f(-1.5f, -1.5f, 0.5f)));
    }
    cuda::Depth depth;
    cuda::Dists dists, next;
    depth.upload(sphere_depth(1.5f), W);
    cuda::computeDists(depth, dists, intr);
    vol.clearAndIntegrate(dists, Affine3f(), intr), plain.clearAndIntegrate(dists, Affine3f(), intr);
    depth.upload(sphere_depth(1.48f), W);
    cuda::computeDists(depth, next, intr);
    std::vector<float> hp, hq, hw;
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
            hp.insert(hp.end(), {1.1f + 0.1f * i, 1.1f + 0.1f * j, 0.55f + 0.01f * ((i * 7 + j * 3) % 5)});
            hw.push_back(0.12f + 0.01f * ((i + j) % 4));
            const float t[3] = {0.004f * (i - 4), 0.003f * (j - 4), -0.02f};
            hq.insert(hq.end(), {1.f, 0.f, 0.f, 0.f, 0.f, 0.5f * t[0], 0.5f * t[1], 0.5f * t[2]});
        }
    dfa::DeviceArray<float> pos, dq, w;
    pos.upload(hp), dq.upload(hq), w.upload(hw);
    const int D = 81;
    ASSERT_TRUE(vol.knnField() == nullptr && vol.knnFieldNodes() == 0);
    ASSERT_TRUE(vol.buildKnnField(pos.ptr(), w.ptr(), 60, 8));
    ASSERT_TRUE(vol.knnField() != nullptr && vol.knnFieldNodes() == 60);
    // 81 nodes against a field over 60: the call searches, and is right
    vol.integrateWarped(next, Affine3f(), intr, pos.ptr(), dq.ptr(), w.ptr(), D, 8);
    plain.integrateWarped(next, Affine3f(), intr, pos.ptr(), dq.ptr(), w.ptr(), D, 8);
    ASSERT_TRUE(same(voxels(vol), voxels(plain)));
    ASSERT_TRUE(vol.appendKnnField(pos.ptr(), w.ptr(), D) && vol.knnFieldNodes() == D);
    for (const auto mode : {cuda::TsdfVolume::UnsupportedMode::Skip, cuda::TsdfVolume::UnsupportedMode::Rigid}) {
        vol.integrateWarped(next, Affine3f(), intr, pos.ptr(), dq.ptr(), w.ptr(), D, 8, mode);
        plain.integrateWarped(next, Affine3f(), intr, pos.ptr(), dq.ptr(), w.ptr(), D, 8, mode);
        ASSERT_TRUE(same(voxels(vol), voxels(plain)));
    }
    // another k, and the 6-DoF call against a field without a frame: searched, and right
    vol.integrateWarped(next, Affine3f(), intr, pos.ptr(), dq.ptr(), w.ptr(), D, 4);
    plain.integrateWarped(next, Affine3f(), intr, pos.ptr(), dq.ptr(), w.ptr(), D, 4);
    const Affine3f frame = Affine3f().translate(Vec3f(0.1f, -0.2f, 0.05f));
    vol.integrateWarped6(next, Affine3f(), intr, frame, pos.ptr(), dq.ptr(), w.ptr(), D, 8);
    plain.integrateWarped6(next, Affine3f(), intr, frame, pos.ptr(), dq.ptr(), w.ptr(), D, 8);
    ASSERT_TRUE(same(voxels(vol), voxels(plain)));
    // a field with that frame serves the 6-DoF call
    ASSERT_TRUE(vol.buildKnnField(pos.ptr(), w.ptr(), D, 8, &frame));
    vol.integrateWarped6(next, Affine3f(), intr, frame, pos.ptr(), dq.ptr(), w.ptr(), D, 8, cuda::TsdfVolume::UnsupportedMode::Rigid);
    plain.integrateWarped6(next, Affine3f(), intr, frame, pos.ptr(), dq.ptr(), w.ptr(), D, 8, cuda::TsdfVolume::UnsupportedMode::Rigid);
    ASSERT_TRUE(same(voxels(vol), voxels(plain)));
    ASSERT_TRUE(static_cast<const cuda::TsdfVolume&>(vol).occupancy() != nullptr);  // the map is kept as the searching calls keep it
    // a cap below one record: the build reports it, and the volume has no field
    ASSERT_TRUE(!vol.buildKnnField(pos.ptr(), w.ptr(), D, 8, nullptr, 100) && vol.knnField() == nullptr);
    bool thrown = false;
    try {
        vol.appendKnnField(pos.ptr(), w.ptr(), D);
    } catch (const dfa::Error&) {
        thrown = true;
    }
    ASSERT_TRUE(thrown);
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
