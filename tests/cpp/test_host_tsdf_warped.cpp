// test_host_tsdf_warped.cpp — kfusion::cuda::TsdfVolume::integrateWarped and DynFusion's canonical volume
// (DynFuParams::fuse_canonical, DynFusion::canonicalVolume): the adaptor's voxels are the C call's bit for bit (and
// dfa_tsdf_integrate_warped itself is checked against the numpy statement by tests/test_gpu_tsdf_warped.py), its occupancy
// map stays usable, a sequence with the switch on is the sequence with it off in everything but the canonical volume, and that
// volume accumulates.
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

// a volume of the KinFu set-up with the sphere at 1.5 m fused, the dists of the sphere at 1.48 m, and 9 x 9 nodes on a
// plane through the sphere's front (volume frame), each with a small rigid transform
struct Scene {
    cuda::TsdfVolume vol{Vec3i::all(DIM)};
    Intr intr{F, F, W / 2 - 0.5f, H / 2 - 0.5f};
    cuda::Dists next;
    dfa::DeviceArray<float> pos, dq, w;
    int D = 81;
    Scene() {
        vol.setTruncDist(0.1f), vol.setMaxWeight(64), vol.setSize(Vec3f::all(3.f));
        vol.setPose(Affine3f().translate(Vec3f(-1.5f, -1.5f, 0.5f)));
        cuda::Depth depth;
        cuda::Dists dists;
        depth.upload(sphere_depth(1.5f), W);
        cuda::computeDists(depth, dists, intr);
        vol.clearAndIntegrate(dists, Affine3f(), intr);
        depth.upload(sphere_depth(1.48f), W);
        cuda::computeDists(depth, next, intr);
        std::vector<float> hp, hq, hw;
        for (int i = 0; i < 9; ++i)
            for (int j = 0; j < 9; ++j) {
                hp.insert(hp.end(), {1.1f + 0.1f * i, 1.1f + 0.1f * j, 0.55f + 0.01f * ((i * 7 + j * 3) % 5)});
                hw.push_back(0.12f + 0.01f * ((i + j) % 4));
                // a translation (dual = (0, t) / 2) by up to 2 cm
                const float t[3] = {0.004f * (i - 4), 0.003f * (j - 4), -0.02f};
                hq.insert(hq.end(), {1.f, 0.f, 0.f, 0.f, 0.f, 0.5f * t[0], 0.5f * t[1], 0.5f * t[2]});
            }
        pos.upload(hp), dq.upload(hq), w.upload(hw);
    }
    const cuda::TsdfVolume& cvol() const { return vol; }
};

// everything of a frame the canonical fusion must not change
struct FrameOutputs {
    bool flag;
    std::vector<dfa::PointXYZ> warped, live;
    std::vector<float> pos, w, dq;
    std::vector<uint32_t> live_volume;
};
FrameOutputs outputs(DynFusion& df, bool flag) {
    FrameOutputs o;
    o.flag   = flag;
    o.warped = df.getCanonicalWarpedToLive()->vertices().points;
    if (df.getLiveFrame()) o.live = df.getLiveFrame()->vertices().points;
    df.getWarpfield()->hostArrays(o.pos, o.w, o.dq);
    o.live_volume = voxels(static_cast<const cuda::TsdfVolume&>(df.tsdf()));
    return o;
}

DynFuParams small_params(bool fuse_canonical) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(DIM);
    p.epsilon = 0.05f;
    p.fuse_canonical = fuse_canonical;
    return p;
}
}  // namespace

TEST(TsdfWarpedTest, IntegrateWarpedMatchesTheCCall) {
    for (const auto mode : {cuda::TsdfVolume::UnsupportedMode::Skip, cuda::TsdfVolume::UnsupportedMode::Rigid}) {
        Scene s;
        const std::vector<uint32_t> before = voxels(s.cvol());
        // the C call on a copy of the voxels, with vol2cam formed as integrate() forms it
        dfa::DeviceArray<uint32_t> direct(before.size());
        direct.upload(before);
        float aff[12];
        (Affine3f().inv() * s.vol.getPose()).to12(aff);
        const Vec3f vs = s.vol.getVoxelSize();
        dfa::check(dfa_tsdf_integrate_warped(s.next.ptr(), (int)s.next.step(), W, H, direct.ptr(), DIM, DIM, DIM, nullptr, vs.v,
                                             s.vol.getTruncDist(), s.vol.getMaxWeight(), aff, F, F, W / 2 - 0.5f, H / 2 - 0.5f,
                                             s.pos.ptr(), s.dq.ptr(), s.w.ptr(), s.D, 8,
                                             mode == cuda::TsdfVolume::UnsupportedMode::Rigid ? DFA_WARPED_RIGID : DFA_WARPED_SKIP, nullptr),
                   "dfa_tsdf_integrate_warped");
        ASSERT_TRUE(s.cvol().occupancy() != nullptr);
        s.vol.integrateWarped(s.next, Affine3f(), s.intr, s.pos.ptr(), s.dq.ptr(), s.w.ptr(), s.D, 8, mode);
        ASSERT_TRUE(s.cvol().occupancy() != nullptr);  // the map is kept, under integrate()'s sole-owner rule
        std::vector<uint32_t> want;
        direct.download(want);
        const std::vector<uint32_t> got = voxels(s.cvol());
        size_t changed = 0;
        for (size_t i = 0; i < got.size(); ++i) changed += got[i] != before[i];
        std::printf("mode %d: %zu voxels changed\n", (int)mode, changed);
        ASSERT_TRUE(changed > 200);  // (the sphere's front is ~700 voxels per layer of this 64^3 volume: not a handful)
        ASSERT_TRUE(same(got, want));
        // the map covers what the call wrote: the cloud read through it is the cloud read from every voxel
        dfa::DeviceArray<Point> b1, b2;
        std::vector<Point> with_map, without;
        s.cvol().fetchCloud(b1).download(with_map);
        cuda::TsdfVolume copy(s.vol);  // (a copy of the object: neither side trusts its map any more)
        ASSERT_TRUE(copy.occupancy() == nullptr);
        copy.fetchCloud(b2).download(without);
        ASSERT_TRUE(with_map.size() > 100 && same(with_map, without));
    }
}

TEST(TsdfWarpedTest, CopyVoxelsFromCopiesVoxelsAndMap) {
    Scene s;
    cuda::TsdfVolume other(Vec3i::all(DIM));
    other.copyVoxelsFrom(s.cvol());
    ASSERT_TRUE(same(voxels(other), voxels(s.cvol())));
    ASSERT_TRUE(static_cast<const cuda::TsdfVolume&>(other).occupancy() != nullptr && s.cvol().occupancy() != nullptr);
    ASSERT_TRUE(other.data().ptr<uint32_t>() != s.cvol().data().ptr<uint32_t>());
    bool thrown = false;
    try {
        cuda::TsdfVolume small(Vec3i::all(32));
        small.copyVoxelsFrom(s.cvol());
    } catch (const dfa::Error&) {
        thrown = true;
    }
    ASSERT_TRUE(thrown);
}

TEST(TsdfWarpedTest, FuseCanonicalNeedsReferenceMode) {
    DynFuParams p = small_params(true);
    p.north_star  = true;
    bool thrown   = false;
    try {
        DynFusion df(p);
    } catch (const dfa::Error&) {
        thrown = true;
    }
    ASSERT_TRUE(thrown);
}

TEST(TsdfWarpedTest, SequenceWithAndWithoutTheCanonicalVolume) {
    cuda::Depth d[4];
    for (int f = 0; f < 4; ++f) d[f].upload(sphere_depth(1.5f - 0.01f * f), W);
    // two runs are compared bit for bit: the reference-mode solve assembles with float atomics unless asked for its
    // order-stable form (read once per solver plan)
    ::setenv("DFA_ASSEMBLE_DETERMINISTIC", "1", 1);
    DynFusion off(small_params(false)), on(small_params(true));
    for (DynFusion* df : {&off, &on}) df->solverParams.numIter = 2, df->solverParams.nonLinearIter = 2, df->solverParams.linearIter = 64;
    std::vector<uint32_t> prev;
    for (int f = 0; f < 4; ++f) {
        const FrameOutputs a = outputs(off, off(d[f]));
        const FrameOutputs b = outputs(on, on(d[f]));
        ASSERT_TRUE(a.flag == (f > 0) && b.flag == a.flag);
        ASSERT_TRUE(!a.warped.empty() && !a.pos.empty());
        ASSERT_TRUE(same(a.warped, b.warped) && same(a.live, b.live) && same(a.pos, b.pos) && same(a.w, b.w) && same(a.dq, b.dq));
        ASSERT_TRUE(same(a.live_volume, b.live_volume));
        ASSERT_TRUE(off.canonicalVolume() == nullptr && on.canonicalVolume() != nullptr);
        const std::vector<uint32_t> canon = voxels(*on.canonicalVolume());
        if (f == 0) ASSERT_TRUE(same(canon, b.live_volume));  // the canonical volume starts as what frame 0 saw
        unsigned top = 0;
        size_t lower = 0, grown = 0;
        for (size_t i = 0; i < canon.size(); ++i) {
            top = std::max(top, canon[i] >> 16);
            if (f > 0) lower += (canon[i] >> 16) < (prev[i] >> 16), grown += (canon[i] >> 16) > (prev[i] >> 16);
        }
        std::printf("frame %d: largest weight %u, %zu voxels gained weight\n", f, top, grown);
        ASSERT_EQ(lower, (size_t)0);  // weights never fall: not below the frame before, hence not below frame 0
        ASSERT_TRUE(f == 0 || grown > 200);
        ASSERT_EQ(top, (unsigned)(f + 1));
        prev = canon;
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
