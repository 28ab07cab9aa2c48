// test_host_tsdf_warped6.cpp — kfusion::cuda::TsdfVolume::integrateWarped6 and DynFusion's canonical volume in north-star mode
// (DynFuParams::north_star_fuse_canonical, DynFusion::canonicalVolume): the adaptor's voxels are the C call's bit for bit (and
// dfa_tsdf_integrate_warped6 itself is checked against the numpy statement by tests/test_gpu_tsdf_warped6.py), its occupancy
// map stays usable, the switches' rules, and a north-star sequence with the switch on is the sequence with it off in
// everything but the canonical volume — which accumulates, and after frame 1 is integrateWarped6 applied by hand.
#include <algorithm>
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

// the node frame of the first test: turned by 0.1 rad about y and shifted against the world
Affine3f node_frame() {
    Affine3f a;
    const float c = std::cos(0.1f), s = std::sin(0.1f);
    a.R[0] = c, a.R[2] = s, a.R[6] = -s, a.R[8] = c;
    return a.translate(Vec3f(0.05f, -0.03f, 0.1f));
}

// a volume of the KinFu set-up with the sphere at 1.5 m fused, the dists of the sphere at 1.48 m, and 9 x 9 nodes on a plane
// through the sphere's front, given in the node frame, each with a small rotation and translation
struct Scene {
    cuda::TsdfVolume vol{Vec3i::all(DIM)};
    Intr intr{F, F, W / 2 - 0.5f, H / 2 - 0.5f};
    cuda::Dists next;
    dfa::DeviceArray<float> pos, dq, w;
    Affine3f frame = node_frame();
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
        const Affine3f vol2node = frame.inv() * vol.getPose();
        std::vector<float> hp, hq, hw;
        for (int i = 0; i < 9; ++i)
            for (int j = 0; j < 9; ++j) {
                const float v[3] = {1.1f + 0.1f * i, 1.1f + 0.1f * j, 0.55f + 0.01f * ((i * 7 + j * 3) % 5)};  // volume frame
                for (int c = 0; c < 3; ++c)
                    hp.push_back(vol2node.R[3 * c] * v[0] + vol2node.R[3 * c + 1] * v[1] + vol2node.R[3 * c + 2] * v[2] + vol2node.t[c]);
                hw.push_back(0.12f + 0.01f * ((i + j) % 4));
                // a rotation by up to 0.04 rad about x, then a translation by up to 2 cm: real (cos, sin, 0, 0), dual (0, t) real / 2
                const float a = 0.01f * (j - 4), cr = std::cos(0.5f * a), sr = std::sin(0.5f * a);
                const float t[3] = {0.004f * (i - 4), 0.003f * (j - 4), -0.02f};
                hq.insert(hq.end(), {cr, sr, 0.f, 0.f, 0.5f * (-t[0] * sr), 0.5f * (t[0] * cr), 0.5f * (t[1] * cr + t[2] * sr),
                                     0.5f * (t[2] * cr - t[1] * sr)});
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

// DynFusionTest.NorthStarModeFollowsTheDepthFrame's set-up at half its resolution: 64^3 voxels, 160 x 120 pixels
DynFuParams small_params(bool north_star, bool fuse_canonical, bool north_star_fuse_canonical) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(DIM);
    p.epsilon = 0.05f;
    p.north_star = north_star, p.fuse_canonical = fuse_canonical, p.north_star_fuse_canonical = north_star_fuse_canonical;
    return p;
}
}  // namespace

TEST(TsdfWarped6Test, IntegrateWarped6MatchesTheCCall) {
    for (const auto mode : {cuda::TsdfVolume::UnsupportedMode::Skip, cuda::TsdfVolume::UnsupportedMode::Rigid}) {
        Scene s;
        const std::vector<uint32_t> before = voxels(s.cvol());
        // the C call on a copy of the voxels, with the two transforms formed by hand
        dfa::DeviceArray<uint32_t> direct(before.size());
        direct.upload(before);
        const Affine3f camera;
        float vol2node[12], node2cam[12];
        (s.frame.inv() * s.vol.getPose()).to12(vol2node);
        (camera.inv() * s.frame).to12(node2cam);
        const Vec3f vs = s.vol.getVoxelSize();
        const int cmode = mode == cuda::TsdfVolume::UnsupportedMode::Rigid ? DFA_WARPED_RIGID : DFA_WARPED_SKIP;
        dfa::check(dfa_tsdf_integrate_warped6(s.next.ptr(), (int)s.next.step(), W, H, direct.ptr(), DIM, DIM, DIM, nullptr, vs.v,
                                              s.vol.getTruncDist(), s.vol.getMaxWeight(), vol2node, node2cam, F, F, W / 2 - 0.5f,
                                              H / 2 - 0.5f, s.pos.ptr(), s.dq.ptr(), s.w.ptr(), s.D, 8, cmode, nullptr),
                   "dfa_tsdf_integrate_warped6");
        ASSERT_TRUE(s.cvol().occupancy() != nullptr);
        s.vol.integrateWarped6(s.next, camera, s.intr, s.frame, s.pos.ptr(), s.dq.ptr(), s.w.ptr(), s.D, 8, mode);
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

TEST(TsdfWarped6Test, ConstructorRules) {
    ASSERT_TRUE(construction_throws(small_params(false, false, true)));  // north_star_fuse_canonical without north_star
    ASSERT_TRUE(construction_throws(small_params(true, true, false)));   // fuse_canonical with north_star: still refused
    ASSERT_TRUE(construction_throws(small_params(true, true, true)));
    ASSERT_TRUE(!construction_throws(small_params(true, false, true)));
    ASSERT_TRUE(!construction_throws(small_params(true, false, false)));
    ASSERT_TRUE(!construction_throws(small_params(false, true, false)));
}

TEST(TsdfWarped6Test, NorthStarSequenceWithAndWithoutTheCanonicalVolume) {
    cuda::Depth d[4];
    for (int f = 0; f < 4; ++f) d[f].upload(sphere_depth(1.5f - 0.01f * f), W);  // the sphere comes 1 cm closer per frame
    DynFusion off(small_params(true, false, false)), on(small_params(true, false, true));
    off.nodeStep = on.nodeStep = 16;  // (64 at 128^3: a quarter of the vertices here)
    std::vector<uint32_t> prev;
    cuda::TsdfVolume hand{Vec3i::all(DIM)};
    size_t nodes_before = 0;
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
        std::printf("frame %d: %zu nodes, largest weight %u, %zu voxels gained weight\n", f, b.w.size(), top, grown);
        ASSERT_EQ(lower, (size_t)0);  // weights never fall: not below the frame before, hence not below frame 0
        ASSERT_TRUE(f == 0 || grown > 200);
        ASSERT_EQ(top, (unsigned)(f + 1));
        if (f == 0) {
            hand.setSize(on.tsdf().getSize()), hand.setPose(on.tsdf().getPose());
            hand.setTruncDist(on.tsdf().getTruncDist()), hand.setMaxWeight(on.tsdf().getMaxWeight());
            hand.copyVoxelsFrom(*on.canonicalVolume());
            nodes_before = b.w.size();
        }
        if (f == 1) {
            // frame 1 by hand: integrateWarped6 on a copy of frame 0's volume, through the nodes the solve had — the first D of
            // the warp field's arrays: Warpfield::update has grown it since —, the node frame the camera of frame 0
            ASSERT_TRUE(nodes_before > 20 && b.w.size() >= nodes_before);
            std::vector<float> pos(b.pos.begin(), b.pos.begin() + 3 * nodes_before), w(b.w.begin(), b.w.begin() + nodes_before),
                dq(b.dq.begin(), b.dq.begin() + 8 * nodes_before);
            dfa::DeviceArray<float> dpos, dw, ddq;
            dpos.upload(pos), dw.upload(w), ddq.upload(dq);
            const KinFuParams& kp = on.KinFu::params();
            cuda::Dists dists;
            cuda::computeDists(d[1], dists, kp.intr);
            hand.integrateWarped6(dists, Affine3f(), kp.intr, Affine3f(), dpos.ptr(), ddq.ptr(), dw.ptr(), (int)nodes_before,
                                  std::min(on.getWarpfield()->getKnn(), 8));
            ASSERT_TRUE(same(voxels(hand), canon));
        }
        prev = canon;
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
