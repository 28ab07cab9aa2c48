// test_host_rigid_loop.cpp — the rigid pre-alignment of north-star mode with its Gauss-Newton loop on the device
// (DynFuParams::rigid_prealign_device, rigid_prealign_steps, rigid_prealign_level_iters, rigid_prealign_stop_rot / _trans;
// NorthStarSolver::alignRigid(..., RigidSchedule, T), rigidIterationsRun; DynFusion::northStarRigidIterations) on the
// four-frame planted-motion sequence of test_host_rigid_align.cpp, 320 x 240 / 256^3.  With the schedule {1} x 10 and no
// stop the device loop is the host loop: each frame's pose agrees to 0.1 mm and 1e-4 rad (far inside that test's 5 mm bar,
// far above float32 noise).  With the default schedule the estimate is the inverse of the planted motion at that test's
// bars, the solve starts from a lower energy than without the step and at least one frame stops early.  An empty depth frame
// is a skipped frame, the switch's rule throws, and with the switch off the new fields change no bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <dynfu/dyn_fusion.hpp>

#include "../../include/dynfu_amd.h"
#include "dynfu_fixtures.hpp"
#include "minitest.hpp"

using namespace kfusion;
using namespace dynfu_fixtures;
using namespace dynfu_fixtures::planted_motion_scene;

namespace {
// -------------------------------------------------------------------------------------------------------- the sequence
// (the planted-motion scene of dynfu_fixtures.hpp: 320 x 240, 256^3 voxels over 2.2 m)

struct Switches {
    bool prealign = false, device = false;
    std::vector<int> steps, iters;  // empty: DynFuParams' defaults
    float stop = -1.f;              // < 0: DynFuParams' defaults
    // every PCG gets its full launch budget: two runs that are compared must not depend on which plan the cache hands them
    bool full_budget = true;
};
DynFuParams params(const Switches& s) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(DIM);
    p.kinfuParams.volume_size = Vec3f::all(VOLUME);
    p.kinfuParams.volume_pose = Affine3f().translate(Vec3f(-VOLUME / 2, -VOLUME / 2, VOLUME_Z0));
    p.intr = p.kinfuParams.intr;
    p.epsilon = 0.05f;
    p.north_star = true;
    p.north_star_rigid_prealign = s.prealign;
    p.rigid_prealign_device = s.device;
    if (!s.steps.empty()) p.rigid_prealign_steps = s.steps, p.rigid_prealign_level_iters = s.iters;
    if (s.stop >= 0.f) p.rigid_prealign_stop_rot = p.rigid_prealign_stop_trans = s.stop;
    p.northStarParams.adaptiveLaunch = !s.full_budget;
    return p;
}
Switches host_loop() {
    Switches s;
    s.prealign = true;
    return s;
}
Switches device_loop(std::vector<int> steps = {}, std::vector<int> iters = {}, float stop = -1.f) {
    Switches s;
    s.prealign = s.device = true, s.steps = steps, s.iters = iters, s.stop = stop;
    return s;
}
// the angle of Ra Rb^T (radians) and |ta - tb| (metres)
void pose_difference(const Affine3f& a, const Affine3f& b, double& angle, double& dist) {
    double D[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[3 * i + j] = (double)a.R[3 * i] * b.R[3 * j] + (double)a.R[3 * i + 1] * b.R[3 * j + 1] + (double)a.R[3 * i + 2] * b.R[3 * j + 2];
    const double x = 0.5 * (D[7] - D[5]), y = 0.5 * (D[2] - D[6]), z = 0.5 * (D[3] - D[1]);
    angle = std::asin(std::fmin(1.0, std::sqrt(x * x + y * y + z * z)));
    dist  = std::sqrt(std::pow((double)a.t[0] - b.t[0], 2) + std::pow((double)a.t[1] - b.t[1], 2) + std::pow((double)a.t[2] - b.t[2], 2));
}
}  // namespace

TEST(RigidLoopTest, TenIterationsAtFullResolutionAreTheHostLoop) {
    Depths in;
    DynFusion host(params(host_loop())), dev(params(device_loop({1}, {10}, 0.f)));
    host.nodeStep = dev.nodeStep = 64;
    for (int f = 0; f < 4; ++f) {
        ASSERT_TRUE(host(in.d[f]) == (f > 0));
        ASSERT_TRUE(dev(in.d[f]) == (f > 0));
        ASSERT_TRUE(host.northStarRigidIterations().empty());
        if (f == 0) {
            ASSERT_TRUE(is_identity(dev.northStarRigidPose()) && dev.northStarRigidIterations().empty());
            continue;
        }
        double angle, dist;
        pose_difference(dev.northStarRigidPose(), host.northStarRigidPose(), angle, dist);
        std::printf("frame %d: device loop vs host loop: %.3e rad, %.3e m; matched %lld -> %lld (host %lld -> %lld)\n", f, angle, dist,
                    dev.northStarRigidMatched().first, dev.northStarRigidMatched().last, host.northStarRigidMatched().first,
                    host.northStarRigidMatched().last);
        ASSERT_TRUE(!is_identity(dev.northStarRigidPose()));
        ASSERT_TRUE(angle <= 1e-4);
        ASSERT_TRUE(dist <= 1e-4);
        ASSERT_TRUE(dev.northStarRigidIterations() == std::vector<int>{10});
        ASSERT_EQ(dev.northStarRigidMatched().first, host.northStarRigidMatched().first);  // the same cloud at the identity
        ASSERT_EQ(dev.rigidSkippedFrames(), 0);
    }
}

TEST(RigidLoopTest, TheDefaultScheduleRecoversThePlantedMotionStartsTheSolveLowerAndStopsEarly) {
    Depths in;
    DynFusion off(params(Switches{})), on(params(device_loop()));
    off.nodeStep = on.nodeStep = 64;
    ASSERT_TRUE(on.params().rigid_prealign_steps == (std::vector<int>{16, 4, 1}));
    ASSERT_TRUE(on.params().rigid_prealign_level_iters == (std::vector<int>{4, 5, 10}));
    ASSERT_TRUE(on.params().rigid_prealign_stop_rot == 1e-5f && on.params().rigid_prealign_stop_trans == 1e-5f);
    const Affine3f want = motion().inv();
    int fewest = 19;
    for (int f = 0; f < 4; ++f) {
        off(in.d[f]), on(in.d[f]);
        if (f == 0) continue;
        const Affine3f T = on.northStarRigidPose();
        const std::vector<int> ran = on.northStarRigidIterations();
        ASSERT_EQ(ran.size(), (size_t)3);
        std::printf("frame %d: iterations %d + %d + %d; matched %lld -> %lld; initial cost %.6g (off %.6g)\n", f, ran[0], ran[1], ran[2],
                    on.northStarRigidMatched().first, on.northStarRigidMatched().last, on.northStarInitialCost(), off.northStarInitialCost());
        if (f == 1) {
            for (int i = 0; i < 9; ++i) ASSERT_NEAR(T.R[i], want.R[i], 3e-3);
            for (int i = 0; i < 3; ++i) ASSERT_NEAR(T.t[i], want.t[i], 5e-3);
        }
        ASSERT_TRUE(on.northStarInitialCost() < off.northStarInitialCost());
        ASSERT_TRUE(ran[0] >= 1 && ran[0] <= 4 && ran[1] >= 1 && ran[1] <= 5 && ran[2] >= 1 && ran[2] <= 10);
        ASSERT_TRUE(on.northStarRigidMatched().first > 0);
        ASSERT_EQ(on.rigidSkippedFrames(), 0);
        fewest = std::min(fewest, ran[0] + ran[1] + ran[2]);
    }
    ASSERT_TRUE(fewest < 19);
}

TEST(RigidLoopTest, AnEmptyDepthFrameIsASkippedFrame) {
    Depths in;
    DynFusion off(params(Switches{})), on(params(device_loop()));
    off.nodeStep = on.nodeStep = 64;
    off(in.d[0]), on(in.d[0]);
    off(in.empty), on(in.empty);
    ASSERT_EQ(on.rigidSkippedFrames(), 1);
    ASSERT_TRUE(is_identity(on.northStarRigidPose()));
    ASSERT_EQ(on.northStarRigidMatched().first, 0);
    ASSERT_EQ(on.northStarRigidMatched().last, 0);
    ASSERT_TRUE(on.northStarRigidIterations() == (std::vector<int>{1, 0, 0}));  // the first system is the singular one
    ASSERT_TRUE(same(node_transforms(off), node_transforms(on)));
    ASSERT_TRUE(!node_transforms(on).empty());
}

TEST(RigidLoopTest, TheSwitchNeedsThePreAlignmentAndASchedule) {
    DynFuParams p = params(device_loop());
    ASSERT_TRUE(!construction_throws(p));
    p.north_star_rigid_prealign = false;
    ASSERT_TRUE(construction_throws(p));
    p.rigid_prealign_device = false;
    ASSERT_TRUE(!construction_throws(p));
    for (int k = 0; k < 6; ++k) {
        DynFuParams q = params(device_loop());
        if (k == 0) q.rigid_prealign_steps = {}, q.rigid_prealign_level_iters = {};
        if (k == 1) q.rigid_prealign_steps = {16, 4};
        if (k == 2) q.rigid_prealign_steps = {16, 0, 1};
        if (k == 3) q.rigid_prealign_level_iters = {40, 20, 5};
        if (k == 4) q.rigid_prealign_steps = {16, 8, 4, 2, 1}, q.rigid_prealign_level_iters = {1, 1, 1, 1, 1};
        if (k == 5) q.rigid_prealign_stop_rot = -1.f;
        ASSERT_TRUE(construction_throws(q));
        q.rigid_prealign_device = false;  // off, the fields are not looked at
        ASSERT_TRUE(!construction_throws(q));
    }
}

TEST(RigidLoopTest, WithTheSwitchOffTheNewFieldsChangeNoBit) {
    Depths in;
    Switches other = host_loop();
    other.steps = {3}, other.iters = {2}, other.stop = 1.f;
    DynFusion plain(params(host_loop())), set(params(other));
    plain.nodeStep = set.nodeStep = 64;
    for (int f = 0; f < 4; ++f) {
        plain(in.d[f]), set(in.d[f]);
        ASSERT_TRUE(same(warped_vertices(plain), warped_vertices(set)));
        ASSERT_TRUE(same(node_transforms(plain), node_transforms(set)));
        ASSERT_TRUE(!node_transforms(set).empty());
        const Affine3f a = plain.northStarRigidPose(), b = set.northStarRigidPose();
        ASSERT_TRUE(std::memcmp(a.R, b.R, sizeof a.R) == 0 && std::memcmp(a.t, b.t, sizeof a.t) == 0);
        ASSERT_TRUE(set.northStarRigidIterations().empty());
        ASSERT_TRUE(plain.northStarInitialCost() == set.northStarInitialCost() && plain.northStarFinalCost() == set.northStarFinalCost());
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
