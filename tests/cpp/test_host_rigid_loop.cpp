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
#include "minitest.hpp"

using namespace kfusion;

namespace {
// -------------------------------------------------------------------------------------------------------- the sequence
// test_host_icp.cpp's image.  The volume is the smallest cube that holds the scene: 2.2 m from z = 1 m — the spheres reach
// from x = -0.85 to 0.7 and from z = 1.15, the wall crosses the cube between z = 2.01 and 3.19 — at 256 voxels a side.  The
// voxel size matters to the first check below: the integration takes voxel i at i * voxel, marching cubes puts its vertices
// at (i + 0.5) * voxel (both as the reference does), so the canonical model stands half a voxel, 4.3 mm, off the scene it
// was fused from, along every axis.  The rigid estimate maps the MODEL into the live camera, offset included: 4.3 of the
// 5 mm of the translation bar are that offset (measured: 4.1, 4.5, 4.3 mm; at 128 voxels a side and 3 m it is 11.7 mm).
const int W = 320, H = 240, DIM = 256;
const float F = 262.5f, VOLUME = 2.2f, VOLUME_Z0 = 1.0f;

// test_host_icp.cpp's scene: depth of two spheres in front of a tilted wall seen from camera pose X_world = R X_cam + t
std::vector<unsigned short> render(const float R[9], const float t[3]) {
    std::vector<unsigned short> d((size_t)W * H, 0);
    const float cx = W / 2 - 0.5f, cy = H / 2 - 0.5f;
    const float C[2][3] = {{0.25f, -0.1f, 1.6f}, {-0.55f, 0.3f, 2.0f}}, rad[2] = {0.45f, 0.3f};
    const float pn[3] = {0.3f, 0.2f, -0.933f}, pd = -2.6f * 0.933f;  // wall: pn . X = pd
    for (int y = 3; y < H - 3; ++y)
        for (int x = 3; x < W - 3; ++x) {
            const float dc[3] = {(x - cx) / F, (y - cy) / F, 1.f};
            float dw[3], best = 1e9f;
            for (int i = 0; i < 3; ++i) dw[i] = R[3 * i] * dc[0] + R[3 * i + 1] * dc[1] + R[3 * i + 2] * dc[2];
            for (int k = 0; k < 2; ++k) {
                const float oc[3] = {t[0] - C[k][0], t[1] - C[k][1], t[2] - C[k][2]};
                const float a = dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2], b = 2 * (oc[0] * dw[0] + oc[1] * dw[1] + oc[2] * dw[2]),
                            c = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - rad[k] * rad[k], disc = b * b - 4 * a * c;
                if (disc > 0) {
                    const float s = (-b - std::sqrt(disc)) / (2 * a);
                    if (s > 0 && s < best) best = s;
                }
            }
            const float den = pn[0] * dw[0] + pn[1] * dw[1] + pn[2] * dw[2];
            if (std::fabs(den) > 1e-6f) {
                const float s = (pd - (pn[0] * t[0] + pn[1] * t[1] + pn[2] * t[2])) / den;
                if (s > 0 && s < best) best = s;
            }
            if (best < 1e8f && best < 60.f) d[(size_t)y * W + x] = (unsigned short)std::lround(best * 1000.f);
        }
    return d;
}

// the planted motion of test_host_icp.cpp: 1.2 degrees about y, (15, -8, 10) mm: X_before = M X_after
Affine3f motion() {
    const float a = 0.021f;
    Affine3f m;
    const float R[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)};
    for (int i = 0; i < 9; ++i) m.R[i] = R[i];
    m.t[0] = 0.015f, m.t[1] = -0.008f, m.t[2] = 0.010f;
    return m;
}

struct Depths {
    cuda::Depth d[4], empty;
    Depths() {
        Affine3f pose;  // frame f's camera: X_world = M^f X_cam
        for (int f = 0; f < 4; ++f) {
            d[f].upload(render(pose.R, pose.t), W);
            pose = pose * motion();
        }
        empty.upload(std::vector<unsigned short>((size_t)W * H, 0), W);
    }
};

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

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
std::vector<float> warped_vertices(DynFusion& df) {
    std::vector<float> v;
    dfa::DeviceArray<float> v3, n3;
    df.getCanonicalWarpedToLive()->deviceArrays(v3, n3);
    if (df.getCanonicalWarpedToLive()->size()) v3.download(v);
    return v;
}
std::vector<float> node_transforms(DynFusion& df) {
    std::vector<float> pos, w, dq;
    df.getWarpfield()->hostArrays(pos, w, dq);
    return dq;
}
bool is_identity(const Affine3f& a) {
    const Affine3f i;
    return std::memcmp(a.R, i.R, sizeof a.R) == 0 && std::memcmp(a.t, i.t, sizeof a.t) == 0;
}
bool construction_throws(const DynFuParams& p) {
    try {
        DynFusion df(p);
    } catch (const dfa::Error& e) {
        return e.code == DFA_ERR_INVALID;
    }
    return false;
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
