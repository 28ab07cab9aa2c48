// test_host_rigid_align.cpp — the rigid pre-alignment of north-star mode (DynFuParams::north_star_rigid_prealign,
// rigid_prealign_iters; Warpfield::composeRigid, NorthStarSolver::alignRigid; DynFusion::northStarRigidPose,
// northStarRigidMatched, rigidSkippedFrames).  composeRigid against the float64 statement's known answers; then four-frame
// north-star sequences on the scene of test_host_icp.cpp (two spheres before a tilted wall) with the camera moved by that
// test's motion per frame, cumulatively: the estimate is the inverse of the planted motion, the solve starts from a lower
// energy than without the step, zero iterations change nothing, an empty depth frame skips the step, the other switches run
// with it, and the switch's rule.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
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
// ---------------------------------------------------------------------------------------------- composeRigid's fixture
// minimal reader of tests/golden/rigid_compose_kat.json (tests/golden/make_rigid_compose_kat.py): per case the keys "T",
// "dq", "after" in that order
const int KAT_D = 5;
struct KatCase {
    std::string name;
    float T[12], dq[8 * KAT_D], after[8 * KAT_D];
};
void read_floats(const std::string& s, size_t& at, const char* key, float* out, int n) {
    at = s.find(std::string("\"") + key + "\":", at);
    if (at == std::string::npos) throw mt::Failure{std::string("rigid_compose_kat.json: missing key ") + key};
    const char* p = std::strchr(s.c_str() + at, '[') + 1;
    for (int i = 0; i < n; ++i) {
        while (*p == ' ' || *p == '\n') ++p;
        char* end;
        out[i] = (float)std::strtod(p, &end);  // the fixture holds float32 values: exact
        if (end == p) throw mt::Failure{std::string("rigid_compose_kat.json: short array ") + key};
        p = end;
        while (*p == ',' || *p == ' ' || *p == '\n') ++p;
    }
    at = (size_t)(p - s.c_str());
}
std::vector<KatCase> read_kat() {
    std::string dir = __FILE__;  // tests/cpp/test_host_rigid_align.cpp
    dir = dir.substr(0, dir.find_last_of('/') + 1) + "../golden/rigid_compose_kat.json";
    std::ifstream in(dir);
    if (!in) in.open("tests/golden/rigid_compose_kat.json");
    if (!in) throw mt::Failure{"rigid_compose_kat.json not found"};
    const std::string s((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<KatCase> out;
    for (size_t at = s.find("\"name\":"); at != std::string::npos; at = s.find("\"name\":", at)) {
        KatCase c;
        const size_t q0 = s.find('"', at + 7) + 1;
        c.name          = s.substr(q0, s.find('"', q0) - q0);
        read_floats(s, at, "T", c.T, 12);
        read_floats(s, at, "dq", c.dq, 8 * KAT_D);
        read_floats(s, at, "after", c.after, 8 * KAT_D);
        out.push_back(c);
    }
    return out;
}
void check_entries(const std::string& name, const float* got, const float* want_f, int n) {
    for (int i = 0; i < n; ++i) {  // test_host_icp.cpp's bar: 2 float32 ulps of the entry's magnitude or 1e-7
        const double want = want_f[i], tol = std::fmax(2.0 * std::ldexp(1.0, std::ilogb(std::fabs(want) > 0 ? std::fabs(want) : 1e-30) - 23), 1e-7);
        if (!(std::fabs((double)got[i] - want) <= tol)) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "%s: dq[%d] = %.9g, statement %.9g, tolerance %.3g", name.c_str(), i, got[i], want, tol);
            throw mt::Failure{buf};
        }
    }
}

// -------------------------------------------------------------------------------------------------------- the sequence
// (the planted-motion scene of dynfu_fixtures.hpp: 320 x 240, 256^3 voxels over 2.2 m)

struct Switches {
    bool prealign = false, everything = false;
    int iters = 10;
    // every PCG gets its full launch budget.  The adaptive budget (NorthStarParameters::adaptiveLaunch) is sized from the solves a
    // PLAN has seen, and the plans travel between the solvers of a process through the plan cache: two runs that are compared
    // bit for bit must not depend on which of them ran first
    bool full_budget = false;
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
    p.north_star_rigid_prealign = s.prealign, p.rigid_prealign_iters = s.iters;
    p.northStarParams.adaptiveLaunch = !s.full_budget;
    if (s.everything) {
        p.north_star_fuse_canonical = p.fuse_unsupported_rigid = p.north_star_regrow_canonical = true;
        p.model_view = p.north_star_visible_only = true;
    }
    return p;
}
}  // namespace

// Warpfield::composeRigid against the float64 statement's known answers (tests/rigid_align_statement.py:compose_rigid).  Needs
// no GPU.
TEST(RigidAlignTest, ComposeRigidKnownAnswers) {
    const std::vector<KatCase> kat = read_kat();
    ASSERT_EQ(kat.size(), (size_t)7);
    for (const KatCase& c : kat) {
        Affine3f T;
        for (int i = 0; i < 9; ++i) T.R[i] = c.T[i];
        for (int i = 0; i < 3; ++i) T.t[i] = c.T[9 + i];
        float dq[8 * KAT_D];
        std::memcpy(dq, c.dq, sizeof dq);
        Warpfield::composeRigid(T, dq, KAT_D);
        check_entries(c.name, dq, c.after, 8 * KAT_D);
    }
}

TEST(RigidAlignTest, TheEstimateIsTheInverseOfThePlantedMotionAndTheSolveStartsLower) {
    Depths in;
    Switches on_s;
    on_s.prealign = true;
    DynFusion off(params(Switches{})), on(params(on_s));
    off.nodeStep = on.nodeStep = 64;
    const Affine3f want = motion().inv();  // the model, in frame 0's camera frame, into frame 1's camera frame
    for (int f = 0; f < 4; ++f) {
        ASSERT_TRUE(off(in.d[f]) == (f > 0));
        ASSERT_TRUE(on(in.d[f]) == (f > 0));
        ASSERT_TRUE(is_identity(off.northStarRigidPose()));
        ASSERT_EQ(off.rigidSkippedFrames(), 0);
        if (f == 0) {
            ASSERT_TRUE(is_identity(on.northStarRigidPose()));
            continue;
        }
        const Affine3f T = on.northStarRigidPose();
        const DynFusion::RigidMatched m = on.northStarRigidMatched();
        std::printf("frame %d: R err %.2e, t err %.2e; matched %lld -> %lld of %zu; initial cost %.6g (off %.6g), final %.6g (off %.6g), rows %lld (off %lld)\n",
                    f, std::fabs(T.R[2] - want.R[2]), std::fabs(T.t[0] - want.t[0]), m.first, m.last, on.canonicalVertexCount(),
                    on.northStarInitialCost(), off.northStarInitialCost(), on.northStarFinalCost(), off.northStarFinalCost(),
                    on.northStarValidRows(), off.northStarValidRows());
        if (f == 1) {
            for (int i = 0; i < 9; ++i) ASSERT_NEAR(T.R[i], want.R[i], 3e-3);
            for (int i = 0; i < 3; ++i) ASSERT_NEAR(T.t[i], want.t[i], 5e-3);
        }
        ASSERT_TRUE(!is_identity(T));
        ASSERT_TRUE(on.northStarInitialCost() < off.northStarInitialCost());
        ASSERT_TRUE(m.first > 0 && m.last >= m.first);
        ASSERT_EQ(on.rigidSkippedFrames(), 0);
    }
}

TEST(RigidAlignTest, ZeroIterationsChangeNothing) {
    Depths in;
    Switches plain, zero;
    plain.full_budget = zero.full_budget = true;
    zero.prealign = true, zero.iters = 0;
    DynFusion off(params(plain)), on(params(zero));
    off.nodeStep = on.nodeStep = 64;
    for (int f = 0; f < 4; ++f) {
        off(in.d[f]), on(in.d[f]);
        ASSERT_TRUE(same(warped_vertices(off), warped_vertices(on)));
        ASSERT_TRUE(same(node_transforms(off), node_transforms(on)));
        ASSERT_TRUE(!node_transforms(on).empty());
        ASSERT_TRUE(is_identity(on.northStarRigidPose()));
        ASSERT_EQ(on.rigidSkippedFrames(), 0);
    }
}

TEST(RigidAlignTest, AnEmptyDepthFrameSkipsTheAlignmentAndLeavesTheNodesToTheSolve) {
    Depths in;
    Switches on_s;
    on_s.prealign = true;
    // frame 0, then an all-zero depth frame: the rigid system is singular.  The step is skipped and counted, and the frame is
    // the one the sequence without the step produces, node for node
    Switches plain;
    plain.full_budget = on_s.full_budget = true;
    DynFusion off(params(plain)), on(params(on_s));
    off.nodeStep = on.nodeStep = 64;
    off(in.d[0]), on(in.d[0]);
    off(in.empty), on(in.empty);
    ASSERT_EQ(on.rigidSkippedFrames(), 1);
    ASSERT_TRUE(is_identity(on.northStarRigidPose()));
    ASSERT_EQ(on.northStarRigidMatched().first, 0);
    ASSERT_EQ(on.northStarRigidMatched().last, 0);
    ASSERT_TRUE(same(node_transforms(off), node_transforms(on)));
    ASSERT_TRUE(!node_transforms(on).empty());
}

TEST(RigidAlignTest, RunsWithEveryOtherNorthStarSwitch) {
    Depths in;
    Switches all, all_on;
    all.everything = all_on.everything = true, all_on.prealign = true;
    DynFusion off(params(all)), on(params(all_on));
    off.nodeStep = on.nodeStep = 64;
    for (int f = 0; f < 4; ++f) {
        off(in.d[f]), on(in.d[f]);
        if (f == 0) continue;
        std::printf("frame %d: valid rows %lld (off %lld), visible %lld (off %lld), %zu canonical vertices (off %zu)\n", f,
                    on.northStarValidRows(), off.northStarValidRows(), on.northStarVisibleVertices(), off.northStarVisibleVertices(),
                    on.canonicalVertexCount(), off.canonicalVertexCount());
        ASSERT_TRUE(on.northStarValidRows() >= off.northStarValidRows());
        ASSERT_TRUE(on.northStarValidRows() > 0);
        ASSERT_EQ(on.rigidSkippedFrames(), 0);
    }
}

TEST(RigidAlignTest, TheSwitchNeedsNorthStar) {
    Switches on_s;
    on_s.prealign = true;
    DynFuParams p = params(on_s);
    ASSERT_TRUE(!construction_throws(p));
    p.north_star = false;
    ASSERT_TRUE(construction_throws(p));
    p.north_star_rigid_prealign = false;
    ASSERT_TRUE(!construction_throws(p));
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
