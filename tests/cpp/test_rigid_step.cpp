// test_rigid_step.cpp — dynfu_amd/csrc/rigid_step.hpp on the CPU: no HIP, no library.  The step against the known answers
// of kfusion::cuda::icp_update (tests/golden/icp_update_kat.json, the fixture of test_host_icp.cpp) at that test's bar —
// `ok` exactly, every entry of the next pose within 2 float32 ulps of its magnitude or 1e-7, the refused cases with the pose
// untouched — and the rules of the loop (rigid_loop_advance) on sums taken from the same fixture.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "../../dynfu_amd/csrc/rigid_step.hpp"
#include "minitest.hpp"

using namespace dfa;

namespace {
// per case the keys "sums", "before", "ok", "check_affine", "after" in that order; a null among the sums is a NaN
struct KatCase {
    std::string name;
    float sums[27], before[12], after[12];
    bool ok, check_affine;
};
const char* after_key(const std::string& s, size_t& at, const char* key) {
    at = s.find(std::string("\"") + key + "\":", at);
    if (at == std::string::npos) throw mt::Failure{std::string("icp_update_kat.json: missing key ") + key};
    at += std::strlen(key) + 3;
    return s.c_str() + at;
}
void read_floats(const std::string& s, size_t& at, const char* key, float* out, int n) {
    const char* p = std::strchr(after_key(s, at, key), '[') + 1;
    for (int i = 0; i < n; ++i) {
        while (*p == ' ' || *p == '\n') ++p;
        char* end;
        if (std::strncmp(p, "null", 4) == 0) out[i] = std::nanf(""), end = const_cast<char*>(p) + 4;
        else out[i] = (float)std::strtod(p, &end);  // the fixture holds float32 values: exact
        if (end == p) throw mt::Failure{std::string("icp_update_kat.json: short array ") + key};
        p = end;
        while (*p == ',' || *p == ' ' || *p == '\n') ++p;
    }
}
bool read_bool(const std::string& s, size_t& at, const char* key) {
    const char* p = after_key(s, at, key);
    while (*p == ' ') ++p;
    return std::strncmp(p, "true", 4) == 0;
}
std::vector<KatCase> read_kat() {
    std::string path = __FILE__;  // tests/cpp/test_rigid_step.cpp
    path = path.substr(0, path.find_last_of('/') + 1) + "../golden/icp_update_kat.json";
    const char* env = std::getenv("DFA_ICP_UPDATE_KAT");
    std::ifstream in(env ? std::string(env) : path);
    if (!in) in.open("tests/golden/icp_update_kat.json");
    if (!in) throw mt::Failure{"icp_update_kat.json not found (DFA_ICP_UPDATE_KAT names it)"};
    const std::string s((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<KatCase> out;
    for (size_t at = s.find("\"name\":"); at != std::string::npos; at = s.find("\"name\":", at)) {
        KatCase c;
        const size_t q0 = s.find('"', at + 7) + 1;
        c.name          = s.substr(q0, s.find('"', q0) - q0);
        read_floats(s, at, "sums", c.sums, 27);
        read_floats(s, at, "before", c.before, 12);
        c.ok           = read_bool(s, at, "ok");
        c.check_affine = read_bool(s, at, "check_affine");
        read_floats(s, at, "after", c.after, 12);
        out.push_back(c);
    }
    return out;
}
double bar(double want) { return std::fmax(2.0 * std::ldexp(1.0, std::ilogb(std::fabs(want) > 0 ? std::fabs(want) : 1e-30) - 23), 1e-7); }

const KatCase& named(const std::vector<KatCase>& kat, bool ok) {
    for (const KatCase& c : kat)
        if (c.ok == ok && (c.check_affine || !ok)) return c;
    throw mt::Failure{"no such case in the fixture"};
}
const float IDENT[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
}  // namespace

TEST(RigidStepTest, KnownAnswers) {
    const std::vector<KatCase> kat = read_kat();
    ASSERT_EQ(kat.size(), (size_t)9);
    int refused = 0;
    for (const KatCase& c : kat) {
        float aff[12];
        std::memcpy(aff, c.before, sizeof aff);
        const RigidStep r = rigid_step(c.sums, aff);
        if (r.ok != c.ok) throw mt::Failure{c.name + ": ok differs from the statement's"};
        if (!r.ok) {
            ++refused;
            if (std::memcmp(aff, c.before, sizeof aff) != 0) throw mt::Failure{c.name + ": a refused update touched the pose"};
            ASSERT_TRUE(r.rot == 0.0 && r.trans == 0.0);
            continue;
        }
        ASSERT_TRUE(r.rot >= 0.0 && r.trans >= 0.0);
        if (!c.check_affine) continue;
        for (int i = 0; i < 12; ++i)
            if (!(std::fabs((double)aff[i] - (double)c.after[i]) <= bar(c.after[i]))) {
                char buf[200];
                std::snprintf(buf, sizeof buf, "%s: affine[%d] = %.9g, statement %.9g, tolerance %.3g", c.name.c_str(), i, aff[i], c.after[i], bar(c.after[i]));
                throw mt::Failure{buf};
            }
    }
    ASSERT_TRUE(refused >= 1);
}

// the twist's norms are those of the increment: from the identity the pose IS the increment, |tvec| = |t| and the
// rotation angle = acos((trace - 1) / 2), both to float32 rounding of the pose
TEST(RigidStepTest, NormsAreTheIncrements) {
    const std::vector<KatCase> kat = read_kat();
    const KatCase& c = named(kat, true);
    float aff[12];
    std::memcpy(aff, IDENT, sizeof aff);
    const RigidStep r = rigid_step(c.sums, aff);
    ASSERT_TRUE(r.ok);
    ASSERT_NEAR(r.trans, std::sqrt((double)aff[9] * aff[9] + (double)aff[10] * aff[10] + (double)aff[11] * aff[11]), 1e-6);
    // sin of the angle from the antisymmetric part (well conditioned at small angles, where acos of the trace is not)
    const double ax = 0.5 * ((double)aff[7] - aff[5]), ay = 0.5 * ((double)aff[2] - aff[6]), az = 0.5 * ((double)aff[3] - aff[1]);
    ASSERT_NEAR(std::sin(r.rot), std::sqrt(ax * ax + ay * ay + az * az), 1e-6);
}

TEST(RigidLoopTest, ZeroThresholdsNeverStopAndThePoseStartsAtAff0) {
    const std::vector<KatCase> kat = read_kat();
    const KatCase& c = named(kat, true);
    RigidLoopState st;
    std::memset(&st, 0, sizeof st);
    float pose[12], want[12];
    rigid_loop_pose(st, c.before, pose);
    ASSERT_TRUE(std::memcmp(pose, c.before, sizeof pose) == 0);  // a zeroed state: aff0, not twelve zeros
    std::memcpy(want, c.before, sizeof want);
    for (int it = 0; it < 3; ++it) {
        ASSERT_TRUE(rigid_loop_active(st, 1));
        rigid_loop_advance(st, c.before, 1, it, c.sums, 0.f, 0.f);
        rigid_step(c.sums, want);
        ASSERT_TRUE(st.have_pose == 1 && std::memcmp(st.aff, want, sizeof want) == 0);
    }
    ASSERT_TRUE(st.status == 0 && st.iters_run[1] == 3 && st.iters_run[0] == 0 && st.last_iter == 2 && !st.finished[1]);
    ASSERT_TRUE(st.last_rot > 0.f && st.last_trans > 0.f);
}

TEST(RigidLoopTest, AStepUnderBothThresholdsFinishesItsLevelOnly) {
    const std::vector<KatCase> kat = read_kat();
    const KatCase& c = named(kat, true);
    float aff[12];
    std::memcpy(aff, IDENT, sizeof aff);
    const RigidStep r = rigid_step(c.sums, aff);
    const float above_rot = (float)(r.rot * 2), above_trans = (float)(r.trans * 2), below_rot = (float)(r.rot / 2),
                below_trans = (float)(r.trans / 2);
    const float th[4][2] = {{above_rot, above_trans}, {below_rot, above_trans}, {above_rot, below_trans}, {1e30f, 1e30f}};
    const bool stops[4]  = {true, false, false, true};
    for (int k = 0; k < 4; ++k) {
        RigidLoopState st;
        std::memset(&st, 0, sizeof st);
        rigid_loop_advance(st, IDENT, 0, 0, c.sums, th[k][0], th[k][1]);
        ASSERT_TRUE(st.status == 0 && st.iters_run[0] == 1);
        ASSERT_EQ(rigid_loop_active(st, 0), !stops[k]);
        ASSERT_TRUE(rigid_loop_active(st, 1) && rigid_loop_active(st, 3));  // the next level starts from the pose reached
        ASSERT_TRUE(std::memcmp(st.aff, aff, sizeof aff) == 0);
    }
    // the compare is strict: a threshold equal to the norm does not stop, and a NaN norm never does
    RigidLoopState st;
    std::memset(&st, 0, sizeof st);
    rigid_loop_advance(st, IDENT, 0, 0, c.sums, (float)r.rot, 1e30f);
    ASSERT_EQ(rigid_loop_active(st, 0), !((double)(float)r.rot > r.rot));
}

TEST(RigidLoopTest, ARefusedUpdateEndsEveryLevelAndKeepsThePose) {
    const std::vector<KatCase> kat = read_kat();
    const KatCase &good = named(kat, true), &bad = named(kat, false);
    RigidLoopState st;
    std::memset(&st, 0, sizeof st);
    rigid_loop_advance(st, IDENT, 0, 0, good.sums, 0.f, 0.f);
    float reached[12];
    std::memcpy(reached, st.aff, sizeof reached);
    const float rot = st.last_rot, trans = st.last_trans;
    rigid_loop_advance(st, IDENT, 0, 1, bad.sums, 0.f, 0.f);
    ASSERT_TRUE(st.status == 1 && st.iters_run[0] == 2 && st.last_iter == 1);
    ASSERT_TRUE(std::memcmp(reached, st.aff, sizeof reached) == 0 && st.last_rot == rot && st.last_trans == trans);
    for (int l = 0; l < RIGID_MAX_LEVELS; ++l) ASSERT_TRUE(!rigid_loop_active(st, l));
    // all-zero sums (an empty cloud) are refused at the first pivot
    RigidLoopState empty;
    std::memset(&empty, 0, sizeof empty);
    const float zeros[27] = {};
    rigid_loop_advance(empty, IDENT, 0, 0, zeros, 0.f, 0.f);
    ASSERT_TRUE(empty.status == 1 && empty.iters_run[0] == 1 && empty.have_pose == 0);
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
