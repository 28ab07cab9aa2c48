// test_host_icp.cpp — kfusion::cuda::ProjectiveICP::estimateTransform through the host adaptor, the way
// KinFu::operator() drives it (src/kfusion/kinfu.cpp:150-200): bilateral -> pyramids -> masked depth + normals per
// level -> ICP.  The reference has no ICP test; here a synthetic scene is rendered from two camera poses and the
// estimate must recover the relative pose.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include <kfusion/cuda/icp_update.hpp>
#include <kfusion/cuda/imgproc.hpp>
#include <kfusion/cuda/projective_icp.hpp>

#include "minitest.hpp"

using namespace kfusion;

namespace {
// depth of two spheres in front of a tilted wall (roll about the optical axis is observable), seen from camera
// pose (R, t): X_world = R X_cam + t
std::vector<unsigned short> render(int W, int H, float f, const float R[9], const float t[3]) {
    std::vector<unsigned short> d((size_t)W * H, 0);
    const float cx = W / 2 - 0.5f, cy = H / 2 - 0.5f;
    const float C[2][3] = {{0.25f, -0.1f, 1.6f}, {-0.55f, 0.3f, 2.0f}}, rad[2] = {0.45f, 0.3f};
    const float pn[3] = {0.3f, 0.2f, -0.933f}, pd = -2.6f * 0.933f;  // wall: pn . X = pd
    for (int y = 3; y < H - 3; ++y)
        for (int x = 3; x < W - 3; ++x) {
            const float dc[3] = {(x - cx) / f, (y - cy) / f, 1.f};
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
            if (best < 1e8f && best < 60.f) d[(size_t)y * W + x] = (unsigned short)std::lround(best * 1000.f);  // z_cam = s (dc.z = 1)
        }
    return d;
}

struct Pyramids {
    cuda::ProjectiveICP::DepthPyr depth;
    cuda::ProjectiveICP::NormalsPyr normals;
    cuda::ProjectiveICP::PointsPyr points;
    cuda::ProjectiveICP::NormalsPyr pnormals;
};
Pyramids build(const std::vector<unsigned short>& raw, int W, const Intr& intr, int levels) {
    Pyramids p;
    p.depth.resize(levels), p.normals.resize(levels), p.points.resize(levels), p.pnormals.resize(levels);
    cuda::Depth in;
    in.upload(raw, W);
    cuda::depthBilateralFilter(in, p.depth[0], 7, 4.5f, 0.04f);  // kinfu.cpp:150-153
    for (int i = 1; i < levels; ++i) cuda::depthBuildPyramid(p.depth[i - 1], p.depth[i], 0.04f);
    for (int i = 0; i < levels; ++i) {
        const int div = 1 << i;
        const Intr li(intr.fx / div, intr.fy / div, intr.cx / div, intr.cy / div);
        cuda::computePointNormals(li, p.depth[i], p.points[i], p.pnormals[i]);
        cuda::computeNormalsAndMaskDepth(li, p.depth[i], p.normals[i]);  // kinfu.cpp:161-167
    }
    return p;
}
}  // namespace

TEST(ProjectiveIcpTest, DefaultsAndLevels) {
    cuda::ProjectiveICP icp;
    ASSERT_NEAR(icp.getDistThreshold(), 0.1f, 1e-9);
    ASSERT_NEAR(icp.getAngleThreshold(), 20.f * 0.017453293f, 1e-9);
    ASSERT_EQ(icp.getUsedLevelsNum(), 3);  // {10, 5, 4, 0}
    icp.setIterationsNum({3});
    ASSERT_EQ(icp.getUsedLevelsNum(), 1);
    icp.setIterationsNum({1, 2, 3, 4, 5, 6});
    ASSERT_EQ(icp.getUsedLevelsNum(), 4);
}

TEST(ProjectiveIcpTest, EstimateTransformRecoversTheCameraMotion) {
    const int W = 320, H = 240;
    const Intr intr(262.5f, 262.5f, W / 2 - 0.5f, H / 2 - 0.5f);
    // previous camera at the origin; current camera rotated by 1.2 degrees about y and moved by (15, -8, 10) mm
    const float a = 0.021f, Rc[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)}, tc[3] = {0.015f, -0.008f, 0.010f};
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
    Pyramids prev = build(render(W, H, intr.fx, I, z), W, intr, 3), curr = build(render(W, H, intr.fx, Rc, tc), W, intr, 3);
    cuda::ProjectiveICP icp;
    icp.setDistThreshold(0.1f), icp.setAngleThreshold(30.f * 0.017453293f);  // kinfu.cpp:31-32
    for (int variant = 0; variant < 2; ++variant) {
        Affine3f est;
        const bool ok = variant == 0 ? icp.estimateTransform(est, intr, curr.depth, curr.normals, prev.depth, prev.normals)
                                     : icp.estimateTransform(est, intr, curr.points, curr.pnormals, prev.points, prev.pnormals);
        ASSERT_TRUE(ok);
        // the estimate maps current-camera coordinates into the previous camera's frame: X_prev = R_c X_cur + t_c
        for (int i = 0; i < 9; ++i) ASSERT_NEAR(est.R[i], Rc[i], 3e-3);
        for (int i = 0; i < 3; ++i) ASSERT_NEAR(est.t[i], tc[i], 5e-3);
    }
    // nothing to align against: the normal equations are singular and the reference returns false (:136-142)
    cuda::ProjectiveICP::DepthPyr empty(3);
    cuda::ProjectiveICP::NormalsPyr nempty(3);
    for (int i = 0; i < 3; ++i) {
        std::vector<unsigned short> zeros((size_t)(W >> i) * (H >> i), 0);
        empty[i].upload(zeros, W >> i);
        const int div = 1 << i;
        cuda::computeNormalsAndMaskDepth(Intr(intr.fx / div, intr.fy / div, intr.cx / div, intr.cy / div), empty[i], nempty[i]);
    }
    Affine3f est;
    ASSERT_TRUE(!icp.estimateTransform(est, intr, empty, nempty, prev.depth, prev.normals));
}

namespace {
// minimal reader of tests/golden/icp_update_kat.json (tests/golden/make_icp_update_kat.py): per case the keys "sums",
// "before", "ok", "check_affine", "after" in that order; a null among the sums is a NaN (JSON has no token for it)
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
    std::string dir = __FILE__;  // tests/cpp/test_host_icp.cpp
    dir = dir.substr(0, dir.find_last_of('/') + 1) + "../golden/icp_update_kat.json";
    const char* env = std::getenv("DFA_ICP_UPDATE_KAT");
    std::ifstream in(env ? std::string(env) : dir);
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
}  // namespace

// kfusion::cuda::icp_update against the float64 statement's known answers (tests/img_statement.py:icp_update): `ok`
// exactly; every entry of the next affine within 2 float32 ulps of its magnitude or 1e-7, whichever is larger (both
// sides solve in double).  At the two systems on the determinant gate only `ok`.  Needs no GPU.
TEST(ProjectiveIcpTest, IcpUpdateKnownAnswers) {
    const std::vector<KatCase> kat = read_kat();
    ASSERT_EQ(kat.size(), (size_t)9);
    for (const KatCase& c : kat) {
        Affine3f a;
        for (int i = 0; i < 9; ++i) a.R[i] = c.before[i];
        for (int i = 0; i < 3; ++i) a.t[i] = c.before[9 + i];
        const bool ok = cuda::icp_update(c.sums, a);
        if (ok != c.ok) throw mt::Failure{c.name + ": ok differs from the statement's"};
        if (!c.check_affine) continue;
        float got[12];
        a.to12(got);
        for (int i = 0; i < 12; ++i) {
            const double want = c.after[i], tol = std::fmax(2.0 * std::ldexp(1.0, std::ilogb(std::fabs(want) > 0 ? std::fabs(want) : 1e-30) - 23), 1e-7);
            if (!(std::fabs((double)got[i] - want) <= tol)) {
                char buf[200];
                std::snprintf(buf, sizeof buf, "%s: affine[%d] = %.9g, statement %.9g, tolerance %.3g", c.name.c_str(), i, got[i], want, tol);
                throw mt::Failure{buf};
            }
        }
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
