// test_host_visible_term.cpp — the north-star data term over the visible model surface through the C++ host adaptor:
// kfusion::cuda::visibleVertices on the two-plane case of tests/visibility_cases.py, DynFuParams::north_star_visible_only on
// the synthetic sphere of test_host_mesh_view.cpp (the front surface is the whole model: every vertex is visible, so frames
// with the switch on are the frames with it off, bit for bit), the count against the rule stated on the device's dumped
// model map, and the constructor's throws.  (dfa_visible_vertices itself is checked against the numpy statement by
// tests/test_gpu_visibility.py, the mask of the plan by tests/test_gpu_solve6_vertex_mask.py.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include <dynfu/dyn_fusion.hpp>
#include <kfusion/cuda/mesh_render.hpp>

#include "../../include/dynfu_amd.h"
#include "dynfu_fixtures.hpp"
#include "minitest.hpp"

using namespace kfusion;
using dynfu_fixtures::construction_throws;
using namespace dynfu_fixtures::sphere_scene;

namespace {
// The sphere frames run on a 128^3 volume, not test_host_mesh_view.cpp's 64^3.  At 64^3 (47 mm voxels, 16 nodes at frame 0)
// frame 1's solve leaves the model 34 mm from the canonical one on average for a 10 mm step, Warpfield::update then adds 46
// nodes with identity transforms at the rim, and the model frame 2 starts from folds over itself there: 71.3 % of the cloud
// is visible in frame 2 (1 411 of 1 980; the solve with the switch off keeps 976 valid rows of frame 1's 1 924), 89.7 % at
// 96^3 (4 170 of 4 647).  128^3 is the nearest size at which the front surface stays the whole model in all three frames
// (8 802 of 8 802 in each; profiles/visible_data_term.md).
DynFuParams small_params(bool model_view, bool north_star, bool visible_only, int dim = 128) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(dim);
    p.kinfuParams.light_pose = Vec3f(0.2f, 0.1f, 0.f);
    p.epsilon = 0.05f;
    p.mesh_normals = true;
    p.model_view = model_view, p.north_star = north_star, p.north_star_visible_only = visible_only;
    return p;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

struct FrameOutputs {
    bool flag;
    std::vector<dfa::PointXYZ> warped;
    std::vector<dfa::Normal> warped_n;
    std::vector<float> pos, w, dq;
    double cost0, cost1;
    long long valid;
};
FrameOutputs outputs(DynFusion& df, bool flag) {
    FrameOutputs o;
    o.flag = flag;
    o.warped = df.getCanonicalWarpedToLive()->vertices().points, o.warped_n = df.getCanonicalWarpedToLive()->normals().points;
    df.getWarpfield()->hostArrays(o.pos, o.w, o.dq);
    o.cost0 = df.northStarInitialCost(), o.cost1 = df.northStarFinalCost(), o.valid = df.northStarValidRows();
    return o;
}
bool same(const FrameOutputs& a, const FrameOutputs& b) {
    return a.flag == b.flag && same(a.warped, b.warped) && same(a.warped_n, b.warped_n) && same(a.pos, b.pos) && same(a.w, b.w) &&
           same(a.dq, b.dq) && std::memcmp(&a.cost0, &b.cost0, sizeof(double)) == 0 && std::memcmp(&a.cost1, &b.cost1, sizeof(double)) == 0 &&
           a.valid == b.valid;
}

// the rule of dfa_visible_vertices (include/dynfu_amd.h) on host copies: float32 operations in its order, std::fmaf and
// std::nearbyintf (round to nearest even) where it has fmaf and rintf
unsigned char visible_by_rule(const float* p, const std::vector<Point>& map, int cols, int rows, const Intr& intr, float z_tol) {
    const float x = p[0], y = p[1], z = p[2];
    if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z)) || z <= 0.f) return 0;
    const volatile float qx = x / z, qy = y / z;
    const float u = std::fmaf(intr.fx, qx, intr.cx), v = std::fmaf(intr.fy, qy, intr.cy);
    const float ru = std::nearbyintf(u), rv = std::nearbyintf(v);
    if (!(ru >= 0.f && ru <= (float)(cols - 1) && rv >= 0.f && rv <= (float)(rows - 1))) return 0;
    const Point& m = map[(size_t)(int)rv * cols + (int)ru];
    if (m.x != m.x) return 1;
    const volatile float limit = m.z + z_tol;
    return z <= limit ? 1 : 0;
}
}  // namespace

TEST(VisibleTermTest, ConstructorNeedsNorthStarAndModelView) {
    ASSERT_TRUE(construction_throws(small_params(false, true, true)));   // without model_view
    ASSERT_TRUE(construction_throws(small_params(true, false, true)));   // without north_star
    ASSERT_TRUE(construction_throws(small_params(false, false, true)));
    ASSERT_TRUE(!construction_throws(small_params(true, true, true)));
    ASSERT_TRUE(!construction_throws(small_params(true, true, false)));
    DynFusion df(small_params(true, true, true));
    ASSERT_EQ(df.northStarVisibleVertices(), -1ll);  // before a frame
}

// tests/visibility_cases.py: two_planes — a 64 x 48 image, a near quad at z = 1 over the left 40 columns, 1 031 points on
// the plane z = 1.5 all over the image and the quad's own vertices
TEST(VisibleTermTest, VisibleVerticesOnTheTwoPlaneCase) {
    const int cols = 64, rows = 48, quad_cols = 40, n_plane = 1031;
    const Intr intr(60.f, 60.f, 31.5f, 23.5f);
    const float u0 = -0.25f, u1 = quad_cols - 0.75f, v0 = -0.25f, v1 = rows - 0.75f;
    const float corner[4][2] = {{u0, v0}, {u1, v0}, {u1, v1}, {u0, v1}};
    std::vector<dfa::PointXYZ> quad;
    for (const auto& c : corner) quad.push_back(dfa::PointXYZ((c[0] - intr.cx) / intr.fx, (c[1] - intr.cy) / intr.fy, 1.f));
    dfa::DeviceArray<dfa::PointXYZ> dq;
    dfa::DeviceArray<dfa::Normal> none;
    dfa::DeviceArray<int> di;
    dq.upload(quad), di.upload(std::vector<int>{0, 1, 2, 0, 2, 3});
    cuda::Cloud points;
    cuda::Normals normals;
    dfa::DeviceArray<uint64_t> zb;
    cuda::rasterizeMesh(dq, none, di, Affine3f(), intr, cols, rows, 0.1f, points, normals, zb);
    // the cloud, stride 3, and what its geometry says
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> du(-0.4f, cols - 0.6f), dv(-0.4f, rows - 0.6f);
    std::vector<float> cloud;
    std::vector<unsigned char> expected;
    const float edge = quad_cols - 0.5f, z = 1.5f;
    for (int i = 0; i < n_plane; ++i) {
        float u = du(rng);
        const float v = dv(rng);
        if (std::fabs(u - edge) < 0.05f) u += 0.1f;
        cloud.insert(cloud.end(), {(u - intr.cx) * z / intr.fx, (v - intr.cy) * z / intr.fy, z});
        expected.push_back(u > edge ? 1 : 0);
    }
    for (const auto& p : quad) cloud.insert(cloud.end(), {p.x, p.y, p.z}), expected.push_back(1);
    dfa::DeviceArray<float> dc;
    dc.upload(cloud);
    dfa::DeviceArray<unsigned char> flags;
    dfa::DeviceArray<int> count;
    cuda::visibleVertices(dc.ptr(), 3, expected.size(), points, intr, 0.01f, flags, &count);
    std::vector<unsigned char> got;
    std::vector<int> n;
    flags.download(got), count.download(n);
    ASSERT_EQ(got.size(), expected.size());
    size_t wrong = 0, set = 0;
    for (size_t i = 0; i < got.size(); ++i) wrong += got[i] != expected[i], set += expected[i];
    std::printf("two planes: %zu vertices, %zu visible, %zu differ from the geometry\n", got.size(), set, wrong);
    ASSERT_EQ(wrong, (size_t)0);
    ASSERT_TRUE(n.size() == 1 && (size_t)n[0] == set && set > 300 && set < got.size() - 300);
    // the float4 form of the same cloud, and without the count
    std::vector<float> cloud4;
    for (size_t i = 0; i < expected.size(); ++i) cloud4.insert(cloud4.end(), {cloud[3 * i], cloud[3 * i + 1], cloud[3 * i + 2], 1.f});
    dfa::DeviceArray<float> dc4;
    dc4.upload(cloud4);
    dfa::DeviceArray<unsigned char> flags4;
    cuda::visibleVertices(dc4.ptr(), 4, expected.size(), points, intr, 0.01f, flags4);
    std::vector<unsigned char> got4;
    flags4.download(got4);
    ASSERT_TRUE(same(got4, expected));
}

TEST(VisibleTermTest, FramesOfTheSphereAreTheSameWithTheSwitchOn) {
    cuda::Depth d[3];
    d[0].upload(sphere_depth(1.5f), W), d[1].upload(sphere_depth(1.49f), W), d[2].upload(sphere_depth(1.48f), W);
    DynFusion off(small_params(true, true, false)), on(small_params(true, true, true));
    for (int f = 0; f < 3; ++f) {
        const FrameOutputs a = outputs(off, off(d[f]));
        const FrameOutputs b = outputs(on, on(d[f]));
        ASSERT_TRUE(a.flag == (f > 0));
        ASSERT_TRUE(off.northStarVisibleVertices() == -1);
        if (f == 0) {
            ASSERT_TRUE(on.northStarVisibleVertices() == -1);
            ASSERT_TRUE(same(a, b));
            continue;
        }
        const long long cloud = (long long)on.getCanonicalWarpedToLive()->size(), seen = on.northStarVisibleVertices();
        std::printf("frame %d: %lld of %lld canonical vertices visible (%.4f), valid rows %lld (off: %lld), cost %.9g -> %.9g (off: %.9g -> %.9g)\n",
                    f, seen, cloud, (double)seen / (double)cloud, b.valid, a.valid, b.cost0, b.cost1, a.cost0, a.cost1);
        ASSERT_TRUE(seen >= 0 && seen <= cloud);
        ASSERT_TRUE(100 * seen >= 99 * cloud);  // the front surface is the whole model
        ASSERT_TRUE(same(a, b));                // node transforms, costs, warped cloud: bit for bit
        ASSERT_TRUE(!on.getWarpedModelMaps().points.empty());  // the frame's own rasterisation left its maps
    }
}

// the count of a frame is the rule applied to what the device had: the model map the frame rasterised, and the canonical
// cloud under the transforms the solve started from (made again by hand: frame 1 starts from frame 0's identity transforms)
TEST(VisibleTermTest, CountIsTheRuleOnTheDumpedModelMap) {
    cuda::Depth d0, d1;
    d0.upload(sphere_depth(1.5f), W), d1.upload(sphere_depth(1.49f), W);
    DynFusion df(small_params(true, true, true));
    ASSERT_TRUE(df(d0) == false);
    // the transforms frame 1's solve starts from are the nodes' now; the cloud warped by them, on a plan of the test's own
    std::vector<float> pos, w, dq;
    df.getWarpfield()->hostArrays(pos, w, dq);
    const auto canonical = df.getCanonicalWarpedToLive();  // (frame 0: a copy of the canonical frame)
    const size_t n = canonical->size();
    dfa::DeviceArray<float> dpos, dw, ddq, start(3 * n);
    dpos.upload(pos), dw.upload(w), ddq.upload(dq);
    {
        const dynfu::Frame::DeviceView c = canonical->device();
        dfa_solver6* plan = nullptr;
        dfa::check(dfa_solver6_create((int)w.size(), (int)n, std::min(df.getWarpfield()->getKnn(), 8), &plan), "dfa_solver6_create");
        dfa::check(dfa_solver6_set_problem(plan, dpos.ptr(), ddq.ptr(), dw.ptr(), (int)w.size(), c.vertices, c.normals, (int)n, nullptr), "set_problem");
        dfa::check(dfa_solver6_warp_with(plan, ddq.ptr(), start.ptr(), nullptr, nullptr), "dfa_solver6_warp_with");
        std::vector<float> wait;
        start.download(wait);  // (synchronises before the plan goes)
        dfa_solver6_destroy(plan);
    }
    ASSERT_TRUE(df(d1) == true);
    const long long seen = df.northStarVisibleVertices();
    std::vector<Point> map;
    int cols = 0;
    df.getWarpedModelMaps().points.download(map, cols);
    ASSERT_TRUE(cols == W && map.size() == (size_t)W * H);
    std::vector<float> cloud;
    start.download(cloud);
    const Vec3f vs = df.tsdf().getVoxelSize();
    const float z_tol = 2.f * std::max(vs[0], std::max(vs[1], vs[2]));
    long long by_rule = 0, off_image = 0, hidden = 0;
    for (size_t i = 0; i < n; ++i) {
        const unsigned char f = visible_by_rule(&cloud[3 * i], map, W, H, df.KinFu::params().intr, z_tol);
        by_rule += f;
        if (!f) {
            const float u = F * cloud[3 * i] / cloud[3 * i + 2] + (W / 2 - 0.5f), v = F * cloud[3 * i + 1] / cloud[3 * i + 2] + (H / 2 - 0.5f);
            (u < -0.5f || v < -0.5f || u > W - 0.5f || v > H - 0.5f ? off_image : hidden)++;
        }
    }
    std::printf("frame 1: %lld visible on the device, %lld by the rule on the dumped map, of %zu (%lld hidden, %lld outside the image); z_tol %.6f\n",
                seen, by_rule, n, hidden, off_image, z_tol);
    ASSERT_EQ(seen, by_rule);
    ASSERT_TRUE(100 * seen >= 99 * (long long)n);
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
