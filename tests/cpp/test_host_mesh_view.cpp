// test_host_mesh_view.cpp — kfusion::cuda::rasterizeMesh (kfusion/cuda/mesh_render.hpp) and DynFusion's view of the warped
// canonical model (DynFuParams::model_view, renderWarpedModel, getWarpedModelMaps, getCanonicalMesh) on the synthetic sphere
// alone: the wrapper against the C call, image sizes per flag, the view against the manual sequence
// warpToLive (north-star mode: dfa_solver6_warp_with, and the warped mesh against the warped cloud) -> dfa_mesh_rasterize ->
// dfa_render_image_points / dfa_render_tangent_colors byte for byte in both solve modes, the throws, and that
// switching the view on changes nothing else a frame produces.  (dfa_mesh_rasterize itself is checked against the numpy
// statement by tests/test_gpu_raster.py.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <dynfu/dyn_fusion.hpp>
#include <kfusion/cuda/mesh_render.hpp>

#include "../../include/dynfu_amd.h"
#include "dynfu_fixtures.hpp"
#include "minitest.hpp"

using namespace kfusion;
using namespace dynfu_fixtures::sphere_scene;

namespace {
DynFuParams small_params(bool model_view, bool north_star) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(64);
    p.kinfuParams.light_pose = Vec3f(0.2f, 0.1f, 0.f);
    p.epsilon = 0.05f;
    p.mesh_normals = true;
    p.model_view = model_view, p.north_star = north_star;
    return p;
}

void tune(DynFusion& df) { df.solverParams.numIter = 2, df.solverParams.nonLinearIter = 2, df.solverParams.linearIter = 64; }

template <class T>
std::vector<T> pixels(const dfa::DeviceArray2D<T>& image) {
    std::vector<T> h;
    int cols = 0;
    if (!image.empty()) image.download(h, cols);
    return h;
}
template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}
std::vector<RGB> columns(const std::vector<RGB>& img, int wide, int x0, int cols) {
    std::vector<RGB> out;
    for (size_t y = 0; y < img.size() / wide; ++y) out.insert(out.end(), img.begin() + y * wide + x0, img.begin() + y * wide + x0 + cols);
    return out;
}
// pixels of the surface are grey, those of the background ramp are not
void count(const std::vector<RGB>& img, size_t& grey, size_t& ramp) {
    grey = ramp = 0;
    for (const RGB& p : img) (p.b == p.g && p.g == p.r ? grey : ramp)++;
}
bool throws(DynFusion& df) {
    try {
        cuda::Image none;
        df.renderWarpedModel(none, 0);
    } catch (const dfa::Error&) {
        return true;
    }
    return false;
}

// everything of a frame the view must not change
struct FrameOutputs {
    bool flag;
    std::vector<dfa::PointXYZ> warped, live;
    std::vector<dfa::Normal> warped_n, live_n;
    std::vector<float> pos, w, dq;
};
FrameOutputs outputs(DynFusion& df, bool flag) {
    FrameOutputs o;
    o.flag = flag;
    o.warped = df.getCanonicalWarpedToLive()->vertices().points, o.warped_n = df.getCanonicalWarpedToLive()->normals().points;
    if (df.getLiveFrame()) o.live = df.getLiveFrame()->vertices().points, o.live_n = df.getLiveFrame()->normals().points;
    df.getWarpfield()->hostArrays(o.pos, o.w, o.dq);
    return o;
}
template <class T>
bool same_or_both_empty(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
bool same(const FrameOutputs& a, const FrameOutputs& b) {
    return a.flag == b.flag && same(a.warped, b.warped) && same(a.warped_n, b.warped_n) && same_or_both_empty(a.live, b.live) &&
           same_or_both_empty(a.live_n, b.live_n) && same(a.pos, b.pos) && same(a.w, b.w) && same(a.dq, b.dq);
}
}  // namespace

TEST(MeshViewTest, RasterizeMeshEqualsTheCCall) {
    // two triangles that cross in front of the camera, and one behind it that is skipped
    const std::vector<dfa::PointXYZ> v = {{-0.6f, -0.5f, 1.0f}, {0.7f, -0.1f, 2.0f}, {-0.4f, 0.6f, 1.2f},
                                          {-0.6f, -0.3f, 2.0f}, {0.6f, -0.5f, 1.0f}, {0.5f, 0.7f, 1.4f},
                                          {0.f, 0.f, -1.f}};
    std::vector<dfa::Normal> n;
    for (int i = 0; i < 7; ++i) n.push_back(dfa::Normal(0.1f * i, 0.3f, -1.f));
    const std::vector<int> idx = {0, 1, 2, 3, 4, 5, 0, 1, 6};
    dfa::DeviceArray<dfa::PointXYZ> dv;
    dfa::DeviceArray<dfa::Normal> dn, none;
    dfa::DeviceArray<int> di;
    dv.upload(v), dn.upload(n), di.upload(idx);
    Affine3f pose;
    pose.t[0] = 0.05f, pose.t[2] = 0.1f;
    const Intr intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    for (const dfa::DeviceArray<dfa::Normal>* normals : {&dn, &none}) {
        cuda::Cloud points, direct_p(H, W);
        cuda::Normals normals_out, direct_n(H, W);
        dfa::DeviceArray<uint64_t> zb, direct_z((size_t)W * H);
        cuda::rasterizeMesh(dv, *normals, di, pose, intr, W, H, 0.1f, points, normals_out, zb);
        ASSERT_TRUE(points.rows() == H && points.cols() == W && normals_out.rows() == H && normals_out.cols() == W);
        ASSERT_EQ(zb.size(), (size_t)W * H);
        float aff[12];
        pose.to12(aff);
        dfa::check(dfa_mesh_rasterize((const float*)dv.ptr(), normals->empty() ? nullptr : (const float*)normals->ptr(), 7, di.ptr(), 3,
                                      aff, intr.fx, intr.fy, intr.cx, intr.cy, 0.1f, W, H, direct_z.ptr(), (float*)direct_p.ptr(),
                                      (int)direct_p.step(), (float*)direct_n.ptr(), (int)direct_n.step(), nullptr),
                   "dfa_mesh_rasterize");
        std::vector<uint64_t> z0, z1;
        zb.download(z0), direct_z.download(z1);
        ASSERT_TRUE(same(z0, z1));
        ASSERT_TRUE(same(pixels(points), pixels(direct_p)));
        ASSERT_TRUE(same(pixels(normals_out), pixels(direct_n)));
        size_t hit[3] = {0, 0, 0}, miss = 0;
        for (uint64_t k : z0) k == ~0ull ? ++miss : ++hit[(size_t)(k & 0xffffffffu)];
        ASSERT_TRUE(hit[0] > 100 && hit[1] > 100 && hit[2] == 0 && miss > 1000);
        // the outputs are kept when they already have the right size
        const Point* before = points.ptr();
        cuda::rasterizeMesh(dv, *normals, di, pose, intr, W, H, 0.1f, points, normals_out, zb);
        ASSERT_TRUE(points.ptr() == before);
    }
}

TEST(MeshViewTest, ThrowsWithoutModelViewAndBeforeTheFirstFrame) {
    cuda::Depth d0;
    d0.upload(sphere_depth(1.5f), W);
    DynFusion off(small_params(false, false));
    ASSERT_TRUE(throws(off));
    off(d0);
    ASSERT_TRUE(throws(off));
    ASSERT_TRUE(off.getCanonicalMesh().vertices.empty() && off.getWarpedModelMaps().points.empty());
    DynFusion on(small_params(true, false));
    ASSERT_TRUE(throws(on));  // before frame 0
    on(d0);
    ASSERT_TRUE(!throws(on));
}

namespace {
// the warp of the mode, made by hand: Warpfield::warpToLive in reference mode; in north-star mode the blend of the north-star
// solve, on a plan of the test's own over the warp field's nodes (the first `nodes` of them, if given) and the mesh
std::shared_ptr<dynfu::Frame> warp_by_hand(DynFusion& df, bool north_star, std::shared_ptr<dynfu::Frame> canonical, size_t nodes = 0) {
    if (!north_star) return df.getWarpfield()->warpToLive(canonical);
    std::vector<float> pos, w, dq;
    df.getWarpfield()->hostArrays(pos, w, dq);
    if (nodes) pos.resize(3 * nodes), w.resize(nodes), dq.resize(8 * nodes);
    dfa::DeviceArray<float> dpos, dw, ddq;
    dpos.upload(pos), dw.upload(w), ddq.upload(dq);
    const size_t n = canonical->size();
    const dynfu::Frame::DeviceView c = canonical->device();
    dfa_solver6* plan = nullptr;
    dfa::check(dfa_solver6_create((int)w.size(), (int)n, std::min(df.getWarpfield()->getKnn(), 8), &plan), "dfa_solver6_create");
    dfa::DeviceArray<float> ov(3 * n), on(3 * n);
    dfa::check(dfa_solver6_set_problem(plan, dpos.ptr(), ddq.ptr(), dw.ptr(), (int)w.size(), c.vertices, c.normals, (int)n, nullptr), "set_problem");
    dfa::check(dfa_solver6_warp_with(plan, ddq.ptr(), ov.ptr(), on.ptr(), nullptr), "dfa_solver6_warp_with");
    auto out = dynfu::Frame::fromDevice(0, ov, on, n);
    (void)out->vertices();  // (downloads: synchronises before the plan goes)
    dfa_solver6_destroy(plan);
    return out;
}
double dist(const dfa::PointXYZ& a, const dfa::PointXYZ& b) {
    return std::sqrt((double)(a.x - b.x) * (a.x - b.x) + (double)(a.y - b.y) * (a.y - b.y) + (double)(a.z - b.z) * (a.z - b.z));
}
}  // namespace

TEST(MeshViewTest, ViewOfTheWarpedModelIsWarpRasteriseShade) {
    cuda::Depth d0, d1;
    d0.upload(sphere_depth(1.5f), W), d1.upload(sphere_depth(1.49f), W);
    for (const bool north_star : {false, true}) {
        DynFusion df(small_params(true, north_star));
        tune(df);
        ASSERT_TRUE(df(d0) == false);
        const KinFuParams& kp = df.KinFu::params();
        // the canonical mesh: welded (a fifth of the soup's vertices)
        const auto mesh = df.getCanonicalMesh();
        const size_t n = mesh.vertices.size();
        std::printf("%s: canonical mesh: %zu vertices, %zu indices\n", north_star ? "north-star mode" : "reference mode", n, mesh.indices.size());
        ASSERT_TRUE(n > 100 && mesh.indices.size() % 3 == 0 && mesh.indices.size() > 3 * n);  // (two triangles per vertex, less the rim)
        ASSERT_EQ(mesh.indices.size(), df.getCanonicalWarpedToLive()->size());  // one index per vertex of run()'s soup, in its order
        std::vector<int> index;
        mesh.indices.download(index);
        // the same mesh extracted by hand — the volume still is frame 0's — with its normals, in the frame of the canonical cloud
        dfa::DeviceArray<cuda::MarchingCubes::PointType> vb;
        dfa::DeviceArray<int> ib;
        const auto own = df.mc().runIndexed(df.tsdf(), vb, ib);
        ASSERT_EQ(own.vertices.size(), n);
        dfa::DeviceArray<dfa::Normal> normals4;
        df.mc().computeNormals(df.tsdf(), own.vertices, normals4);
        dfa::DeviceArray<float> v3(3 * n), n3(3 * n);
        dfa::check(dfa_repack_points((const float*)own.vertices.ptr(), 4, v3.ptr(), 3, (int)n, 0.f, nullptr), "repack");
        dfa::check(dfa_repack_points((const float*)normals4.ptr(), 4, n3.ptr(), 3, (int)n, 0.f, nullptr), "repack");
        if (north_star) {  // the camera is at the origin: volume frame -> camera frame is the volume's pose
            float to_camera[12];
            (Affine3f().inv() * df.tsdf().getPose()).to12(to_camera);
            dfa::check(dfa_transform_points(v3.ptr(), (int)n, to_camera, 1, v3.ptr(), nullptr), "transform");
            dfa::check(dfa_transform_points(n3.ptr(), (int)n, to_camera, 0, n3.ptr(), nullptr), "transform");
        }
        const auto canonical = dynfu::Frame::fromDevice(0, v3, n3, n);

        for (int frame = 0; frame < 2; ++frame) {
            const size_t nodes_before = df.getWarpfield()->getNodes().size();  // the nodes this frame's solve moves
            if (frame == 1) ASSERT_TRUE(df(d1) == true);
            cuda::Image i0, i1, i2, i3, i7;
            df.renderWarpedModel(i0), df.renderWarpedModel(i1, 1), df.renderWarpedModel(i2, 2), df.renderWarpedModel(i3, 3);
            df.renderWarpedModel(i7, 7);
            ASSERT_TRUE(i0.rows() == H && i0.cols() == W && i1.cols() == W && i2.cols() == W && i7.cols() == W);
            ASSERT_TRUE(i3.rows() == H && i3.cols() == 2 * W);
            const std::vector<RGB> p0 = pixels(i0), p2 = pixels(i2), p3 = pixels(i3);
            ASSERT_TRUE(same(pixels(i1), p0) && same(pixels(i7), p0));
            ASSERT_TRUE(same(columns(p3, 2 * W, 0, W), p0) && same(columns(p3, 2 * W, W, W), p2));
            // the manual sequence
            const auto warped = warp_by_hand(df, north_star, canonical);
            const dynfu::Frame::DeviceView w = warped->device();
            ASSERT_EQ(w.n, n);
            ASSERT_TRUE(same(warped->vertices().points, df.warpCanonicalMesh()->vertices().points));
            ASSERT_TRUE(same(warped->normals().points, df.warpCanonicalMesh()->normals().points));
            if (north_star) {
                // The mesh moves with the cloud the solve fitted.  Index j names the mesh vertex at soup vertex j, and
                // getCanonicalWarpedToLive() is that soup under the solved transforms of the nodes the solve had — the
                // nodes Warpfield::update added afterwards come last and are left out here.  The same function of position
                // at the same position: the two agree to rounding, asserted as a median below a millimetre (the frames
                // are 10 mm apart; the reference's blend of the same transforms is centimetres away).
                const auto with_solved_nodes = warp_by_hand(df, true, canonical, nodes_before);
                const std::vector<dfa::PointXYZ>& cloud = df.getCanonicalWarpedToLive()->vertices().points;
                const std::vector<dfa::PointXYZ>& moved = with_solved_nodes->vertices().points;
                std::vector<double> d;
                for (size_t j = 0; j < index.size(); ++j) d.push_back(dist(moved[(size_t)index[j]], cloud[j]));
                std::sort(d.begin(), d.end());
                std::printf("frame %d: %zu nodes in the solve, %zu after it; warped mesh against the warped cloud: median %.3g m, max %.3g m\n",
                            frame, nodes_before, df.getWarpfield()->getNodes().size(), d[d.size() / 2], d.back());
                ASSERT_TRUE(d[d.size() / 2] < 1e-3);
            }
            dfa::DeviceArray<float> wv(4 * n), wn(4 * n);
            dfa::check(dfa_repack_points(w.vertices, 3, wv.ptr(), 4, (int)n, 1.f, nullptr), "repack");
            dfa::check(dfa_repack_points(w.normals, 3, wn.ptr(), 4, (int)n, 0.f, nullptr), "repack");
            cuda::Cloud points(H, W);
            cuda::Normals normals(H, W);
            dfa::DeviceArray<uint64_t> zb((size_t)W * H);
            float aff[12];
            // reference mode: the mesh is in the volume's frame; north-star mode: in the camera's
            (north_star ? Affine3f() : df.getCameraPose().inv() * df.tsdf().getPose()).to12(aff);
            dfa::check(dfa_mesh_rasterize(wv.ptr(), wn.ptr(), (int)n, mesh.indices.ptr(), (int)(mesh.indices.size() / 3), aff, kp.intr.fx,
                                          kp.intr.fy, kp.intr.cx, kp.intr.cy, df.params().model_view_z_near, W, H, zb.ptr(),
                                          (float*)points.ptr(), (int)points.step(), (float*)normals.ptr(), (int)normals.step(), nullptr),
                       "dfa_mesh_rasterize");
            cuda::Image phong(H, W), colours(H, W);
            dfa::check(dfa_render_image_points((const float*)points.ptr(), (int)points.step(), (const float*)normals.ptr(),
                                               (int)normals.step(), W, H, kp.light_pose.v, (uint8_t*)phong.ptr(), (int)phong.step(), nullptr),
                       "dfa_render_image_points");
            dfa::check(dfa_render_tangent_colors((const float*)normals.ptr(), (int)normals.step(), W, H, (uint8_t*)colours.ptr(),
                                                 (int)colours.step(), nullptr),
                       "dfa_render_tangent_colors");
            ASSERT_TRUE(same(pixels(phong), p0));
            ASSERT_TRUE(same(pixels(colours), p2));
            const auto maps = df.getWarpedModelMaps();
            ASSERT_TRUE(same(pixels(maps.points), pixels(points)) && same(pixels(maps.normals), pixels(normals)));
            // both sides of the hit / miss branch: the sphere, and the background around it
            size_t grey, ramp;
            count(p0, grey, ramp);
            std::printf("frame %d: %zu surface pixels, %zu background pixels\n", frame, grey, ramp);
            ASSERT_TRUE(grey > (size_t)W * H / 10 && ramp > (size_t)W * H / 10);
        }
    }
}

TEST(MeshViewTest, FrameOutputsDoNotDependOnTheView) {
    cuda::Depth d[3];
    d[0].upload(sphere_depth(1.5f), W), d[1].upload(sphere_depth(1.49f), W), d[2].upload(sphere_depth(1.48f), W);
    // two runs are compared bit for bit: the reference-mode solve assembles with float atomics unless asked for its
    // order-stable form (read once per solver plan); the north-star solve has no such freedom
    ::setenv("DFA_ASSEMBLE_DETERMINISTIC", "1", 1);
    for (const bool north_star : {false, true}) {
        DynFusion off(small_params(false, north_star)), on(small_params(true, north_star));
        tune(off), tune(on);
        for (int f = 0; f < 3; ++f) {
            const FrameOutputs a = outputs(off, off(d[f]));
            const FrameOutputs b = outputs(on, on(d[f]));
            ASSERT_TRUE(a.flag == (f > 0));
            ASSERT_TRUE(same(a, b));
            cuda::Image image;
            on.renderWarpedModel(image, 3);  // between the frames: the next one must not notice
            ASSERT_TRUE(image.cols() == 2 * W && image.rows() == H);
            size_t grey, ramp;
            count(columns(pixels(image), 2 * W, 0, W), grey, ramp);
            std::printf("%s, frame %d: %zu surface pixels, %zu background pixels\n", north_star ? "north-star mode" : "reference mode", f, grey, ramp);
            ASSERT_TRUE(grey > (size_t)W * H / 10 && ramp > (size_t)W * H / 10);
            if (north_star) {  // the mesh is kept in the camera frame, as the canonical cloud is: in front of the camera
                std::vector<dfa::PointXYZ> v;
                on.getCanonicalMesh().vertices.download(v);
                double z = 0;
                for (const auto& p : v) z += p.z;
                ASSERT_TRUE(z / (double)v.size() > 1.0 && z / (double)v.size() < 1.6);
            }
        }
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
