// test_host_render.cpp — KinFu::renderImage (reference: include/kfusion/kinfu.hpp, src/kfusion/kinfu.cpp:264-316) and
// the cuda::renderImage / renderTangentColors adaptors (include/kfusion/cuda/imgproc.hpp:26-33) on the synthetic sphere
// in front of a wall: image sizes per flag, the flag == 1 rule, equality with the C entry points on the same maps (those
// are checked against the numpy statement by tests/test_gpu_render.py), the fused view from a pose against raycast +
// render, DynFusion's inherited overloads, and a PNG of the view.
// With DFA_RENDER_PNG=<path> in the environment the PNG test keeps its file there and writes the image's bytes
// (b, g, r, 0 per pixel, dense) to <path>.raw: tests/test_host_render.py inflates the one and compares it with the other.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <string>

#include <unistd.h>

#include <dynfu/dyn_fusion.hpp>
#include <kfusion/kinfu.hpp>

#include "../../include/dynfu_amd.h"
#include "minitest.hpp"

using namespace kfusion;

namespace {
// a sphere of radius 0.5 m at `cz` metres in front of a wall at 2.5 m (test_host_dynfusion.cpp), 3 invalid border pixels
std::vector<unsigned short> sphere_depth(int W, int H, float f, float cz) {
    std::vector<unsigned short> d((size_t)W * H);
    const float cx = W / 2 - 0.5f, cy = H / 2 - 0.5f, R = 0.5f;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float dir[3] = {(x - cx) / f, (y - cy) / f, 1.f};
            const float n = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + 1.f);
            for (float& v : dir) v /= n;
            const float b = dir[2] * cz, disc = b * b - (cz * cz - R * R);
            float z = 2.5f;
            if (disc > 0) z = (b - std::sqrt(disc)) * dir[2];
            d[(size_t)y * W + x] = (x < 3 || y < 3 || x >= W - 3 || y >= H - 3) ? 0 : (unsigned short)std::lround(z * 1000.f);
        }
    return d;
}

struct Probe : KinFu {  // the model maps renderImage(image, flag) reads
    using KinFu::KinFu;
    const cuda::Cloud& points() const { return prev_.points_pyr[0]; }
    const cuda::Normals& normals() const { return prev_.normals_pyr[0]; }
};

KinFuParams vga_params() {
    KinFuParams p = KinFuParams::default_params();  // 640 x 480, f = 525
    p.volume_dims = Vec3i::all(256);
    return p;
}

// three frames of the static scene: the model maps are the raycast of the volume from the tracked pose
void feed(KinFu& k, int frames = 3) {
    cuda::Depth depth;
    depth.upload(sphere_depth(k.params().cols, k.params().rows, k.params().intr.fx, 1.5f), k.params().cols);
    for (int i = 0; i < frames; ++i) k(depth);
}

std::vector<RGB> pixels(const cuda::Image& image) {
    std::vector<RGB> h;
    int cols = 0;
    image.download(h, cols);
    return h;
}
bool same(const std::vector<RGB>& a, const std::vector<RGB>& b) {
    return a.size() == b.size() && !a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(RGB)) == 0;
}
// columns [x0, x0 + cols) of an image `wide` pixels wide
std::vector<RGB> columns(const std::vector<RGB>& img, int wide, int x0, int cols) {
    std::vector<RGB> out;
    for (size_t y = 0; y < img.size() / wide; ++y) out.insert(out.end(), img.begin() + y * wide + x0, img.begin() + y * wide + x0 + cols);
    return out;
}
// pixels of the surface are grey, those of the background ramp are not (b > g everywhere on it)
void count(const std::vector<RGB>& img, size_t& grey, size_t& ramp) {
    grey = ramp = 0;
    for (const RGB& p : img) (p.b == p.g && p.g == p.r ? grey : ramp)++;
}
}  // namespace

TEST(RenderTest, DefaultLightPoseIsTheCamera) {
    const KinFuParams p = KinFuParams::default_params();  // kinfu.cpp:41
    ASSERT_TRUE(p.light_pose[0] == 0.f && p.light_pose[1] == 0.f && p.light_pose[2] == 0.f);
    ASSERT_EQ(sizeof(RGB), (size_t)4);
}

TEST(RenderTest, RenderImageOfTheModelMapsPerFlag) {
    Probe k(vga_params());
    cuda::Image none;
    bool threw = false;
    try {
        k.renderImage(none, 0);  // before the first frame: no maps
    } catch (const dfa::Error&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
    feed(k);
    const int W = k.params().cols, H = k.params().rows;
    k.params().light_pose = Vec3f(0.4f, -0.3f, 0.2f);
    cuda::Image i0, i1, i2, i3, i7;
    k.renderImage(i0, 0), k.renderImage(i1, 1), k.renderImage(i2, 2), k.renderImage(i3, 3), k.renderImage(i7, 7);
    ASSERT_TRUE(i0.rows() == H && i0.cols() == W && i1.cols() == W && i2.cols() == W && i7.cols() == W);
    ASSERT_TRUE(i3.rows() == H && i3.cols() == 2 * W);  // kinfu.cpp:266
    const std::vector<RGB> p0 = pixels(i0), p2 = pixels(i2), p3 = pixels(i3);
    ASSERT_TRUE(same(pixels(i1), p0));  // flag == 1 is the Phong view (the deviation stated in kfusion/kinfu.hpp)
    ASSERT_TRUE(same(pixels(i7), p0));  // any flag outside 1 ... 3
    ASSERT_TRUE(same(columns(p3, 2 * W, 0, W), p0));
    ASSERT_TRUE(same(columns(p3, 2 * W, W, W), p2));
    // the C entry points on the same maps
    cuda::Image d0(H, W), d2(H, W);
    dfa::check(dfa_render_image_points((const float*)k.points().ptr(), (int)k.points().step(), (const float*)k.normals().ptr(),
                                       (int)k.normals().step(), W, H, k.params().light_pose.v, (uint8_t*)d0.ptr(), (int)d0.step(),
                                       nullptr),
               "dfa_render_image_points");
    dfa::check(dfa_render_tangent_colors((const float*)k.normals().ptr(), (int)k.normals().step(), W, H, (uint8_t*)d2.ptr(),
                                         (int)d2.step(), nullptr),
               "dfa_render_tangent_colors");
    ASSERT_TRUE(same(pixels(d0), p0));
    ASSERT_TRUE(same(pixels(d2), p2));
    // the view has both surface and background (the 3 invalid border pixels of the frame, and what the volume does not hold)
    size_t grey, ramp;
    count(p0, grey, ramp);
    ASSERT_TRUE(grey > p0.size() / 10 && ramp > 1000);
    // the light matters
    cuda::Image lit;
    k.params().light_pose = Vec3f::all(0.f);
    k.renderImage(lit, 0);
    ASSERT_TRUE(!same(pixels(lit), p0));
}

TEST(RenderTest, RenderImageFromAPoseIsRaycastThenRender) {
    Probe k(vga_params());
    feed(k);
    const KinFuParams& p = k.params();
    k.params().light_pose = Vec3f(0.4f, -0.3f, 0.2f);
    Affine3f moved = k.getCameraPose();
    const float a = 0.3f;
    const float R[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)};
    for (int i = 0; i < 9; ++i) moved.R[i] = R[i];
    moved.t[0] += 0.05f, moved.t[1] -= 0.02f;
    int at = 0;
    for (const Affine3f& pose : {k.getCameraPose(), moved}) {
        cuda::Cloud points(p.rows, p.cols);
        cuda::Normals normals(p.rows, p.cols);
        k.tsdf().raycast(pose, p.intr, points, normals);
        cuda::Image phong, colours;
        cuda::renderImage(points, normals, p.intr, p.light_pose, phong);
        cuda::renderTangentColors(normals, colours);
        cuda::Image f0, f2, f3;
        k.renderImage(f0, pose, 0), k.renderImage(f2, pose, 2), k.renderImage(f3, pose, 3);
        ASSERT_TRUE(f0.cols() == p.cols && f2.cols() == p.cols && f3.cols() == 2 * p.cols && f3.rows() == p.rows);
        ASSERT_TRUE(same(pixels(f0), pixels(phong)));
        ASSERT_TRUE(same(pixels(f2), pixels(colours)));
        const std::vector<RGB> p3 = pixels(f3);
        ASSERT_TRUE(same(columns(p3, 2 * p.cols, 0, p.cols), pixels(phong)));
        ASSERT_TRUE(same(columns(p3, 2 * p.cols, p.cols, p.cols), pixels(colours)));
        cuda::Image f1;
        k.renderImage(f1, pose, 1);
        ASSERT_TRUE(same(pixels(f1), pixels(phong)));
        size_t grey, ramp;
        count(pixels(f0), grey, ramp);
        ASSERT_TRUE(grey > (size_t)p.rows * p.cols / 10 && ramp > (at == 0 ? (size_t)1000 : (size_t)p.rows * p.cols / 10));
        if (at++ == 0) {  // at the tracked pose the model maps ARE this raycast (kinfu.cpp:222)
            cuda::Image model;
            k.renderImage(model, 0);
            ASSERT_TRUE(same(pixels(model), pixels(f0)));
        }
    }
}

TEST(RenderTest, RenderImageOfADepthMap) {
    Probe k(vga_params());
    feed(k);
    const KinFuParams& p = k.params();
    cuda::Depth depth(p.rows, p.cols);
    cuda::Normals normals(p.rows, p.cols);
    k.tsdf().raycast(k.getCameraPose(), p.intr, depth, normals);
    cuda::Image image, direct(p.rows, p.cols);
    const Vec3f light(0.4f, -0.3f, 0.2f);
    cuda::renderImage(depth, normals, p.intr, light, image);
    ASSERT_TRUE(image.rows() == p.rows && image.cols() == p.cols);
    dfa::check(dfa_render_image_depth(depth.ptr(), (int)depth.step(), (const float*)normals.ptr(), (int)normals.step(), p.cols,
                                      p.rows, p.intr.fx, p.intr.fy, p.intr.cx, p.intr.cy, light.v, (uint8_t*)direct.ptr(),
                                      (int)direct.step(), nullptr),
               "dfa_render_image_depth");
    ASSERT_TRUE(same(pixels(image), pixels(direct)));
    // millimetre depths instead of float points: close to the view of the point map, not equal to it
    cuda::Image of_points;
    k.params().light_pose = light;
    k.renderImage(of_points, 0);
    const std::vector<RGB> a = pixels(image), b = pixels(of_points);
    size_t far = 0;
    for (size_t i = 0; i < a.size(); ++i) far += std::abs((int)a[i].g - (int)b[i].g) > 2;
    ASSERT_TRUE(far < a.size() / 100);
}

TEST(RenderTest, DynFusionInheritsTheViews) {
    const int W = 160, H = 120;
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(131.25f, 131.25f, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(64);
    p.kinfuParams.light_pose = Vec3f(0.2f, 0.1f, 0.f);
    p.epsilon = 0.05f;
    DynFusion df(p);
    df.solverParams.numIter = 2, df.solverParams.nonLinearIter = 2, df.solverParams.linearIter = 64;
    cuda::Depth d0, d1;
    d0.upload(sphere_depth(W, H, 131.25f, 1.5f), W);
    d1.upload(sphere_depth(W, H, 131.25f, 1.49f), W);
    df(d0), df(d1);
    const KinFuParams& kp = df.KinFu::params();
    const Affine3f pose = df.getCameraPose();
    cuda::Cloud points(H, W);
    cuda::Normals normals(H, W);
    df.tsdf().raycast(pose, kp.intr, points, normals);
    cuda::Image phong, colours, f0, f2, f3;
    cuda::renderImage(points, normals, kp.intr, kp.light_pose, phong);
    cuda::renderTangentColors(normals, colours);
    df.renderImage(f0, pose), df.renderImage(f2, pose, 2), df.renderImage(f3, pose, 3);
    ASSERT_TRUE(same(pixels(f0), pixels(phong)));
    ASSERT_TRUE(same(pixels(f2), pixels(colours)));
    ASSERT_TRUE(f3.cols() == 2 * W && same(columns(pixels(f3), 2 * W, W, W), pixels(colours)));
    size_t grey, ramp;
    count(pixels(f0), grey, ramp);
    ASSERT_TRUE(grey > (size_t)W * H / 10 && ramp > 100);
    // DynFusion::operator() skips the rigid tracker and keeps no model maps: the overload that reads them says so
    bool threw = false;
    try {
        cuda::Image none;
        df.renderImage(none, 0);
    } catch (const dfa::Error&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
}

TEST(RenderTest, WritesTheViewAsPng) {
    Probe k(vga_params());
    feed(k);
    cuda::Image image;
    k.renderImage(image, 0);
    ASSERT_TRUE(image.cols() == 640 && image.rows() == 480);
    const std::vector<RGB> px = pixels(image);
    const char* keep = std::getenv("DFA_RENDER_PNG");
    const std::string path = keep ? std::string(keep)
                                  : (std::filesystem::temp_directory_path() / ("dfa_render_" + std::to_string(::getpid()) + ".png")).string();
    dfa::io::writeImagePng(path, (const uint8_t*)px.data(), 640, 480);
    const std::vector<uint8_t> bytes = dfa::io::encodeImagePng((const uint8_t*)px.data(), 640, 480, 640 * 4);
    std::ifstream in(path, std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    ASSERT_TRUE(file == bytes && bytes.size() > 1000);
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    ASSERT_TRUE(std::memcmp(bytes.data(), sig, 8) == 0);
    ASSERT_TRUE(bytes[24] == 8 && bytes[25] == 2);  // IHDR: 8 bits, truecolour
    if (keep) {
        std::ofstream raw(path + ".raw", std::ios::binary);
        raw.write((const char*)px.data(), (std::streamsize)(px.size() * sizeof(RGB)));
    } else std::remove(path.c_str());
    // a grey lit surface on the ramp: near-black at the top, light blue at the bottom (the frame's invalid border rows)
    const RGB top = px[320], bottom = px[(size_t)479 * 640 + 320], centre = px[(size_t)240 * 640 + 320];
    ASSERT_TRUE(top.b == 4 && top.g == 2 && top.r == 2);
    ASSERT_TRUE(bottom.b == 235 && bottom.g == 119 && bottom.r == 119);
    ASSERT_TRUE(centre.b == centre.g && centre.g == centre.r && centre.g > 200);  // facing the camera and its light
    bool threw = false;
    try {
        dfa::io::encodeImagePng((const uint8_t*)px.data(), 640, 480, 100);
    } catch (const dfa::Error&) {
        threw = true;
    }
    ASSERT_TRUE(threw);
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
