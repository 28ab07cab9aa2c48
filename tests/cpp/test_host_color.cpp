// test_host_color.cpp — colour in the host adaptor: kfusion::cuda::TsdfVolume::integrateWarped6Color against the C call's bits
// (dfa_tsdf_integrate_warped6_color itself is checked against the numpy statement by tests/test_gpu_tsdf_color.py), the rules
// of DynFuParams::north_star_fuse_color, and a four-frame static north-star sequence before a colour ramp: with the switch on
// the canonical volume and the warped cloud are those of north_star_fuse_canonical alone, bit for bit, and
// DynFusion::canonicalColors() returns the ramp at every vertex's own projection.
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

namespace {

std::vector<uint32_t> words(const uint32_t* device, size_t n) {
    dfa::DeviceArray<uint32_t> view(const_cast<uint32_t*>(device), n);  // (non-owning)
    std::vector<uint32_t> h;
    view.download(h);
    return h;
}

// the ramp of the sequence test: b = 3 u / 4, g = v, r = 128 — monotone over the whole 320 x 240 image, no wrap
const float SLOPE_B = 0.75f, SLOPE_G = 1.f;
std::vector<RGB> ramp(int W, int H) {
    std::vector<RGB> px((size_t)W * H);
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            RGB& p = px[(size_t)v * W + u];
            p.bgra = 0;
            p.b = (unsigned char)(3 * u / 4), p.g = (unsigned char)v, p.r = 128;
        }
    return px;
}

}  // namespace

// ------------------------------------------------------------------------------------------ the adaptor against the C call
TEST(HostColorTest, IntegrateWarped6ColorMatchesTheCCall) {
    using namespace dynfu_fixtures::sphere_scene;
    const int DIM = 64, D = 81;
    const Intr intr{F, F, W / 2 - 0.5f, H / 2 - 0.5f};
    // test_host_tsdf_warped6.cpp's scene: the sphere at 1.5 m fused, the sphere at 1.48 m next, 9 x 9 nodes in a frame of their own
    Affine3f frame;
    frame.R[0] = std::cos(0.1f), frame.R[2] = std::sin(0.1f), frame.R[6] = -std::sin(0.1f), frame.R[8] = std::cos(0.1f);
    frame = frame.translate(Vec3f(0.05f, -0.03f, 0.1f));
    cuda::TsdfVolume vol{Vec3i::all(DIM)};
    vol.setTruncDist(0.1f), vol.setMaxWeight(64), vol.setSize(Vec3f::all(3.f));
    vol.setPose(Affine3f().translate(Vec3f(-1.5f, -1.5f, 0.5f)));
    cuda::Depth depth;
    cuda::Dists dists, next;
    depth.upload(sphere_depth(1.5f), W);
    cuda::computeDists(depth, dists, intr);
    vol.clearAndIntegrate(dists, Affine3f(), intr);
    depth.upload(sphere_depth(1.48f), W);
    cuda::computeDists(depth, next, intr);
    const Affine3f v2n = frame.inv() * vol.getPose();
    std::vector<float> hp, hq, hw;
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
            const float v[3] = {1.1f + 0.1f * i, 1.1f + 0.1f * j, 0.55f + 0.01f * ((i * 7 + j * 3) % 5)};
            for (int c = 0; c < 3; ++c) hp.push_back(v2n.R[3 * c] * v[0] + v2n.R[3 * c + 1] * v[1] + v2n.R[3 * c + 2] * v[2] + v2n.t[c]);
            hw.push_back(0.12f + 0.01f * ((i + j) % 4));
            const float a = 0.01f * (j - 4), cr = std::cos(0.5f * a), sr = std::sin(0.5f * a);
            const float t[3] = {0.004f * (i - 4), 0.003f * (j - 4), -0.02f};
            hq.insert(hq.end(), {cr, sr, 0.f, 0.f, 0.5f * (-t[0] * sr), 0.5f * (t[0] * cr), 0.5f * (t[1] * cr + t[2] * sr), 0.5f * (t[2] * cr - t[1] * sr)});
        }
    dfa::DeviceArray<float> pos, dq, w;
    pos.upload(hp), dq.upload(hq), w.upload(hw);
    std::vector<RGB> px((size_t)W * H);
    for (size_t i = 0; i < px.size(); ++i) px[i].bgra = (int)(i * 2654435761u);
    cuda::Image image;
    image.upload(px, W);

    const std::vector<uint32_t> before = voxels(static_cast<const cuda::TsdfVolume&>(vol));
    const size_t n = before.size();
    for (const bool update_tsdf : {true, false}) {
        for (const bool with_field : {false, true}) {
            cuda::TsdfVolume a{Vec3i::all(DIM)};
            a.setTruncDist(0.1f), a.setMaxWeight(64), a.setSize(Vec3f::all(3.f)), a.setPose(vol.getPose());
            a.copyVoxelsFrom(vol);
            a.createColors();
            ASSERT_TRUE(a.colors() != nullptr);
            if (with_field) ASSERT_TRUE(a.buildKnnField(pos.ptr(), w.ptr(), D, 8, &frame));
            a.integrateWarped6Color(next, image, Affine3f(), intr, frame, pos.ptr(), dq.ptr(), w.ptr(), D, 8,
                                    cuda::TsdfVolume::UnsupportedMode::Rigid, update_tsdf, 200);
            // the C call by hand on copies (searching: the field gives the same bits)
            dfa::DeviceArray<uint32_t> dvol(n), dcol(n);
            dvol.upload(before), dcol.upload(std::vector<uint32_t>(n, 0u));
            float vol2node[12], node2cam[12];
            (frame.inv() * vol.getPose()).to12(vol2node);
            (Affine3f().inv() * frame).to12(node2cam);
            const Vec3f vs = vol.getVoxelSize();
            dfa::check(dfa_tsdf_integrate_warped6_color(next.ptr(), (int)next.step(), W, H, (const uint8_t*)image.ptr(), (int)image.step(),
                                                        update_tsdf ? dvol.ptr() : nullptr, dcol.ptr(), DIM, DIM, DIM, nullptr, vs.v,
                                                        vol.getTruncDist(), vol.getMaxWeight(), 200, vol2node, node2cam, F, F, W / 2 - 0.5f,
                                                        H / 2 - 0.5f, pos.ptr(), dq.ptr(), w.ptr(), D, 8, DFA_WARPED_RIGID, nullptr, nullptr),
                       "dfa_tsdf_integrate_warped6_color");
            std::vector<uint32_t> want_vol, want_col;
            dvol.download(want_vol), dcol.download(want_col);
            const std::vector<uint32_t> got_col = words(a.colors(), n);
            size_t coloured = 0;
            for (uint32_t c : got_col) coloured += c != 0;
            std::printf("update_tsdf %d, field %d: %zu coloured voxels\n", (int)update_tsdf, (int)with_field, coloured);
            ASSERT_TRUE(coloured > 200);
            ASSERT_TRUE(same(got_col, want_col));
            ASSERT_TRUE(same(voxels(static_cast<const cuda::TsdfVolume&>(a)), want_vol));  // (colours only: `before`, untouched)
            if (!update_tsdf) ASSERT_TRUE(same(want_vol, before));
        }
    }
    // without createColors the call is refused
    bool threw = false;
    try {
        vol.integrateWarped6Color(next, image, Affine3f(), intr, frame, pos.ptr(), dq.ptr(), w.ptr(), D, 8);
    } catch (const dfa::Error& e) {
        threw = e.code == DFA_ERR_INVALID;
    }
    ASSERT_TRUE(threw);
}

// ------------------------------------------------------------------------------------------ the switch
namespace {
using namespace dynfu_fixtures::planted_motion_scene;
const int CDIM = 128;  // (the scene's cube at half the resolution of the rigid tests: 17 mm voxels)

DynFuParams color_params(bool fuse_canonical, bool fuse_color) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(CDIM);
    p.kinfuParams.volume_size = Vec3f::all(VOLUME);
    p.kinfuParams.volume_pose = Affine3f().translate(Vec3f(-VOLUME / 2, -VOLUME / 2, VOLUME_Z0));
    p.intr = p.kinfuParams.intr;
    p.epsilon = 0.05f;
    p.north_star = true, p.north_star_fuse_canonical = fuse_canonical, p.north_star_fuse_color = fuse_color;
    return p;
}
}  // namespace

TEST(HostColorTest, SwitchRules) {
    ASSERT_TRUE(construction_throws(color_params(false, true)));  // colour without the canonical fusion
    ASSERT_TRUE(!construction_throws(color_params(true, true)));
    ASSERT_TRUE(!construction_throws(color_params(true, false)));
    try {
        color_params(false, true).validate();
        ASSERT_TRUE(false);
    } catch (const dfa::Error& e) {
        ASSERT_TRUE(std::strstr(e.what(), "north_star_fuse_color") != nullptr);
    }
    for (int cap : {0, 256}) {
        DynFuParams p = color_params(true, true);
        p.canonical_max_color_weight = cap;
        ASSERT_TRUE(construction_throws(p));
    }
    ASSERT_EQ(DynFuParams::defaultParams().north_star_fuse_color, false);
    ASSERT_EQ(DynFuParams::defaultParams().canonical_max_color_weight, 255);
    // with the switch on a frame needs its image: the depth-only overload throws, before it touches anything
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, O[3] = {0, 0, 0};
    cuda::Depth d;
    d.upload(render(I, O), W);
    DynFusion on(color_params(true, true));
    bool threw = false;
    try {
        on(d);
    } catch (const dfa::Error& e) {
        threw = e.code == DFA_ERR_INVALID;
    }
    ASSERT_TRUE(threw);
    // ... and an image of another size is refused
    cuda::Image small;
    small.upload(ramp(W / 2, H / 2), W / 2);
    threw = false;
    try {
        on(d, small);
    } catch (const dfa::Error& e) {
        threw = e.code == DFA_ERR_INVALID;
    }
    ASSERT_TRUE(threw);
    // canonicalColors with the switch off
    DynFusion off(color_params(true, false));
    threw = false;
    try {
        off.canonicalColors();
    } catch (const dfa::Error& e) {
        threw = e.code == DFA_ERR_INVALID;
    }
    ASSERT_TRUE(threw);
}

// ------------------------------------------------------------------------------------------ the sequence
namespace {
// what one run of the four-frame static sequence leaves for the checks (regrow: north_star_regrow_canonical + model_view)
struct SequenceResult {
    bool geometry_same = true, flags_ok = true, colours_only_where_on = true, mesh_same = true, unlit_are_zero = true, r_ok = true;
    size_t N = 0, got = 0, projecting = 0, lit = 0, lit_projecting = 0, unlit_at_edge = 0;
    float worst_b = 0.f, worst_g = 0.f, bound_b = 0.f, bound_g = 0.f;
};

SequenceResult run_sequence(bool regrow) {
    SequenceResult r;
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, O[3] = {0, 0, 0};
    const std::vector<unsigned short> depth_host = render(I, O);  // the camera does not move
    cuda::Depth d;
    d.upload(depth_host, W);
    cuda::Image image;
    image.upload(ramp(W, H), W);
    float z_min = 1e9f;
    for (unsigned short mm : depth_host)
        if (mm) z_min = std::min(z_min, mm * 0.001f);

    DynFuParams pa = color_params(true, false), pb = color_params(true, true);
    pa.north_star_regrow_canonical = pb.north_star_regrow_canonical = regrow;
    pa.model_view = pb.model_view = regrow;
    DynFusion plain(pa), colour(pb);
    plain.nodeStep = colour.nodeStep = 64;
    for (int f = 0; f < 4; ++f) {
        const bool a = plain(d), b = colour(d, image);
        r.flags_ok = r.flags_ok && a == b && a == (f > 0);
        r.geometry_same = r.geometry_same && same(voxels(*plain.canonicalVolume()), voxels(*colour.canonicalVolume())) &&
                          same(warped_vertices(plain), warped_vertices(colour)) && same(node_transforms(plain), node_transforms(colour));
        r.colours_only_where_on = r.colours_only_where_on && plain.canonicalVolume()->colors() == nullptr &&
                                  colour.canonicalVolume()->colors() != nullptr;
    }
    // the colours of the canonical vertices against the ramp at their own projection: the bound from the parameters
    const float trunc = colour.canonicalVolume()->getTruncDist();
    const float reach = trunc * F / z_min;  // how far a band voxel's pixel can lie from the surface point's
    r.bound_b = 1.f + SLOPE_B * reach, r.bound_g = 1.f + SLOPE_G * reach;
    std::vector<RGB> got;
    colour.canonicalColors().download(got);
    dfa::DeviceArray<float> v3, n3;
    colour.getCanonicalFrame()->deviceArrays(v3, n3);
    std::vector<float> v;
    v3.download(v);
    r.N = colour.getCanonicalFrame()->size(), r.got = got.size();
    if (r.got != r.N || v.size() < 3 * r.N) return r;
    const float cx = W / 2 - 0.5f, cy = H / 2 - 0.5f;
    for (size_t i = 0; i < r.N; ++i) {
        const float x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
        const bool has = (unsigned char)(got[i].bgra >> 24) == 255;
        r.lit += has;
        if (!has) r.unlit_are_zero = r.unlit_are_zero && got[i].bgra == 0;
        if (!(z > 0)) continue;
        const float u = F * x / z + cx, w = F * y / z + cy;
        const int pu = (int)std::floor(u), pv = (int)std::floor(w);
        if (pu < 0 || pv < 0 || pu >= W || pv >= H || depth_host[(size_t)pv * W + pu] == 0) continue;
        ++r.projecting;
        if (!has) {
            // (diagnosis: does the vertex stand at a depth edge — no depth, or a jump of more than trunc, within the band's reach?)
            const int rad = (int)std::ceil(reach) + 1;
            const int here = depth_host[(size_t)pv * W + pu];
            bool edge = false;
            for (int dy = -rad; dy <= rad && !edge; ++dy)
                for (int dx = -rad; dx <= rad && !edge; ++dx) {
                    const int qx = pu + dx, qy = pv + dy;
                    if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
                    const int there = depth_host[(size_t)qy * W + qx];
                    edge = there == 0 || std::abs(there - here) > (int)(1000.f * trunc);
                }
            r.unlit_at_edge += edge;
            continue;
        }
        ++r.lit_projecting;
        r.worst_b = std::max(r.worst_b, std::fabs((float)got[i].b - SLOPE_B * u));
        r.worst_g = std::max(r.worst_g, std::fabs((float)got[i].g - SLOPE_G * w));
        r.r_ok = r.r_ok && got[i].r == 128;
    }
    std::printf("regrow %d: %zu vertices, %zu project onto depth, %zu with colour (%zu of the projecting; of the %zu without, %zu stand at a "
                "depth edge); trunc %.4f m, z_min %.3f m, reach %.2f px; |b - ramp| <= %.2f (bound %.2f), |g - ramp| <= %.2f (bound %.2f)\n",
                (int)regrow, r.N, r.projecting, r.lit, r.lit_projecting, r.projecting - r.lit_projecting, r.unlit_at_edge, trunc, z_min,
                reach, r.worst_b, r.bound_b, r.worst_g, r.bound_g);
    if (regrow) {  // model_view: the kept mesh's vertices get the same
        std::vector<RGB> mesh_colours;
        colour.canonicalMeshColors().download(mesh_colours);
        r.mesh_same = mesh_colours.size() == colour.getCanonicalMesh().vertices.size() && mesh_colours.size() == got.size() &&
                      std::memcmp(mesh_colours.data(), got.data(), got.size() * sizeof(RGB)) == 0;
    }
    return r;
}

const SequenceResult& sequence(bool regrow) {
    static SequenceResult res[2];
    static bool have[2] = {false, false};
    if (!have[regrow]) res[regrow] = run_sequence(regrow), have[regrow] = true;
    return res[regrow];
}
}  // namespace

// geometry bit for bit that of north_star_fuse_canonical alone, and every coloured vertex that projects onto depth holds the
// ramp at its own projection within 1 + s * trunc * f / z_min (s: the ramp's slope per pixel)
TEST(HostColorTest, StaticSequenceBeforeAColourRamp) {
    for (const bool regrow : {false, true}) {
        const SequenceResult& r = sequence(regrow);
        ASSERT_TRUE(r.flags_ok && r.geometry_same && r.colours_only_where_on);
        ASSERT_TRUE(r.N > 1000 && r.got == r.N && r.projecting > 1000 && r.unlit_are_zero);
        ASSERT_TRUE(r.lit_projecting > 1000 && r.worst_b <= r.bound_b && r.worst_g <= r.bound_g && r.r_ok);
        ASSERT_TRUE(r.mesh_same);
    }
}

// a = 255 on at least the share of vertices that project inside the image onto non-zero depth.  The vertices are marching
// cubes' — half a voxel off the lattice the colours were fused on — and DynFusion samples them ON their lattice edge
// (TsdfVolume::sampleColors: lattice_offset 0.5), between the two voxels each was interpolated from: the one behind the
// surface always has a colour, so every vertex has one, the closing walls at the scene's depth edges included (sampled half
// a voxel diagonal away, 550 of the 102 615 vertices found less than a quarter of their cell's weight on coloured voxels).
TEST(HostColorTest, EveryProjectingVertexHasAColour) {
    for (const bool regrow : {false, true}) {
        const SequenceResult& r = sequence(regrow);
        ASSERT_TRUE(r.projecting > 1000);
        ASSERT_TRUE(r.lit >= r.projecting);
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
