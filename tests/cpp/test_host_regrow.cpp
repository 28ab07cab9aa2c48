// test_host_regrow.cpp — the growing canonical model (DynFuParams::north_star_regrow_canonical, canonical_min_weight,
// fuse_unsupported_rigid; DynFusion::getCanonicalFrame, canonicalVertexCount, regrowSkippedFrames).  Frame 0 sees the left half
// of a sphere, frames 1-3 the whole sphere: the canonical cloud after every later frame is the canonical volume's welded
// surface at the weight floor — the public calls' bits —, it reaches the right half one frame after the fusion has (weight 2),
// the nodes follow it, each switch changes only what it names, the model view and the visibility test run on the regrown
// mesh, and the switches' rules.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <dynfu/dyn_fusion.hpp>
#include <kfusion/cuda/marching_cubes.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>

#include "../../include/dynfu_amd.h"
#include "dynfu_fixtures.hpp"
#include "minitest.hpp"

using namespace kfusion;
using namespace dynfu_fixtures;
using namespace dynfu_fixtures::sphere_scene;

namespace {
const int DIM = 64;
const float VOXEL = 3.f / DIM;

struct Switches {
    bool rigid = true, regrow = true, knn_field = false, view = false;
};
DynFuParams params(const Switches& s) {
    DynFuParams p = DynFuParams::defaultParams();
    p.kinfuParams.cols = W, p.kinfuParams.rows = H;
    p.kinfuParams.intr = Intr(F, F, W / 2 - 0.5f, H / 2 - 0.5f);
    p.kinfuParams.volume_dims = Vec3i::all(DIM);
    p.epsilon = 0.05f;
    p.north_star = true, p.north_star_fuse_canonical = true;
    p.fuse_unsupported_rigid = s.rigid, p.north_star_regrow_canonical = s.regrow, p.canonical_min_weight = 2;
    p.fuse_knn_field = s.knn_field;
    p.model_view = p.north_star_visible_only = s.view;
    return p;
}

struct Depths {
    cuda::Depth d[4];
    Depths() {
        for (int f = 0; f < 4; ++f) d[f].upload(sphere_depth(1.5f - 0.01f * f, f == 0), W);  // 1 cm closer per frame
    }
};

// a frame's packed device arrays on the host
struct Cloud3 {
    std::vector<float> v, n;
};
Cloud3 download(const std::shared_ptr<dynfu::Frame>& f) {
    Cloud3 c;
    dfa::DeviceArray<float> v3, n3;
    f->deviceArrays(v3, n3);
    if (f->size()) v3.download(c.v), n3.download(c.n);
    return c;
}
float max_x(const std::vector<float>& xyz) {
    float m = -1e30f;
    for (size_t i = 0; i < xyz.size(); i += 3) m = std::max(m, xyz[i]);
    return m;
}
float min_x(const std::vector<float>& xyz) {
    float m = 1e30f;
    for (size_t i = 0; i < xyz.size(); i += 3) m = std::min(m, xyz[i]);
    return m;
}

// the canonical cloud by the public calls: runIndexed at the floor, gradient normals, packed, to the camera frame
Cloud3 by_public_calls(const cuda::TsdfVolume& vol, int min_weight, const Affine3f& vol2cam) {
    cuda::MarchingCubes mc;
    dfa::DeviceArray<cuda::MarchingCubes::PointType> vb;
    dfa::DeviceArray<int> ib;
    const auto mesh = mc.runIndexed(vol, vb, ib, min_weight);
    Cloud3 c;
    const size_t n = mesh.vertices.size();
    if (n == 0) return c;
    dfa::DeviceArray<dfa::Normal> n4;
    mc.computeNormals(vol, mesh.vertices, n4);
    dfa::DeviceArray<float> v3(3 * n), n3(3 * n);
    float aff[12];
    vol2cam.to12(aff);
    dfa::check(dfa_repack_points((const float*)mesh.vertices.ptr(), 4, v3.ptr(), 3, (int)n, 0.f, nullptr), "repack");
    dfa::check(dfa_repack_points((const float*)n4.ptr(), 4, n3.ptr(), 3, (int)n, 0.f, nullptr), "repack");
    dfa::check(dfa_transform_points(v3.ptr(), (int)n, aff, 1, v3.ptr(), nullptr), "transform");
    dfa::check(dfa_transform_points(n3.ptr(), (int)n, aff, 0, n3.ptr(), nullptr), "transform");
    v3.download(c.v), n3.download(c.n);
    return c;
}
}  // namespace

// (a) - (d): the cloud is the public calls', it grows a frame after the fusion has, the nodes follow
TEST(RegrowTest, TheCloudIsTheCanonicalVolumesSurfaceAtTheFloorAndGrows) {
    Depths in;
    DynFusion df(params(Switches{}));
    df.nodeStep = 16;
    float cloud0_min = 0, cloud0_max = 0, node0_max = 0;
    size_t count0 = 0, nodes1 = 0;
    for (int f = 0; f < 4; ++f) {
        ASSERT_TRUE(df(in.d[f]) == (f > 0));
        const Cloud3 cloud = download(df.getCanonicalFrame());
        ASSERT_EQ(cloud.v.size(), 3 * df.canonicalVertexCount());
        ASSERT_TRUE(df.canonicalVertexCount() > 100);
        std::vector<float> pos, w, dq;
        df.getWarpfield()->hostArrays(pos, w, dq);
        const Affine3f vol2cam = df.tsdf().getPose();  // the camera stays at the origin
        std::printf("frame %d: %zu canonical vertices, x in [%.3f, %.3f], %zu nodes, node x up to %.3f, %d skipped\n", f,
                    df.canonicalVertexCount(), min_x(cloud.v), max_x(cloud.v), w.size(), max_x(pos), df.regrowSkippedFrames());
        ASSERT_EQ(df.regrowSkippedFrames(), 0);
        if (f == 0) {
            // the welded vertex set of the frame-0 volume (every weight is 1: no floor)
            const Cloud3 want = by_public_calls(static_cast<const cuda::TsdfVolume&>(df.tsdf()), 1, vol2cam);
            ASSERT_TRUE(same(cloud.v, want.v) && same(cloud.n, want.n));
            cloud0_min = min_x(cloud.v), cloud0_max = max_x(cloud.v), count0 = df.canonicalVertexCount(), node0_max = max_x(pos);
            ASSERT_TRUE(cloud0_max < 2 * VOXEL);  // the left half, in the camera frame
            continue;
        }
        // (a) the public calls' bits, every frame
        const Cloud3 want = by_public_calls(*df.canonicalVolume(), 2, vol2cam);
        ASSERT_TRUE(!want.v.empty());
        ASSERT_TRUE(same(cloud.v, want.v) && same(cloud.n, want.n));
        // getCanonicalWarpedToLive() stays the cloud the solve used: the one before this frame's re-extraction
        ASSERT_TRUE(df.getCanonicalWarpedToLive()->size() > 0);
        if (f == 1) {
            ASSERT_EQ(df.getCanonicalWarpedToLive()->size(), count0);
            // the right half has weight 1: below the floor
            ASSERT_TRUE(max_x(cloud.v) <= cloud0_max + 2 * VOXEL && min_x(cloud.v) >= cloud0_min - 2 * VOXEL);
            nodes1 = w.size();
        }
        if (f == 2) {
            ASSERT_TRUE(max_x(cloud.v) > cloud0_max + 2 * VOXEL);  // (b)
            ASSERT_TRUE(df.canonicalVertexCount() > count0);       // (c)
        }
        if (f == 3) {  // (d) seeds come from the regrown cloud, one 5 cm cell per seed
            ASSERT_TRUE(w.size() > nodes1);
            ASSERT_TRUE(max_x(pos) > node0_max + 0.05f);
        }
    }
}

// (e) each switch's own effect
TEST(RegrowTest, EachSwitchChangesOnlyWhatItNames) {
    Depths in;
    Switches with_field, no_regrow, no_rigid;
    with_field.knn_field = true, no_regrow.regrow = false, no_rigid.rigid = false;
    DynFusion base(params(Switches{})), field(params(with_field)), plain(params(no_regrow)), skip(params(no_rigid));
    base.nodeStep = field.nodeStep = plain.nodeStep = skip.nodeStep = 16;
    cuda::TsdfVolume hand{Vec3i::all(DIM)};
    size_t skip_nodes0 = 0;
    std::vector<uint32_t> base1;
    for (int f = 0; f < 3; ++f) {
        base(in.d[f]), field(in.d[f]);
        // the k-NN field changes nothing: the same canonical volume and cloud, bit for bit
        ASSERT_TRUE(same(voxels(*base.canonicalVolume()), voxels(*field.canonicalVolume())));
        const Cloud3 a = download(base.getCanonicalFrame()), b = download(field.getCanonicalFrame());
        ASSERT_TRUE(!a.v.empty() && same(a.v, b.v) && same(a.n, b.n));
        if (f > 1) continue;
        if (f == 1) base1 = voxels(*base.canonicalVolume());
        skip(in.d[f]);
        std::vector<float> pos, w, dq;
        skip.getWarpfield()->hostArrays(pos, w, dq);
        if (f == 0) {
            hand.setSize(skip.tsdf().getSize()), hand.setPose(skip.tsdf().getPose());
            hand.setTruncDist(skip.tsdf().getTruncDist()), hand.setMaxWeight(skip.tsdf().getMaxWeight());
            hand.copyVoxelsFrom(*skip.canonicalVolume());
            skip_nodes0 = w.size();
            continue;
        }
        // without fuse_unsupported_rigid: north_star_fuse_canonical as it was — integrateWarped6 with Skip, by hand, through
        // the nodes the solve had (the first D: Warpfield::update has grown the field since)
        ASSERT_TRUE(skip_nodes0 > 5 && w.size() >= skip_nodes0);
        dfa::DeviceArray<float> dpos, dw, ddq;
        dpos.upload(std::vector<float>(pos.begin(), pos.begin() + 3 * skip_nodes0));
        dw.upload(std::vector<float>(w.begin(), w.begin() + skip_nodes0));
        ddq.upload(std::vector<float>(dq.begin(), dq.begin() + 8 * skip_nodes0));
        const KinFuParams& kp = skip.KinFu::params();
        cuda::Dists dists;
        cuda::computeDists(in.d[1], dists, kp.intr);
        hand.integrateWarped6(dists, Affine3f(), kp.intr, Affine3f(), dpos.ptr(), ddq.ptr(), dw.ptr(), (int)skip_nodes0,
                              std::min(skip.getWarpfield()->getKnn(), 8));
        ASSERT_TRUE(same(voxels(hand), voxels(*skip.canonicalVolume())));
        // ... and the rigid integration reaches voxels that one leaves alone
        const std::vector<uint32_t> vb = voxels(*base.canonicalVolume()), vs = voxels(*skip.canonicalVolume());
        size_t more = 0;
        for (size_t i = 0; i < vb.size(); ++i) more += (vb[i] >> 16) > (vs[i] >> 16);
        std::printf("frame 1: %zu voxels have a weight only with fuse_unsupported_rigid\n", more);
        ASSERT_TRUE(more > 200);
    }
    // the regrow switch off, the others on.  Its frame 0 keeps the triangle soup as the canonical cloud (the switch's frame-0
    // rule), so its nodes — every nodeStep-th vertex of another cloud — and with them frame 1's solve and warped fusion are
    // other ones: the two canonical volumes after frame 1 cannot be equal bit for bit (measured: 717 of 262 144 voxels differ,
    // 130 of them in their weight).  What the switch itself adds to frame 1 comes after the fusion; that the fusion is the
    // existing call is the next test.
    for (int f = 0; f < 2; ++f) plain(in.d[f]);
    ASSERT_TRUE(plain.canonicalVertexCount() > base.canonicalVertexCount() && plain.regrowSkippedFrames() == 0);
    const std::vector<uint32_t> off1 = voxels(*plain.canonicalVolume());
    size_t differ = 0, weights = 0;
    for (size_t i = 0; i < off1.size(); ++i) differ += off1[i] != base1[i], weights += (off1[i] >> 16) != (base1[i] >> 16);
    std::printf("regrow off against on after frame 1: %zu voxels differ, %zu in their weight\n", differ, weights);
}

// (e), second bullet, in the form that can hold: up to and including frame 1's fusion the regrow switch has changed nothing but
// the cloud frame 0 extracts — the regrow run's canonical volume after frame 1 is the existing call, integrateWarped6 with
// Rigid, applied by hand to frame 0's volume through the nodes its solve had.
TEST(RegrowTest, TheFusionOfFrameOneIsTheExistingCallWithRigid) {
    Depths in;
    DynFusion df(params(Switches{}));
    df.nodeStep = 16;
    df(in.d[0]);
    cuda::TsdfVolume hand{Vec3i::all(DIM)};
    hand.setSize(df.tsdf().getSize()), hand.setPose(df.tsdf().getPose());
    hand.setTruncDist(df.tsdf().getTruncDist()), hand.setMaxWeight(df.tsdf().getMaxWeight());
    hand.copyVoxelsFrom(*df.canonicalVolume());
    std::vector<float> pos, w, dq;
    df.getWarpfield()->hostArrays(pos, w, dq);
    const size_t D0 = w.size();
    df(in.d[1]);
    df.getWarpfield()->hostArrays(pos, w, dq);
    ASSERT_TRUE(D0 > 5 && w.size() >= D0);
    dfa::DeviceArray<float> dpos, dw, ddq;
    dpos.upload(std::vector<float>(pos.begin(), pos.begin() + 3 * D0));
    dw.upload(std::vector<float>(w.begin(), w.begin() + D0));
    ddq.upload(std::vector<float>(dq.begin(), dq.begin() + 8 * D0));
    const KinFuParams& kp = df.KinFu::params();
    cuda::Dists dists;
    cuda::computeDists(in.d[1], dists, kp.intr);
    hand.integrateWarped6(dists, Affine3f(), kp.intr, Affine3f(), dpos.ptr(), ddq.ptr(), dw.ptr(), (int)D0,
                          std::min(df.getWarpfield()->getKnn(), 8), cuda::TsdfVolume::UnsupportedMode::Rigid);
    ASSERT_TRUE(same(voxels(hand), voxels(*df.canonicalVolume())));
}

// (f) with the model view and the visible-surface data term
TEST(RegrowTest, TheModelViewAndTheVisibilityTestFollowTheRegrownMesh) {
    Depths in;
    Switches s;
    s.view = true;
    DynFusion df(params(s));
    df.nodeStep = 16;
    for (int f = 0; f < 4; ++f) {
        ASSERT_TRUE(df(in.d[f]) == (f > 0));
        const auto mesh = df.getCanonicalMesh();
        ASSERT_EQ(mesh.vertices.size(), df.canonicalVertexCount());  // the mesh is the cloud's mesh
        ASSERT_TRUE(mesh.indices.size() > 0 && mesh.indices.size() % 3 == 0);
        // the float4 vertices handed out are the cloud's
        std::vector<cuda::MarchingCubes::PointType> v4;
        mesh.vertices.download(v4);
        const Cloud3 cloud = download(df.getCanonicalFrame());
        size_t differ = 0;
        for (size_t i = 0; i < v4.size(); ++i)
            differ += std::memcmp(&v4[i].x, &cloud.v[3 * i], 3 * sizeof(float)) != 0;
        ASSERT_EQ(differ, (size_t)0);
        if (f > 0) {
            const long long seen = df.northStarVisibleVertices();
            ASSERT_TRUE(seen > 0);  // (this frame's solve tested the cloud it started from)
        }
        cuda::Image image;
        df.renderWarpedModel(image, 0);  // between the frames: on the mesh just regrown, a plan of its size
        const Cloud3 warped = download(df.warpCanonicalMesh());
        ASSERT_EQ(warped.v.size(), cloud.v.size());
        float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f}, moved = 0.f;
        for (size_t i = 0; i < warped.v.size(); ++i) {
            lo[i % 3] = std::min(lo[i % 3], warped.v[i]), hi[i % 3] = std::max(hi[i % 3], warped.v[i]);
            moved = std::max(moved, std::fabs(warped.v[i] - cloud.v[i]));
        }
        std::printf("frame %d: warped mesh in [%.3f, %.3f] x [%.3f, %.3f] x [%.3f, %.3f], a vertex moves by up to %.3f m\n", f, lo[0],
                    hi[0], lo[1], hi[1], lo[2], hi[2], moved);
        std::vector<Point> map;
        int cols = 0;
        df.getWarpedModelMaps().points.download(map, cols);
        ASSERT_TRUE(cols == W && map.size() == (size_t)W * H);
        size_t left = 0, right = 0;
        int last_column = -1;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (!std::isnan(map[(size_t)y * W + x].x)) {
                    if (x >= W / 2 + 8) ++right;
                    else ++left;
                    last_column = std::max(last_column, x);
                }
        std::printf("frame %d: %zu mesh vertices, model pixels left %zu, right of the centre by 8 and more %zu, last column %d\n",
                    f, mesh.vertices.size(), left, right, last_column);
        ASSERT_TRUE(left > 500);
        if (f < 2) ASSERT_EQ(right, (size_t)0);  // the model is still the left half
        if (f == 3) ASSERT_TRUE(right > 500);
    }
}

// (g) the switches' rules
TEST(RegrowTest, ConstructorRules) {
    DynFuParams p = params(Switches{});
    ASSERT_TRUE(!construction_throws(p));
    DynFuParams a = p;  // fuse_unsupported_rigid without a fusion switch
    a.north_star_regrow_canonical = false, a.north_star_fuse_canonical = false;
    ASSERT_TRUE(construction_throws(a));
    DynFuParams b = p;  // regrow without north_star
    b.north_star = false, b.north_star_fuse_canonical = false, b.fuse_canonical = true;
    ASSERT_TRUE(construction_throws(b));
    DynFuParams c = p;  // regrow without north_star_fuse_canonical
    c.north_star_fuse_canonical = false, c.fuse_unsupported_rigid = false;
    ASSERT_TRUE(construction_throws(c));
    DynFuParams d = p;  // a floor outside the weight's 16 bits
    d.canonical_min_weight = 0;
    ASSERT_TRUE(construction_throws(d));
    d.canonical_min_weight = 65536;
    ASSERT_TRUE(construction_throws(d));
    DynFuParams e = p;  // fuse_unsupported_rigid in reference mode, with and without the field
    e.north_star = e.north_star_fuse_canonical = e.north_star_regrow_canonical = false, e.fuse_canonical = true;
    ASSERT_TRUE(!construction_throws(e));
    e.fuse_knn_field = true;
    ASSERT_TRUE(!construction_throws(e));
    // the defaults: everything off, the floor 2
    const DynFuParams def = DynFuParams::defaultParams();
    ASSERT_TRUE(!def.north_star_regrow_canonical && !def.fuse_unsupported_rigid && def.canonical_min_weight == 2);
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
