// test_host_extract.cpp — kfusion::cuda::TsdfVolume::fetchCloud / fetchNormals (reference: include/kfusion/cuda/
// tsdf_volume.hpp:49-50, src/kfusion/tsdf_volume.cpp:131-160) on an integrated depth frame: the adaptor's results are
// the C entry points' (dfa_tsdf_extract_cloud / dfa_tsdf_extract_normals, themselves checked against the numpy
// statement by tests/test_gpu_extract.py), bit for bit, with the reference's buffer behaviour and pose handling.
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <string>

#include <unistd.h>

#include <dfa_host/io.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>

#include "../../include/dynfu_amd.h"
#include "minitest.hpp"

using namespace kfusion;

namespace {
const int W = 160, H = 120, DIM = 64;

std::vector<unsigned short> make_depth() {  // a bump in front of a wall (test_host_tsdf.cpp)
    std::vector<unsigned short> d((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float u = (x - W / 2) / (float)W, v = (y - H / 2) / (float)H;
            const float r2 = u * u + v * v;
            d[(size_t)y * W + x] = r2 < 0.09f ? (unsigned short)(1200 + 900 * r2 * 10) : 2400;
            if (x < 3 || y < 3 || x >= W - 3 || y >= H - 3) d[(size_t)y * W + x] = 0;
        }
    return d;
}

// a volume of the KinFu set-up (kinfu.cpp:20-38) with one fused frame
struct Scene {
    cuda::TsdfVolume vol{Vec3i::all(DIM)};
    Intr intr{131.25f, 131.25f, W / 2 - 0.5f, H / 2 - 0.5f};
    Scene() {
        vol.setTruncDist(0.04f), vol.setMaxWeight(64), vol.setSize(Vec3f::all(3.f));
        vol.setPose(Affine3f().translate(Vec3f(-1.5f, -1.5f, 0.5f)));
        vol.setGradientDeltaFactor(0.5f);
        cuda::Depth depth;
        depth.upload(make_depth(), W);
        cuda::Dists dists;
        cuda::computeDists(depth, dists, intr);
        vol.clearAndIntegrate(dists, Affine3f(), intr);
    }
    const cuda::TsdfVolume& cvol() const { return vol; }  // (the const data(): the occupancy map stays trusted)
};

// dfa_tsdf_extract_cloud called directly with the volume's settings
std::vector<Point> direct_cloud(const cuda::TsdfVolume& vol, int cap, int& total) {
    float aff[12];
    vol.getPose().to12(aff);
    const Vec3f vs = vol.getVoxelSize();
    dfa::DeviceArray<Point> out((size_t)std::max(cap, 1));
    dfa::DeviceArray<int> tot(1);
    dfa::check(dfa_tsdf_extract_cloud(vol.data().ptr<uint32_t>(), DIM, DIM, DIM, vs.v, aff, (float*)out.ptr(), cap, tot.ptr(),
                                      nullptr),
               "dfa_tsdf_extract_cloud");
    std::vector<int> t;
    tot.download(t);
    total = t[0];
    std::vector<Point> h;
    out.download(h);
    h.resize((size_t)std::min(total, cap));
    return h;
}

bool same_bits(const std::vector<Point>& a, const std::vector<Point>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Point)) == 0;
}
}  // namespace

TEST(TsdfVolumeTest, FetchCloudMatchesTheCEntryPoint) {
    Scene s;
    ASSERT_TRUE(s.cvol().occupancy() != nullptr);  // the adaptor takes the _occ entry point here
    dfa::DeviceArray<Point> buffer;
    dfa::DeviceArray<Point> cloud = s.cvol().fetchCloud(buffer);
    ASSERT_EQ(buffer.size(), (size_t)10 * 1000 * 1000);  // DEFAULT_CLOUD_BUFFER_SIZE (tsdf_volume.cpp:132)
    ASSERT_TRUE(cloud.ptr() == buffer.ptr());             // a view of the buffer
    int total = 0;
    const std::vector<Point> want = direct_cloud(s.cvol(), 1 << 20, total);
    ASSERT_TRUE(total > 1000 && total < (1 << 20));
    ASSERT_EQ(cloud.size(), (size_t)total);
    std::vector<Point> got;
    cloud.download(got);
    ASSERT_TRUE(same_bits(got, want));
    // the points lie on the fused surface: the wall at z = 2.4 m or the bump in front of it (camera = world frame)
    size_t on = 0;
    for (const Point& p : got) on += p.w == 0.f && p.z > 1.0f && p.z < 2.5f;
    ASSERT_EQ(on, got.size());
    // without the map (a writable data() handle makes it unknown): the same cloud
    cuda::TsdfVolume copy(s.vol);
    ASSERT_TRUE(copy.occupancy() == nullptr);
    dfa::DeviceArray<Point> buffer2(total + 7);
    std::vector<Point> got2;
    copy.fetchCloud(buffer2).download(got2);
    ASSERT_TRUE(same_bits(got2, want));
}

TEST(TsdfVolumeTest, FetchCloudIntoATooSmallBufferKeepsTheFirstPoints) {
    Scene s;
    int total = 0;
    const std::vector<Point> all = direct_cloud(s.cvol(), 1 << 20, total);
    for (int cap : {1, 100, total - 1, total, total + 1}) {
        dfa::DeviceArray<Point> buffer((size_t)cap);
        dfa::DeviceArray<Point> cloud = s.cvol().fetchCloud(buffer);
        ASSERT_EQ(cloud.size(), (size_t)std::min(total, cap));
        std::vector<Point> got;
        cloud.download(got);
        ASSERT_TRUE(same_bits(got, std::vector<Point>(all.begin(), all.begin() + std::min(total, cap))));
    }
}

TEST(TsdfVolumeTest, FetchNormalsMatchesTheCEntryPoint) {
    Scene s;
    dfa::DeviceArray<Point> buffer;
    const dfa::DeviceArray<Point> cloud = s.cvol().fetchCloud(buffer);
    dfa::DeviceArray<Normal> normals;
    s.cvol().fetchNormals(cloud, normals);
    ASSERT_EQ(normals.size(), cloud.size());
    float aff[12], rinv[9];
    s.vol.getPose().to12(aff), s.vol.getPose().inverse_rotation(rinv);
    const Vec3f vs = s.vol.getVoxelSize();
    dfa::DeviceArray<Normal> direct(cloud.size());
    dfa::check(dfa_tsdf_extract_normals(s.cvol().data().ptr<uint32_t>(), DIM, DIM, DIM, vs.v, aff, rinv, 0.5f,
                                        (const float*)cloud.ptr(), (int)cloud.size(), (float*)direct.ptr(), nullptr),
               "dfa_tsdf_extract_normals");
    std::vector<Normal> got, want;
    normals.download(got), direct.download(want);
    ASSERT_TRUE(same_bits(got, want));
    size_t unit = 0;
    for (const Normal& n : got) unit += std::fabs(n.x * n.x + n.y * n.y + n.z * n.z - 1.f) < 1e-5f;
    ASSERT_TRUE(unit > got.size() * 3 / 4);  // NaN only near the volume's border
}

TEST(TsdfVolumeTest, FetchCloudAppliesThePose) {
    Scene s;
    int total = 0;
    dfa::DeviceArray<Point> buffer;
    std::vector<Point> before, after;
    s.cvol().fetchCloud(buffer).download(before);
    // the volume turned 30 degrees about y and moved: the same voxels, the points moved with it
    const float c = std::cos(0.5235988f), sn = std::sin(0.5235988f);
    Affine3f pose;
    const float R[9] = {c, 0, sn, 0, 1, 0, -sn, 0, c};
    for (int i = 0; i < 9; ++i) pose.R[i] = R[i];
    pose.t[0] = 0.25f, pose.t[1] = -1.5f, pose.t[2] = 1.0f;
    const Affine3f old = s.vol.getPose();
    s.vol.setPose(pose);
    s.cvol().fetchCloud(buffer).download(after);
    ASSERT_EQ(after.size(), before.size());
    ASSERT_TRUE(same_bits(after, direct_cloud(s.cvol(), (int)before.size(), total)));
    const Affine3f rel = pose * old.inv();
    double worst = 0;
    for (size_t i = 0; i < before.size(); ++i) {
        const Point& p = before[i];
        for (int k = 0; k < 3; ++k) {
            const float e = rel.R[3 * k] * p.x + rel.R[3 * k + 1] * p.y + rel.R[3 * k + 2] * p.z + rel.t[k];
            worst = std::max(worst, (double)std::fabs(e - (&after[i].x)[k]));
        }
    }
    ASSERT_NEAR(worst, 0.0, 1e-5);
}

TEST(TsdfVolumeTest, FetchedCloudSavesAsPcd) {
    Scene s;
    dfa::DeviceArray<Point> buffer;
    std::vector<Point> pts;
    s.cvol().fetchCloud(buffer).download(pts);
    dfa::PointCloud<dfa::PointXYZ> cloud;
    for (const Point& p : pts) cloud.push_back(dfa::PointXYZ(p.x, p.y, p.z));
    const std::string path = (std::filesystem::temp_directory_path() / ("dfa_fetch_cloud_" + std::to_string(::getpid()) + ".pcd")).string();
    dfa::io::savePCDFileASCII(path, cloud);
    std::ifstream in(path);
    std::string line;
    size_t header_points = 0, rows = 0;
    bool data = false;
    while (std::getline(in, line)) {
        if (data) rows += !line.empty();
        else if (line.rfind("POINTS ", 0) == 0) header_points = std::stoul(line.substr(7));
        else if (line.rfind("DATA ascii", 0) == 0) data = true;
    }
    std::remove(path.c_str());
    ASSERT_EQ(header_points, pts.size());
    ASSERT_EQ(rows, pts.size());
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
