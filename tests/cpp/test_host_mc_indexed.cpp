// test_host_mc_indexed.cpp — kfusion::cuda::MarchingCubes::runIndexed, dfa::convertToIndexedMesh and
// KinFu-style mesh output on an integrated depth frame: the indexed mesh against run()'s triangle soup (itself checked
// against the numpy statement by tests/test_gpu_mc.py; the C entry point against its own statement by
// tests/test_gpu_mc_indexed.py), the winding, and the VTK text read back.
#include <cmath>
#include <cstring>
#include <sstream>
#include <string>

#include <dfa_host/io.hpp>
#include <kfusion/cuda/marching_cubes.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>

#include "../../include/dynfu_amd.h"
#include "minitest.hpp"

using namespace kfusion;
typedef cuda::MarchingCubes::PointType P;

namespace {
const int W = 160, H = 120, DIM = 64;

std::vector<unsigned short> make_depth() {  // a bump in front of a wall (test_host_extract.cpp)
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

struct HostMesh {
    std::vector<P> vertices;
    std::vector<int> indices;
};

HostMesh indexed(cuda::MarchingCubes& mc, const cuda::TsdfVolume& vol) {
    dfa::DeviceArray<P> vb;
    dfa::DeviceArray<int> ib;
    const auto m = mc.runIndexed(vol, vb, ib);
    HostMesh h;
    if (!m.vertices.empty()) m.vertices.download(h.vertices), m.indices.download(h.indices);
    return h;
}
}  // namespace

TEST(MarchingCubesTest, RunIndexedAgainstRun) {
    Scene s;
    ASSERT_TRUE(s.cvol().occupancy() != nullptr);  // the adaptor hands the map to the entry point here
    cuda::MarchingCubes mc;
    dfa::DeviceArray<P> buffer;
    std::vector<P> soup;
    mc.run(s.cvol(), buffer).download(soup);
    const int soup_total = mc.totalVertices();
    ASSERT_TRUE(soup_total > 3000 && soup_total % 3 == 0);
    dfa::DeviceArray<P> vb;
    dfa::DeviceArray<int> ib;
    const auto m = mc.runIndexed(s.cvol(), vb, ib);
    ASSERT_EQ(ib.size(), (size_t)cuda::MarchingCubes::DEFAULT_TRIANGLES_BUFFER_SIZE);
    ASSERT_EQ(vb.size(), (size_t)cuda::MarchingCubes::DEFAULT_TRIANGLES_BUFFER_SIZE / 3);
    ASSERT_TRUE(m.vertices.ptr() == vb.ptr() && m.indices.ptr() == ib.ptr());  // views of the buffers
    ASSERT_EQ(mc.totalVertices(), soup_total);                                  // one index per soup vertex
    ASSERT_EQ(m.indices.size(), (size_t)soup_total);
    ASSERT_EQ(m.vertices.size(), (size_t)mc.totalUniqueVertices());
    ASSERT_TRUE(mc.totalUniqueVertices() * 4 < soup_total && mc.totalUniqueVertices() * 7 > soup_total);
    HostMesh h;
    m.vertices.download(h.vertices), m.indices.download(h.indices);
    // soup vertex i is vertex indices[i]: the same lattice edge, interpolated from one end or the other — equal across the
    // edge bit for bit, along it within a few float32 ulps of the coordinate (< 1e-6 m in this 3 m volume)
    size_t same = 0;
    double worst = 0;
    for (int i = 0; i < soup_total; ++i) {
        ASSERT_TRUE(h.indices[i] >= 0 && h.indices[i] < (int)h.vertices.size());
        const P &a = soup[i], &b = h.vertices[h.indices[i]];
        const int eq = (a.x == b.x) + (a.y == b.y) + (a.z == b.z);
        ASSERT_TRUE(eq >= 2 && b.pad == 1.f);
        same += eq == 3;
        worst = std::max({worst, (double)std::fabs(a.x - b.x), (double)std::fabs(a.y - b.y), (double)std::fabs(a.z - b.z)});
    }
    ASSERT_TRUE(worst < 1e-6);
    ASSERT_TRUE(same > (size_t)soup_total * 9 / 10);
    // every vertex is used, none twice in a triangle
    std::vector<char> used(h.vertices.size(), 0);
    for (int i = 0; i < soup_total; i += 3) {
        ASSERT_TRUE(h.indices[i] != h.indices[i + 1] && h.indices[i + 1] != h.indices[i + 2] && h.indices[i] != h.indices[i + 2]);
        used[h.indices[i]] = used[h.indices[i + 1]] = used[h.indices[i + 2]] = 1;
    }
    size_t n_used = 0;
    for (char u : used) n_used += u;
    ASSERT_EQ(n_used, h.vertices.size());
    // without the map (a writable data() handle makes it unknown): the same mesh
    cuda::TsdfVolume copy(s.vol);
    ASSERT_TRUE(copy.occupancy() == nullptr);
    const HostMesh h2 = indexed(mc, copy);
    ASSERT_TRUE(h2.indices == h.indices && h2.vertices.size() == h.vertices.size() &&
                std::memcmp(h2.vertices.data(), h.vertices.data(), h.vertices.size() * sizeof(P)) == 0);
}

TEST(MarchingCubesTest, RunIndexedIntoTooSmallBuffersReturnsNothingAndTheTotals) {
    Scene s;
    cuda::MarchingCubes mc;
    const HostMesh all = indexed(mc, s.cvol());
    const int nv = mc.totalUniqueVertices(), ni = mc.totalVertices();
    ASSERT_EQ((size_t)nv, all.vertices.size());
    {
        dfa::DeviceArray<P> vb((size_t)nv - 1);
        dfa::DeviceArray<int> ib((size_t)ni);
        const auto m = mc.runIndexed(s.cvol(), vb, ib);
        ASSERT_TRUE(m.vertices.empty() && m.indices.empty());
        ASSERT_EQ(mc.totalUniqueVertices(), nv);
        ASSERT_EQ(mc.totalVertices(), ni);
    }
    {
        dfa::DeviceArray<P> vb((size_t)nv);
        dfa::DeviceArray<int> ib((size_t)ni - 1);
        const auto m = mc.runIndexed(s.cvol(), vb, ib);
        ASSERT_TRUE(m.vertices.empty() && m.indices.empty());
        ASSERT_EQ(mc.totalVertices(), ni);
    }
    {
        dfa::DeviceArray<P> vb((size_t)nv);
        dfa::DeviceArray<int> ib((size_t)ni);
        const auto m = mc.runIndexed(s.cvol(), vb, ib);
        std::vector<int> idx;
        m.indices.download(idx);
        ASSERT_TRUE(m.vertices.size() == (size_t)nv && idx == all.indices);
    }
}

TEST(MarchingCubesTest, NormalsOfTheDistinctVertices) {
    Scene s;
    cuda::MarchingCubes mc;
    dfa::DeviceArray<P> vb;
    dfa::DeviceArray<int> ib;
    const auto m = mc.runIndexed(s.cvol(), vb, ib);
    dfa::DeviceArray<dfa::Normal> normals;
    mc.computeNormals(s.cvol(), m.vertices, normals);
    std::vector<dfa::Normal> n;
    normals.download(n);
    ASSERT_TRUE(n.size() >= m.vertices.size());
    size_t unit = 0;
    for (size_t i = 0; i < m.vertices.size(); ++i) {
        const float* d = n[i].data_c;
        unit += std::fabs(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - 1.f) < 1e-5f;
    }
    ASSERT_TRUE(unit > m.vertices.size() * 3 / 4);
}

TEST(IndexedMeshTest, ConvertToIndexedMeshWindingAndVtkText) {
    using dfa::PointXYZ;
    const std::vector<PointXYZ> v = {PointXYZ(0, 0, 0), PointXYZ(1, 0, 0), PointXYZ(0, 1, 0), PointXYZ(1.23456789f, 1, 0)};
    const std::vector<int> idx = {0, 1, 2, 2, 1, 3};
    const dfa::PolygonMesh m = dfa::convertToIndexedMesh(v, idx);
    ASSERT_EQ(m.cloud.points.size(), (size_t)4);
    ASSERT_EQ(m.polygons.size(), (size_t)2);
    ASSERT_TRUE((m.polygons[0] == std::vector<uint32_t>{0, 2, 1}));  // (idx[3i], idx[3i + 2], idx[3i + 1]): convertToMesh's
    ASSERT_TRUE((m.polygons[1] == std::vector<uint32_t>{2, 3, 1}));
    const std::string want =
        "# vtk DataFile Version 3.0\nvtk output\nASCII\nDATASET POLYDATA\nPOINTS 4 float\n"
        "0 0 0\n1 0 0\n0 1 0\n1.2346 1 0\n"
        "\nVERTICES 4 8\n1 0\n1 1\n1 2\n1 3\n"
        "\nPOLYGONS 2 8\n3 0 2 1\n3 2 3 1\n";
    ASSERT_TRUE(dfa::io::vtkMeshString(m) == want);
    ASSERT_TRUE(dfa::convertToIndexedMesh({}, {}).polygons.empty());
    // the same triangles as the soup's mesh, vertex for vertex
    std::vector<PointXYZ> soup;
    for (int i : idx) soup.push_back(v[(size_t)i]);
    const dfa::PolygonMesh ms = dfa::convertToMesh(soup);
    ASSERT_EQ(ms.polygons.size(), m.polygons.size());
    for (size_t t = 0; t < m.polygons.size(); ++t)
        for (int k = 0; k < 3; ++k) {
            const PointXYZ &a = ms.cloud.points[ms.polygons[t][k]], &b = m.cloud.points[m.polygons[t][k]];
            ASSERT_TRUE(a.x == b.x && a.y == b.y && a.z == b.z);
        }
}

TEST(IndexedMeshTest, VtkTextOfAnExtractedMeshParsesBackToTheSameTriangles) {
    Scene s;
    cuda::MarchingCubes mc;
    const HostMesh h = indexed(mc, s.cvol());
    const dfa::PolygonMesh mesh = dfa::convertToIndexedMesh(h.vertices, h.indices);
    ASSERT_EQ(mesh.cloud.points.size(), h.vertices.size());
    std::istringstream in(dfa::io::vtkMeshString(mesh));
    std::string word;
    size_t np = 0, npoly = 0, nints = 0;
    while (in >> word && word != "POINTS") {}
    in >> np >> word;
    ASSERT_EQ(np, h.vertices.size());
    double worst = 0;
    for (size_t i = 0; i < np; ++i) {
        double x, y, z;
        in >> x >> y >> z;
        worst = std::max({worst, std::fabs(x - h.vertices[i].x), std::fabs(y - h.vertices[i].y), std::fabs(z - h.vertices[i].z)});
    }
    ASSERT_TRUE(worst < 5e-4);  // 5 significant digits of coordinates below 3 m
    while (in >> word && word != "POLYGONS") {}
    in >> npoly >> nints;
    ASSERT_EQ(npoly, h.indices.size() / 3);
    ASSERT_EQ(nints, 4 * npoly);
    for (size_t t = 0; t < npoly; ++t) {
        int n, a, b, c;
        in >> n >> a >> b >> c;
        ASSERT_TRUE(n == 3 && a == h.indices[3 * t] && b == h.indices[3 * t + 2] && c == h.indices[3 * t + 1]);
    }
}

int main(int argc, char** argv) { return mt::run_all(argc, argv); }
