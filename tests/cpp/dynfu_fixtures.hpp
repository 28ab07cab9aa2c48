// dynfu_fixtures.hpp — what the test_host_*.cpp programs that drive a DynFusion share: the helpers whose bodies were the same
// in every copy.  Scenes and predicates that differ from file to file stay in their files.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include <dynfu/dyn_fusion.hpp>
#include <kfusion/cuda/tsdf_volume.hpp>

#include "../../include/dynfu_amd.h"

namespace dynfu_fixtures {

// a DynFusion cannot be constructed from `p`: DynFuParams::validate refuses it as an invalid argument
inline bool construction_throws(const DynFuParams& p) {
    try {
        DynFusion df(p);
    } catch (const dfa::Error& e) {
        return e.code == DFA_ERR_INVALID;
    }
    return false;
}

// the same bits; two empty vectors are the same
template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// a volume's voxels on the host
inline std::vector<uint32_t> voxels(const kfusion::cuda::TsdfVolume& vol) {
    const kfusion::Vec3i dims = vol.getDims();
    std::vector<uint32_t> h((size_t)dims[0] * dims[1] * dims[2]);
    vol.data().download(h.data(), h.size() * sizeof(uint32_t));
    return h;
}

// the cloud getCanonicalWarpedToLive() holds (packed N x 3), the node transforms (D x 8), and the identity's bits
inline std::vector<float> warped_vertices(DynFusion& df) {
    std::vector<float> v;
    dfa::DeviceArray<float> v3, n3;
    df.getCanonicalWarpedToLive()->deviceArrays(v3, n3);
    if (df.getCanonicalWarpedToLive()->size()) v3.download(v);
    return v;
}
inline std::vector<float> node_transforms(DynFusion& df) {
    std::vector<float> pos, w, dq;
    df.getWarpfield()->hostArrays(pos, w, dq);
    return dq;
}
inline bool is_identity(const dfa::Affine3f& a) {
    const dfa::Affine3f i;
    return std::memcmp(a.R, i.R, sizeof a.R) == 0 && std::memcmp(a.t, i.t, sizeof a.t) == 0;
}

// The sphere scene: 160 x 120 pixels, a sphere of radius 0.5 m at `cz` metres and nothing behind it — a third of the view is
// surface, the rest has no depth.  left_only: no depth right of the image centre either.
namespace sphere_scene {
const int W = 160, H = 120;
const float F = 131.25f;

inline std::vector<unsigned short> sphere_depth(float cz, bool left_only = false) {
    std::vector<unsigned short> d((size_t)W * H);
    const float cx = W / 2 - 0.5f, cy = H / 2 - 0.5f, R = 0.5f;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float dir[3] = {(x - cx) / F, (y - cy) / F, 1.f};
            const float n = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + 1.f);
            for (float& v : dir) v /= n;
            const float b = dir[2] * cz, disc = b * b - (cz * cz - R * R);
            float z = 0.f;
            if (disc > 0) z = (b - std::sqrt(disc)) * dir[2];
            if (left_only && x >= W / 2) z = 0.f;
            d[(size_t)y * W + x] = (unsigned short)std::lround(z * 1000.f);
        }
    return d;
}
}  // namespace sphere_scene

// The planted-motion scene: four frames of two spheres before a tilted wall, the camera moved by the same motion every frame.
namespace planted_motion_scene {
// test_host_icp.cpp's image.  The volume is the smallest cube that holds the scene: 2.2 m from z = 1 m — the spheres reach
// from x = -0.85 to 0.7 and from z = 1.15, the wall crosses the cube between z = 2.01 and 3.19 — at 256 voxels a side.  The
// voxel size matters to the rigid tests' translation bar: the integration takes voxel i at i * voxel, marching cubes puts its vertices
// at (i + 0.5) * voxel (both as the reference does), so the canonical model stands half a voxel, 4.3 mm, off the scene it
// was fused from, along every axis.  The rigid estimate maps the MODEL into the live camera, offset included: 4.3 of the
// 5 mm of the translation bar are that offset (measured: 4.1, 4.5, 4.3 mm; at 128 voxels a side and 3 m it is 11.7 mm).
const int W = 320, H = 240, DIM = 256;
const float F = 262.5f, VOLUME = 2.2f, VOLUME_Z0 = 1.0f;

// test_host_icp.cpp's scene: depth of two spheres in front of a tilted wall seen from camera pose X_world = R X_cam + t
inline std::vector<unsigned short> render(const float R[9], const float t[3]) {
    std::vector<unsigned short> d((size_t)W * H, 0);
    const float cx = W / 2 - 0.5f, cy = H / 2 - 0.5f;
    const float C[2][3] = {{0.25f, -0.1f, 1.6f}, {-0.55f, 0.3f, 2.0f}}, rad[2] = {0.45f, 0.3f};
    const float pn[3] = {0.3f, 0.2f, -0.933f}, pd = -2.6f * 0.933f;  // wall: pn . X = pd
    for (int y = 3; y < H - 3; ++y)
        for (int x = 3; x < W - 3; ++x) {
            const float dc[3] = {(x - cx) / F, (y - cy) / F, 1.f};
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
            if (best < 1e8f && best < 60.f) d[(size_t)y * W + x] = (unsigned short)std::lround(best * 1000.f);
        }
    return d;
}

// the planted motion of test_host_icp.cpp: 1.2 degrees about y, (15, -8, 10) mm: X_before = M X_after
inline dfa::Affine3f motion() {
    const float a = 0.021f;
    dfa::Affine3f m;
    const float R[9] = {std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)};
    for (int i = 0; i < 9; ++i) m.R[i] = R[i];
    m.t[0] = 0.015f, m.t[1] = -0.008f, m.t[2] = 0.010f;
    return m;
}

struct Depths {
    kfusion::cuda::Depth d[4], empty;
    Depths() {
        dfa::Affine3f pose;  // frame f's camera: X_world = M^f X_cam
        for (int f = 0; f < 4; ++f) {
            d[f].upload(render(pose.R, pose.t), W);
            pose = pose * motion();
        }
        empty.upload(std::vector<unsigned short>((size_t)W * H, 0), W);
    }
};
}  // namespace planted_motion_scene

}  // namespace dynfu_fixtures
