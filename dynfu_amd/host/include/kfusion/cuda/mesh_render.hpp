// kfusion/cuda/mesh_render.hpp — the mesh rasteriser (dfa_mesh_rasterize) as a thin wrapper in the style of
// kfusion/cuda/imgproc.hpp: it creates its outputs when they do not have the right size and makes ONE C-ABI call on the
// default stream.  No counterpart in the reference, which can only raycast the volume: this is how a mesh that has been
// carried through the warp field (MarchingCubes::runIndexed -> Warpfield::warpToLive) becomes the point and normal maps of
// its visible surface — the layout of TsdfVolume::raycast's maps, NaN where nothing is seen, ready for cuda::renderImage /
// renderTangentColors.
#pragma once
#include <cstdint>

#include <kfusion/types.hpp>

namespace kfusion {
namespace cuda {

// vertices / normals: float4 per vertex (normals may be empty: face normals turned towards the camera); indices: three per
// triangle; world2cam: the frame of the vertices -> the camera.  zbuffer is the call's only scratch (rows * cols words) and
// holds (bits(depth) << 32) | triangle per pixel afterwards.
void rasterizeMesh(const dfa::DeviceArray<dfa::PointXYZ>& vertices, const dfa::DeviceArray<dfa::Normal>& normals,
                   const dfa::DeviceArray<int>& indices, const Affine3f& world2cam, const Intr& intr, int cols, int rows,
                   float z_near, Cloud& points, Normals& normals_out, dfa::DeviceArray<uint64_t>& zbuffer);

// dfa_visible_vertices: n vertices in the camera frame, `stride` floats apart (3: a dynfu::Frame's packed arrays, the
// north-star warp's output; 4: float4 clouds), against the point map of the model's visible surface — rasterizeMesh's or
// TsdfVolume::raycast's, NaN where nothing is seen.  flags (created at n bytes) gets 1 where the model does not lie in front
// of the vertex by more than z_tol, 0 elsewhere; count (optional, created at one int, stays on the device): the set flags.
void visibleVertices(const float* vertices, int stride, size_t n, const Cloud& model_points, const Intr& intr, float z_tol,
                     dfa::DeviceArray<unsigned char>& flags, dfa::DeviceArray<int>* count = nullptr);

}  // namespace cuda
}  // namespace kfusion
