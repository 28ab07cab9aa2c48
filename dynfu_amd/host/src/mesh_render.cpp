// mesh_render.cpp — kfusion::cuda::rasterizeMesh on dfa_mesh_rasterize.
#include <kfusion/cuda/mesh_render.hpp>

#include "../../../include/dynfu_amd.h"

namespace kfusion {
namespace cuda {

void rasterizeMesh(const dfa::DeviceArray<dfa::PointXYZ>& vertices, const dfa::DeviceArray<dfa::Normal>& normals,
                   const dfa::DeviceArray<int>& indices, const Affine3f& world2cam, const Intr& intr, int cols, int rows,
                   float z_near, Cloud& points, Normals& normals_out, dfa::DeviceArray<uint64_t>& zbuffer) {
    if (!normals.empty() && normals.size() < vertices.size())
        throw dfa::Error(DFA_ERR_INVALID, "rasterizeMesh: fewer normals than vertices");
    points.create(rows, cols);
    normals_out.create(rows, cols);
    if (cols > 0 && rows > 0 && zbuffer.size() != (size_t)rows * cols) zbuffer.create((size_t)rows * cols);
    float aff[12];
    world2cam.to12(aff);
    dfa::check(dfa_mesh_rasterize((const float*)vertices.ptr(), normals.empty() ? nullptr : (const float*)normals.ptr(),
                                  (int)vertices.size(), indices.ptr(), (int)(indices.size() / 3), aff, intr.fx, intr.fy, intr.cx,
                                  intr.cy, z_near, cols, rows, zbuffer.ptr(), (float*)points.ptr(), (int)points.step(),
                                  (float*)normals_out.ptr(), (int)normals_out.step(), nullptr),
               "rasterizeMesh");
}

}  // namespace cuda
}  // namespace kfusion
