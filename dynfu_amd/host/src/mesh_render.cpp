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

void visibleVertices(const float* vertices, int stride, size_t n, const Cloud& model_points, const Intr& intr, float z_tol,
                     dfa::DeviceArray<unsigned char>& flags, dfa::DeviceArray<int>* count) {
    if (n > 0x7fffffffu) throw dfa::Error(DFA_ERR_INVALID, "visibleVertices: more than 2^31 - 1 vertices");
    if (flags.size() != n) flags.create(n);
    if (count && count->size() != 1) count->create(1);
    dfa::check(dfa_visible_vertices(vertices, stride, (int)n, (const float*)model_points.ptr(), (int)model_points.step(),
                                    model_points.cols(), model_points.rows(), intr.fx, intr.fy, intr.cx, intr.cy, z_tol,
                                    flags.ptr(), count ? count->ptr() : nullptr, nullptr),
               "visibleVertices");
}

}  // namespace cuda
}  // namespace kfusion
