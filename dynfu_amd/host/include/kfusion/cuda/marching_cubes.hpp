// kfusion/cuda/marching_cubes.hpp — kfusion::cuda::MarchingCubes (reference interface:
// include/kfusion/cuda/marching_cubes.hpp:19-60; behaviour: src/kfusion/marching_cubes.cpp:12-61) on
// dfa_marching_cubes / dfa_marching_cubes_indexed.
//
// What differs from the reference, all visible here:
//   * any volume dimensions (the reference's kernels are fixed to 128^3);
//   * vertices come out in ascending linear voxel order (the reference's order depends on atomics);
//   * ONE host synchronisation per run() — to size the returned array — instead of three;
//   * the case tables are a constructor argument: none = the library's derived tables
//     (dfa_mc_default_tables), or the reference's `triTable` / `numVertsTable`
//     (src/kfusion/marching_cubes.cpp:86-354) for meshes identical to the reference's.
#pragma once
#include <kfusion/cuda/tsdf_volume.hpp>
#include <kfusion/types.hpp>

namespace kfusion {
namespace cuda {

class MarchingCubes {
    dfa::DeviceArray<int> tri_dev_, nverts_dev_, total_dev_, totals_dev_;  // 256 x 16, 256, 1, 2 (runIndexed)
    int last_total_ = 0, last_unique_ = 0;
    void uploadTables(const int* tri, const int* nverts);

public:
    typedef dfa::PointXYZ PointType;  // 16 bytes {x, y, z, 1}, the layout of pcl::PointXYZ
    enum { POINTS_PER_TRIANGLE = 3, DEFAULT_TRIANGLES_BUFFER_SIZE = 2 * 1000 * 1000 * POINTS_PER_TRIANGLE };

    MarchingCubes();
    MarchingCubes(const int* triTable /* 256 x 16, -1 padded */, const int* numVertsTable /* 256 */);
    ~MarchingCubes();

    // Extracts the zero level set into `triangles_buffer` (allocated at DEFAULT_TRIANGLES_BUFFER_SIZE when empty,
    // marching_cubes.cpp:23-25) and returns a NON-owning array over the vertices written: three per triangle.
    dfa::DeviceArray<PointType> run(const TsdfVolume& volume, dfa::DeviceArray<PointType>& triangles_buffer);

    // vertices the last run() found; larger than the buffer means only the buffer's worth was written
    int totalVertices() const { return last_total_; }

    // Extension (no counterpart in the reference): the same surface as an indexed mesh, dfa_marching_cubes_indexed — every
    // crossed lattice edge once in `vertex_buffer`, and in `index_buffer` one vertex id per vertex of run()'s soup, in its
    // order.  Empty buffers are allocated at DEFAULT_TRIANGLES_BUFFER_SIZE indices and a third as many vertices.  Returns
    // NON-owning views of what was written; when the mesh does not fit one of the buffers BOTH views are empty and
    // totalUniqueVertices() / totalVertices() say what the buffers need.  Uses the volume's occupancy map when it is
    // trusted.  ONE host synchronisation, to size the views.
    // min_weight other than 1: dfa_marching_cubes_indexed_min_weight — a voxel counts as observed from that weight on (the
    // extraction for a volume that accumulates frames: what one frame touched once stays out at 2).
    struct IndexedMesh {
        dfa::DeviceArray<PointType> vertices;
        dfa::DeviceArray<int> indices;
    };
    IndexedMesh runIndexed(const TsdfVolume& volume, dfa::DeviceArray<PointType>& vertex_buffer,
                           dfa::DeviceArray<int>& index_buffer, int min_weight = 1);

    // distinct vertices the last runIndexed() found (totalVertices(): the indices = run()'s vertices)
    int totalUniqueVertices() const { return last_unique_; }

    // Normals of vertices from the gradient of the TSDF — ANY array of points in the volume's metric frame: run()'s soup or
    // runIndexed()'s distinct vertices (a fifth of the work for the same surface) — the raycaster's compute_normal,
    // tsdf_volume.cu:320-336, with the volume's gradient delta factor.  Extension: the reference leaves the mesh
    // without normals (dyn_fusion.cpp:80-88 "temporary workaround until normals are computed via mc").
    void computeNormals(const TsdfVolume& volume, const dfa::DeviceArray<PointType>& vertices,
                        dfa::DeviceArray<dfa::Normal>& normals);
};

}  // namespace cuda
}  // namespace kfusion
