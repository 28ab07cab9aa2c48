// kfusion/cuda/tsdf_volume.hpp — kfusion::cuda::TsdfVolume: the public interface of the reference's class
// (include/kfusion/cuda/tsdf_volume.hpp:7-73; behaviour src/kfusion/tsdf_volume.cpp:18-129) on the dynfu_amd C ABI.
//
// Layout of this adaptor: the volume's settings live in one plain struct, trivial accessors are inline, the
// operations that touch the GPU (clear / integrate / integrateWarped / raycast / fetchCloud / fetchNormals) are one dfa_tsdf_*
// call each.
// Not provided: get,setGridOrigin (not on the DynFusion path).
#pragma once
#include <algorithm>
#include <memory>

#include <kfusion/types.hpp>

struct dfa_knn_field;  // include/dynfu_amd.h

namespace kfusion {
namespace cuda {

class TsdfVolume {
    struct Settings {
        Vec3i dims;
        Vec3f size          = Vec3f::all(3.f);      // metres            (tsdf_volume.cpp:22)
        Affine3f pose       = Affine3f::Identity(); // volume -> world   (:23)
        float trunc         = 0.03f;                // metres            (:19), clamped by setTruncDist
        int max_weight      = 128;                  //                   (:20)
        float ray_step      = 0.75f;                // in truncation distances (:25)
        float grad_delta    = 0.75f;                // in voxels         (:24)
    } cfg_;
    CudaData blob_;  // X*Y*Z packed voxels {fp16 tsdf, u16 weight}
    // Occupancy map of the volume (dynfu_amd.h: dfa_tsdf_occupancy_bytes): which boxes of 32 x 2 x 8 voxels the sweeps of THIS
    // object may have left a weight in — kept by clear / integrate / clearAndIntegrate, read by cuda::MarchingCubes::run
    // instead of the empty voxels.  The map is only trusted while THIS object is the sole owner of the voxels and of the
    // map: CudaData handles and copies of a TsdfVolume share storage (ref-counted, as the reference's DeviceMemory), so a
    // writable data() handle, a swap, a copy of the object (either side may write afterwards) or a sweep run while another
    // handle is alive all make it unknown until the next clear / fused sweep by a sole owner.
    CudaData occ_;
    // The colour volume (dynfu_amd.h: dfa_tsdf_integrate_warped6_color), when createColors() has made one: X*Y*Z words
    // {b, g, r, 8-bit weight} in the voxels' order, zeroed.  Copies of the object share it, as they share the voxels.
    CudaData colors_;
    mutable bool occ_known_ = false;  // (mutable: copying a volume makes the SOURCE's map unknown too)
    // The k-NN field of the volume (dynfu_amd.h: dfa_knn_field_*), when one has been built: the neighbour rows of the voxels,
    // which integrateWarped / integrateWarped6 read instead of searching while the field matches their call.  What it was
    // created for is kept beside the handle; copies of the object share it (it depends on the geometry, not on the voxels).
    struct KnnFieldState {
        std::shared_ptr<dfa_knn_field> handle;
        Vec3i dims;
        Vec3f voxel;
        int k = 0;
        bool has_frame = false;
        float vol2node[12] = {};
    } field_;
    // the field when it serves a call with this k, node count and frame (vol2node: null for integrateWarped), else null
    const dfa_knn_field* matchingField(int k, int D, const float* vol2node) const;
    bool soleOwner() const { return blob_.unique() && occ_.unique(); }
    bool mapTrusted() const { return occ_known_ && soleOwner(); }

public:
    // --- construction / storage -----------------------------------------------------------------------------
    explicit TsdfVolume(const Vec3i& dims) { cfg_.dims = dims, create(dims); }
    TsdfVolume(const TsdfVolume& o) : cfg_(o.cfg_), blob_(o.blob_), occ_(o.occ_), colors_(o.colors_), field_(o.field_) { o.occ_known_ = false; }
    TsdfVolume& operator=(const TsdfVolume& o) {
        if (this != &o) cfg_ = o.cfg_, blob_ = o.blob_, occ_ = o.occ_, colors_ = o.colors_, field_ = o.field_, occ_known_ = false, o.occ_known_ = false;
        return *this;
    }
    virtual ~TsdfVolume() {}
    void create(const Vec3i& dims);            // allocates and clears
    void swap(CudaData& data) { blob_.swap(data), occ_known_ = false; }
    CudaData data() { return occ_known_ = false, blob_; }
    const CudaData data() const { return blob_; }
    // the occupancy map of the voxels (device) or nullptr when the voxels may have been written from outside this object
    const unsigned char* occupancy() const { return mapTrusted() ? occ_.ptr<unsigned char>() : nullptr; }

    // --- the GPU work -----------------------------------------------------------------------------------------
    virtual void clear();
    virtual void integrate(const Dists& dists, const Affine3f& camera_pose, const Intr& intr);
    // clear() then integrate() as ONE sweep (what DynFusion::operator() does every frame, dyn_fusion.cpp:113-116):
    // same voxels bit for bit, half the HBM traffic.  Extension of the reference's interface.
    void clearAndIntegrate(const Dists& dists, const Affine3f& camera_pose, const Intr& intr);
    // integrate() with every voxel taken through a warp field first (dfa_tsdf_integrate_warped: non-rigid fusion into a
    // canonical volume).  The nodes are plain device arrays in the volume's metric frame — D x 3 positions, D x 8 transforms,
    // D radii, as Warpfield::deviceNodes() hands them out — and not a Warpfield: this header is the kfusion layer, which the
    // dynfu layer is built on.  A voxel no node supports is left alone (Skip) or integrated where it stands (Rigid).  The
    // occupancy map is kept as integrate() keeps it.  Extension of the reference's interface.
    enum class UnsupportedMode { Skip = 0, Rigid = 1 };
    void integrateWarped(const Dists& dists, const Affine3f& camera_pose, const Intr& intr, const float* node_pos,
                         const float* node_dq, const float* node_w, int D, int k, UnsupportedMode mode = UnsupportedMode::Skip);
    // ... through a NORTH-STAR warp field (dfa_tsdf_integrate_warped6: the 6-DoF blend of the dfa_solver6 plans).  Its nodes
    // live in a frame of their own — node_frame_pose is the pose of that frame in the world; for DynFusion's north-star mode
    // the camera of frame 0 —: a voxel goes there by node_frame_pose^-1 * pose, is searched, supported and blended there, and
    // goes on to the camera by camera_pose^-1 * node_frame_pose.  k is 1..8.  The map is kept as integrateWarped keeps it.
    void integrateWarped6(const Dists& dists, const Affine3f& camera_pose, const Intr& intr, const Affine3f& node_frame_pose,
                          const float* node_pos, const float* node_dq, const float* node_w, int D, int k,
                          UnsupportedMode mode = UnsupportedMode::Skip);
    // Colour (dfa_tsdf_integrate_warped6_color, dfa_color_sample).  createColors: a zeroed colour volume of the volume's
    // dimensions, owned by the object (a second call zeroes it again); colors(): its words on the device, nullptr without one.
    // integrateWarped6Color: integrateWarped6 — the same voxels and map, bit for bit, the k-NN field used exactly when
    // integrateWarped6 would use it — that also fuses `image` (b, g, r, x pixels registered to dists) into the colour volume
    // in the same sweep, weights capped at max_color_weight (1..255); update_tsdf = false: colours only, no voxel and no
    // byte of the map is touched.  sampleColors: b, g, r, a per vertex (N vertices of `stride` floats, 3 or 4, on the
    // device, in the frame whose pose in the world is frame_pose), a = 0 where the volume holds no colour around it.
    // lattice_offset, in voxels per axis: how far the vertices stand off the lattice the sweeps integrate on.  The sweeps take
    // voxel i at i * voxel, marching cubes puts the vertex of a lattice edge at (i + 0.5 + t) * voxel (both as the reference
    // does), so the vertices of MarchingCubes::run / runIndexed take 0.5: the sample then lies ON the vertex's lattice edge,
    // between the two voxels it was interpolated from — of which the one behind the surface always has a colour —, not half
    // a voxel diagonal away among voxels that may be clamped or unseen.  0 for points that are where the surface is.
    void createColors();
    const unsigned int* colors() const { return colors_.empty() ? nullptr : colors_.ptr<unsigned int>(); }
    void integrateWarped6Color(const Dists& dists, const Image& image, const Affine3f& camera_pose, const Intr& intr,
                               const Affine3f& node_frame_pose, const float* node_pos, const float* node_dq, const float* node_w, int D,
                               int k, UnsupportedMode mode = UnsupportedMode::Skip, bool update_tsdf = true, int max_color_weight = 255);
    dfa::DeviceArray<RGB> sampleColors(const float* vertices, int N, int stride, const Affine3f& frame_pose, float lattice_offset = 0.f) const;
    // The k-NN field (dfa_knn_field_*): the neighbours of every voxel near a node searched once — buildKnnField — and brought
    // up to date when nodes have been appended — appendKnnField: the arrays hold the old nodes, unchanged, followed by the new
    // ones —, so that integrateWarped / integrateWarped6 with the same k, node count and (integrateWarped6: node_frame_pose
    // given here) frame run without their search: the same voxels and map, bit for bit.  A call the field does not match
    // searches as before.  max_bytes bounds the rows (0: no cap); a build or append that would exceed it drops the field and
    // returns false.  The field belongs to the volume's dimensions, size and pose as they are now.  Extension of the
    // reference's interface.
    bool buildKnnField(const float* node_pos, const float* node_w, int D, int k, const Affine3f* node_frame_pose = nullptr,
                       size_t max_bytes = 0);
    bool appendKnnField(const float* node_pos, const float* node_w, int D_new);
    void dropKnnField() { field_ = KnnFieldState(); }
    const dfa_knn_field* knnField() const { return field_.handle.get(); }
    int knnFieldNodes() const;  // the node count of the field's rows (0 without a field)
    int knnFieldK() const { return field_.handle ? field_.k : 0; }  // ... and the ids per row it was built with
    // the voxels of another volume of the same dimensions, copied (a copy of the OBJECT shares them); the map comes along
    // when the source's is trusted.  Extension of the reference's interface.
    void copyVoxelsFrom(const TsdfVolume& src);
    virtual void raycast(const Affine3f& camera_pose, const Intr& intr, Depth& depth, Normals& normals);
    virtual void raycast(const Affine3f& camera_pose, const Intr& intr, Cloud& points, Normals& normals);
    // the rays of raycast(points) shaded in the same launch (dfa_tsdf_raycast_render; KinFu::renderImage(image, pose, flag)):
    // `image` must hold rows x cols pixels, rows x 2 cols for DFA_RENDER_BOTH.  Extension of the reference's interface.
    void raycastRender(const Affine3f& camera_pose, const Intr& intr, int cols, int rows, const Vec3f& light_pose, int mode,
                       Image& image) const;
    virtual void applyAffine(const Affine3f& affine) { cfg_.pose = affine * cfg_.pose; }
    // the zero crossings on the voxel edges, in the world frame (pose), as float4 {x, y, z, 0} (tsdf_volume.hpp:49,
    // tsdf_volume.cpp:131-147): an empty buffer is created with 10 000 000 points; returns a non-owning array over the
    // first min(points, capacity) of them.  Unlike the reference the order is defined (ascending voxel index), nothing is
    // written past the buffer, and it reads only the boxes of the occupancy map that can hold a point when there is one.
    dfa::DeviceArray<Point> fetchCloud(dfa::DeviceArray<Point>& cloud_buffer) const;
    // normals of fetchCloud's points (tsdf_volume.hpp:50, tsdf_volume.cpp:149-160); NaN within 2 voxels of the border
    void fetchNormals(const dfa::DeviceArray<Point>& cloud, dfa::DeviceArray<Normal>& normals) const;

    // --- settings ---------------------------------------------------------------------------------------------
    Vec3i getDims() const { return cfg_.dims; }
    Vec3f getSize() const { return cfg_.size; }
    Vec3f getVoxelSize() const {
        return Vec3f(cfg_.size[0] / cfg_.dims[0], cfg_.size[1] / cfg_.dims[1], cfg_.size[2] / cfg_.dims[2]);
    }
    Affine3f getPose() const { return cfg_.pose; }
    float getTruncDist() const { return cfg_.trunc; }
    int getMaxWeight() const { return cfg_.max_weight; }
    float getRaycastStepFactor() const { return cfg_.ray_step; }
    float getGradientDeltaFactor() const { return cfg_.grad_delta; }

    void setPose(const Affine3f& pose) { cfg_.pose = pose; }
    void setMaxWeight(int weight) { cfg_.max_weight = weight; }
    void setRaycastStepFactor(float factor) { cfg_.ray_step = factor; }
    void setGradientDeltaFactor(float factor) { cfg_.grad_delta = factor; }
    // never below 2.1 voxel edges (tsdf_volume.cpp:57-61); re-applied when the size changes (:47-50)
    void setTruncDist(float distance) {
        const Vec3f v = getVoxelSize();
        cfg_.trunc    = std::max(distance, 2.1f * std::max(std::max(v[0], v[1]), v[2]));
    }
    void setSize(const Vec3f& size) { cfg_.size = size, setTruncDist(cfg_.trunc); }

    // the packed voxel (tsdf_volume.hpp:53-62); the reference's two converters throw "Not implemented"
    struct Entry {
        typedef unsigned short half;
        half tsdf;
        unsigned short weight;
        static half float2half(float value);
        static float half2float(half value);
    };
};

}  // namespace cuda
}  // namespace kfusion
