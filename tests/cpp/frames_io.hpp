// frames_io.hpp — what the two frame-dump programs share (test_host_northstar_frames.cpp, test_host_dynfusion_frames.cpp): the
// parameter file of a case, and raw files of frames in and of arrays out.
//
// params.txt: `key value ...` per line, keys as the members of KinFuParams / DynFuParams / NorthStarParameters (and frames,
// nodeStep, warp_knn); an unknown key is an error.  The reference-mode file (Keys::Reference) takes four keys more:
// fuse_canonical, and solver_numIter / solver_nonLinearIter / solver_linearIter, the budgets of DynFusion::solverParams (the
// plain numIter and linearIter are NorthStarParameters' in both files).
#pragma once
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <istream>
#include <sstream>
#include <string>
#include <vector>

#include <dynfu/dyn_fusion.hpp>

namespace frames_io {
enum class Keys { NorthStar, Reference };

// what a case sets: DynFuParams, and the public knobs beside it
struct Case {
    DynFuParams p = DynFuParams::defaultParams();
    int frames    = 0;
    int nodeStep  = 128;
    int warp_knn  = KNN;  // Warpfield::setKnn, once frame 0 has created the field
    // Keys::Reference: numIter, nonLinearIter and linearIter of DynFusion::solverParams (the constructor's values here)
    int solver_numIter = 24, solver_nonLinearIter = 16, solver_linearIter = 256;
};

inline std::string g9(float v) {  // nine significant digits carry a float32 exactly
    char buf[32];
    std::snprintf(buf, sizeof buf, "%.9g", v);
    return buf;
}

inline void read_ints(std::istream& in, std::vector<int>& v) {
    int n = 0;
    in >> n;
    if (n < 0 || n > 64) throw dfa::Error(1, "params: bad list length");
    v.assign((size_t)n, 0);
    for (int& x : v) in >> x;
}
inline std::string ints(const std::vector<int>& v) {
    std::string s = std::to_string(v.size());
    for (int x : v) s += " " + std::to_string(x);
    return s;
}

inline Case parse_params(std::istream& in, Keys keys = Keys::NorthStar) {
    using namespace kfusion;
    Case c;
    KinFuParams& k          = c.p.kinfuParams;
    DynFuParams& d          = c.p;
    NorthStarParameters& ns = c.p.northStarParams;
    const bool ref          = keys == Keys::Reference;
    std::string key;
    while (in >> key) {
        if (key == "cols") in >> k.cols;
        else if (key == "rows") in >> k.rows;
        else if (key == "intr") in >> k.intr.fx >> k.intr.fy >> k.intr.cx >> k.intr.cy;
        else if (key == "volume_dims") in >> k.volume_dims[0] >> k.volume_dims[1] >> k.volume_dims[2];
        else if (key == "volume_size") in >> k.volume_size[0] >> k.volume_size[1] >> k.volume_size[2];
        else if (key == "volume_pose") {
            for (float& v : k.volume_pose.R) in >> v;
            for (float& v : k.volume_pose.t) in >> v;
        } else if (key == "bilateral") in >> k.bilateral_sigma_depth >> k.bilateral_sigma_spatial >> k.bilateral_kernel_size;
        else if (key == "icp_truncate_depth_dist") in >> k.icp_truncate_depth_dist;
        else if (key == "tsdf_trunc_dist") in >> k.tsdf_trunc_dist;
        else if (key == "tsdf_max_weight") in >> k.tsdf_max_weight;
        else if (key == "gradient_delta_factor") in >> k.gradient_delta_factor;
        else if (key == "tukeyOffset") in >> d.tukeyOffset;
        else if (key == "lambda") in >> d.lambda;
        else if (key == "psi_data") in >> d.psi_data;
        else if (key == "psi_reg") in >> d.psi_reg;
        else if (key == "L") in >> d.L;
        else if (key == "beta") in >> d.beta;
        else if (key == "epsilon") in >> d.epsilon;
        else if (key == "mesh_normals") in >> d.mesh_normals;
        else if (key == "north_star") in >> d.north_star;
        else if (key == "model_view") in >> d.model_view;
        else if (key == "north_star_fuse_canonical") in >> d.north_star_fuse_canonical;
        else if (key == "north_star_fuse_color") in >> d.north_star_fuse_color;
        else if (key == "canonical_max_color_weight") in >> d.canonical_max_color_weight;
        else if (key == "fuse_knn_field") in >> d.fuse_knn_field;
        else if (key == "north_star_visible_only") in >> d.north_star_visible_only;
        else if (key == "fuse_unsupported_rigid") in >> d.fuse_unsupported_rigid;
        else if (key == "north_star_regrow_canonical") in >> d.north_star_regrow_canonical;
        else if (key == "canonical_min_weight") in >> d.canonical_min_weight;
        else if (key == "north_star_rigid_prealign") in >> d.north_star_rigid_prealign;
        else if (key == "rigid_prealign_iters") in >> d.rigid_prealign_iters;
        else if (key == "rigid_prealign_device") in >> d.rigid_prealign_device;
        else if (key == "rigid_prealign_steps") read_ints(in, d.rigid_prealign_steps);
        else if (key == "rigid_prealign_level_iters") read_ints(in, d.rigid_prealign_level_iters);
        else if (key == "rigid_prealign_stop") in >> d.rigid_prealign_stop_rot >> d.rigid_prealign_stop_trans;
        else if (key == "north_star_reg_hierarchy") in >> d.north_star_reg_hierarchy;
        else if (key == "reg_level_slots") read_ints(in, d.reg_level_slots);
        else if (key == "numIter") in >> ns.numIter;
        else if (key == "gnIter") in >> ns.gnIter;
        else if (key == "linearIter") in >> ns.linearIter;
        else if (key == "distThresh") in >> ns.distThresh;
        else if (key == "cosThresh") in >> ns.cosThresh;
        else if (key == "damping") in >> ns.damping;
        else if (key == "gnTol") in >> ns.gnTol;
        else if (key == "frames") in >> c.frames;
        else if (key == "nodeStep") in >> c.nodeStep;
        else if (key == "warp_knn") in >> c.warp_knn;
        else if (ref && key == "fuse_canonical") in >> d.fuse_canonical;
        else if (ref && key == "solver_numIter") in >> c.solver_numIter;
        else if (ref && key == "solver_nonLinearIter") in >> c.solver_nonLinearIter;
        else if (ref && key == "solver_linearIter") in >> c.solver_linearIter;
        else throw dfa::Error(1, "params: unknown key " + key);
        if (!in) throw dfa::Error(1, "params: bad value of " + key);
    }
    d.intr = k.intr;
    return c;
}

inline std::string format_params(const Case& c, Keys keys = Keys::NorthStar) {
    using namespace kfusion;
    const KinFuParams& k          = c.p.kinfuParams;
    const DynFuParams& d          = c.p;
    const NorthStarParameters& ns = c.p.northStarParams;
    std::ostringstream o;
    o << "cols " << k.cols << "\nrows " << k.rows << "\nintr " << g9(k.intr.fx) << " " << g9(k.intr.fy) << " " << g9(k.intr.cx) << " "
      << g9(k.intr.cy) << "\nvolume_dims " << k.volume_dims[0] << " " << k.volume_dims[1] << " " << k.volume_dims[2] << "\nvolume_size "
      << g9(k.volume_size[0]) << " " << g9(k.volume_size[1]) << " " << g9(k.volume_size[2]) << "\nvolume_pose";
    for (float v : k.volume_pose.R) o << " " << g9(v);
    for (float v : k.volume_pose.t) o << " " << g9(v);
    o << "\nbilateral " << g9(k.bilateral_sigma_depth) << " " << g9(k.bilateral_sigma_spatial) << " " << k.bilateral_kernel_size
      << "\nicp_truncate_depth_dist " << g9(k.icp_truncate_depth_dist) << "\ntsdf_trunc_dist " << g9(k.tsdf_trunc_dist)
      << "\ntsdf_max_weight " << k.tsdf_max_weight << "\ngradient_delta_factor " << g9(k.gradient_delta_factor) << "\ntukeyOffset "
      << g9(d.tukeyOffset) << "\nlambda " << g9(d.lambda) << "\npsi_data " << g9(d.psi_data) << "\npsi_reg " << g9(d.psi_reg) << "\nL " << d.L
      << "\nbeta " << d.beta << "\nepsilon " << g9(d.epsilon) << "\nmesh_normals " << d.mesh_normals << "\nnorth_star " << d.north_star
      << "\nmodel_view " << d.model_view << "\nnorth_star_fuse_canonical " << d.north_star_fuse_canonical << "\nnorth_star_fuse_color "
      << d.north_star_fuse_color << "\ncanonical_max_color_weight " << d.canonical_max_color_weight << "\nfuse_knn_field " << d.fuse_knn_field
      << "\nnorth_star_visible_only " << d.north_star_visible_only << "\nfuse_unsupported_rigid " << d.fuse_unsupported_rigid
      << "\nnorth_star_regrow_canonical " << d.north_star_regrow_canonical << "\ncanonical_min_weight " << d.canonical_min_weight
      << "\nnorth_star_rigid_prealign " << d.north_star_rigid_prealign << "\nrigid_prealign_iters " << d.rigid_prealign_iters
      << "\nrigid_prealign_device " << d.rigid_prealign_device << "\nrigid_prealign_steps " << ints(d.rigid_prealign_steps)
      << "\nrigid_prealign_level_iters " << ints(d.rigid_prealign_level_iters) << "\nrigid_prealign_stop " << g9(d.rigid_prealign_stop_rot)
      << " " << g9(d.rigid_prealign_stop_trans) << "\nnorth_star_reg_hierarchy " << d.north_star_reg_hierarchy << "\nreg_level_slots "
      << ints(d.reg_level_slots) << "\nnumIter " << ns.numIter << "\ngnIter " << ns.gnIter << "\nlinearIter " << ns.linearIter
      << "\ndistThresh " << g9(ns.distThresh) << "\ncosThresh " << g9(ns.cosThresh) << "\ndamping " << g9(ns.damping) << "\ngnTol "
      << g9(ns.gnTol) << "\nframes " << c.frames << "\nnodeStep " << c.nodeStep << "\nwarp_knn " << c.warp_knn << "\n";
    if (keys == Keys::Reference)
        o << "fuse_canonical " << d.fuse_canonical << "\nsolver_numIter " << c.solver_numIter << "\nsolver_nonLinearIter "
          << c.solver_nonLinearIter << "\nsolver_linearIter " << c.solver_linearIter << "\n";
    return o.str();
}

// a raw frame file of exactly n elements
template <class T>
std::vector<T> read_frame(const std::string& path, size_t n) {
    std::vector<T> px(n);
    std::ifstream f(path, std::ios::binary);
    if (!f) throw dfa::Error(1, "no frame file " + path);
    f.read((char*)px.data(), (std::streamsize)(n * sizeof(T)));
    if (!f || f.peek() != std::ifstream::traits_type::eof()) throw dfa::Error(1, "frame file " + path + " has the wrong size");
    return px;
}

template <class T>
void write_raw(const std::string& path, const T* data, size_t n) {
    std::ofstream f(path, std::ios::binary);
    if (n) f.write((const char*)data, (std::streamsize)(n * sizeof(T)));
    if (!f) throw dfa::Error(1, "dump: cannot write " + path);
}
template <class T>
void write_image(const std::string& path, const dfa::DeviceArray2D<T>& img) {
    std::vector<T> host;
    int cols = 0;
    if (!img.empty()) img.download(host, cols);
    write_raw(path, host.data(), host.size());
}
template <class T>
void write_array(const std::string& path, const dfa::DeviceArray<T>& a) {
    std::vector<T> host;
    if (a.size()) a.download(host);
    write_raw(path, host.data(), host.size());
}
inline void write_frame_cloud(const std::string& prefix, const std::shared_ptr<dynfu::Frame>& frame) {
    dfa::DeviceArray<float> v3, n3;
    size_t n = 0;
    if (frame && frame->size()) frame->deviceArrays(v3, n3), n = frame->size();
    std::vector<float> v, nn;
    if (n) v3.download(v), n3.download(nn);
    write_raw(prefix + "_v.bin", v.data(), std::min(v.size(), 3 * n));
    write_raw(prefix + "_n.bin", nn.data(), std::min(nn.size(), 3 * n));
}
}  // namespace frames_io
