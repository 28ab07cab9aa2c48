// projective_icp.cpp — kfusion::cuda::ProjectiveICP on the dynfu_amd C ABI
// (reference: src/kfusion/projective_icp.cpp:62-200).
#include <kfusion/cuda/projective_icp.hpp>

#include <kfusion/cuda/icp_update.hpp>

#include "../../../include/dynfu_amd.h"

namespace kfusion {
namespace cuda {

ProjectiveICP::ProjectiveICP() : gate_angle_(20.f * 0.017453293f), gate_dist_(0.1f) {  // :62
    setIterationsNum({10, 5, 4, 0});                                                      // :63-65
    sums_.create(27);
}
ProjectiveICP::~ProjectiveICP() {}

void ProjectiveICP::setIterationsNum(const std::vector<int>& iters) {  // :82-89
    schedule_.assign(MAX_PYRAMID_LEVELS, 0);
    for (size_t i = 0; i < iters.size() && i < (size_t)MAX_PYRAMID_LEVELS; ++i) schedule_[i] = iters[i];
}

int ProjectiveICP::getUsedLevelsNum() const {  // :91-96
    int i = MAX_PYRAMID_LEVELS - 1;
    for (; i >= 0 && !schedule_[i]; --i) {
    }
    return i + 1;
}

bool ProjectiveICP::runLevel(Affine3f& affine, const Intr& intr, int level, bool depth_variant, const void* curr, int curr_step,
                            const float* ncurr, int ncurr_step, const void* prev, int prev_step, const float* nprev,
                            int nprev_step, int cols, int rows) {
    const int div = 1 << level;  // setLevelIntr, :15-20
    for (int iter = 0; iter < schedule_[level]; ++iter) {
        float aff[12];
        affine.to12(aff);
        dfa::check(dfa_icp_sums(depth_variant ? 1 : 0, curr, curr_step, ncurr, ncurr_step, prev, prev_step, nprev, nprev_step,
                                cols, rows, aff, intr.fx / div, intr.fy / div, intr.cx / div, intr.cy / div, gate_dist_,
                                gate_angle_, sums_.ptr(), nullptr, nullptr),
                   "ProjectiveICP::estimateTransform");
        std::vector<float> h;
        sums_.download(h);  // synchronises (StreamHelper::get, :39-57)
        if (!icp_update(h.data(), affine)) return false;  // :136-147
    }
    return true;
}

bool ProjectiveICP::estimateTransform(Affine3f& affine, const Intr& intr, const DepthPyr& dcurr, const NormalsPyr ncurr,
                                      const DepthPyr dprev, const NormalsPyr nprev) {
    affine = Affine3f::Identity();  // :124
    for (int level = getUsedLevelsNum() - 1; level >= 0; --level) {
        const Normals& n = nprev[level];
        if (!runLevel(affine, intr, level, true, dcurr[level].ptr(), (int)dcurr[level].step(), (const float*)ncurr[level].ptr(),
                     (int)ncurr[level].step(), dprev[level].ptr(), (int)dprev[level].step(), (const float*)n.ptr(),
                     (int)n.step(), n.cols(), n.rows()))
            return false;
    }
    return true;
}

bool ProjectiveICP::estimateTransform(Affine3f& affine, const Intr& intr, const PointsPyr& vcurr, const NormalsPyr ncurr,
                                      const PointsPyr vprev, const NormalsPyr nprev) {
    affine = Affine3f::Identity();  // :159
    for (int level = getUsedLevelsNum() - 1; level >= 0; --level) {
        const Normals& n = nprev[level];
        if (!runLevel(affine, intr, level, false, vcurr[level].ptr(), (int)vcurr[level].step(), (const float*)ncurr[level].ptr(),
                     (int)ncurr[level].step(), vprev[level].ptr(), (int)vprev[level].step(), (const float*)n.ptr(),
                     (int)n.step(), n.cols(), n.rows()))
            return false;
    }
    return true;
}

}  // namespace cuda
}  // namespace kfusion
