// kfusion/cuda/icp_update.hpp — the host step of one rigid-ICP iteration (reference: src/kfusion/projective_icp.cpp:39-57
// StreamHelper::get, :136-152 determinant test, solve and pose update), on its own so that a test can reach it with
// known sums.  OpenCV is not available to this build: a pivoted LU in double stands in for cv::determinant +
// cv::solve(DECOMP_SVD), the Rodrigues formula for cv::Affine3f(rvec, t).
#pragma once
#include <cmath>
#include <utility>

#include <kfusion/types.hpp>

namespace kfusion {
namespace cuda {

namespace detail {
// pivoted LU of a 6x6 system in double: determinant and solution (the reference: cv::determinant, then
// cv::solve(..., DECOMP_SVD) — for the non-singular systems that pass its determinant test the same solution)
inline bool icp_solve6(const double A_in[36], const double b_in[6], double x[6], double& det) {
    double A[36], b[6];
    for (int i = 0; i < 36; ++i) A[i] = A_in[i];
    for (int i = 0; i < 6; ++i) b[i] = b_in[i];
    det = 1.0;
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (std::fabs(A[6 * r + c]) > std::fabs(A[6 * piv + c])) piv = r;
        if (A[6 * piv + c] == 0.0) {
            det = 0.0;
            return false;
        }
        if (piv != c) {
            for (int j = 0; j < 6; ++j) std::swap(A[6 * c + j], A[6 * piv + j]);
            std::swap(b[c], b[piv]);
            det = -det;
        }
        det *= A[6 * c + c];
        for (int r = c + 1; r < 6; ++r) {
            const double f = A[6 * r + c] / A[6 * c + c];
            for (int j = c; j < 6; ++j) A[6 * r + j] -= f * A[6 * c + j];
            b[r] -= f * b[c];
        }
    }
    for (int r = 5; r >= 0; --r) {
        double s = b[r];
        for (int j = r + 1; j < 6; ++j) s -= A[6 * r + j] * x[j];
        x[r] = s / A[6 * r + r];
    }
    return true;
}

// cv::Affine3f(rvec, t): Rodrigues rotation vector -> matrix
inline Affine3f icp_from_rvec(const double r[3], const double t[3]) {
    Affine3f a;
    const double th = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (th > 2.220446049250313e-16) {
        const double c = std::cos(th), s = std::sin(th), c1 = 1.0 - c, k[3] = {r[0] / th, r[1] / th, r[2] / th};
        const double R[9] = {c + c1 * k[0] * k[0],        c1 * k[0] * k[1] - s * k[2], c1 * k[0] * k[2] + s * k[1],
                             c1 * k[0] * k[1] + s * k[2], c + c1 * k[1] * k[1],        c1 * k[1] * k[2] - s * k[0],
                             c1 * k[0] * k[2] - s * k[1], c1 * k[1] * k[2] + s * k[0], c + c1 * k[2] * k[2]};
        for (int i = 0; i < 9; ++i) a.R[i] = (float)R[i];
    }
    for (int i = 0; i < 3; ++i) a.t[i] = (float)t[i];
    return a;
}

}  // namespace detail

// The 27 sums of one linearisation (A's upper triangle with b, row by row) -> the next pose.  false, and the affine
// untouched, when the system is singular: |det A| < 1e-15 or a NaN determinant (:136-147).
inline bool icp_update(const float sums[27], Affine3f& affine) {
    double A[36], b[6], x[6], det;
    int shift = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 7; ++j) {
            const double v = sums[shift++];
            if (j == 6) b[i] = v;
            else A[6 * j + i] = A[6 * i + j] = v;
        }
    const bool ok = detail::icp_solve6(A, b, x, det);
    if (!ok || std::fabs(det) < 1e-15 || std::isnan(det)) return false;  // :136-142
    affine = detail::icp_from_rvec(x, x + 3) * affine;                            // :144-147
    return true;
}

}  // namespace cuda
}  // namespace kfusion
