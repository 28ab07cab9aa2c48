// rigid_step.hpp — one pose update of the rigid Gauss-Newton (kfusion::cuda::icp_update, host/include/kfusion/cuda/
// icp_update.hpp) and the rules of the loop around it, as host/device code: no HIP runtime call, plain g++ compiles it
// (tests/cpp/test_rigid_step.cpp drives it on the CPU), and one lane of rigid_loop_step_kernel (icp.hip) runs it on the
// device.  The step, exactly as the host states it:
//   the 27 float sums (A's upper triangle with b, row by row) -> symmetric A and b in double;
//   a pivoted LU in double, in icp_solve6's pivot order, gives the determinant and the twist x = (rvec, tvec);
//   the update is REFUSED when the factorisation fails, when |det| < 1e-15 or when det is NaN;
//   the Rodrigues matrix of rvec in double, rounded to float (icp_from_rvec); pose <- exp(x) pose in float
//   (Affine3f::operator*).
// It also returns |rvec| and |tvec| in double.
//
// The rules of the loop (dfa_rigid_align_cloud; rigid_loop_advance below is their only statement):
//   levels run in the order given, level l at most level_iters[l] iterations, every iteration linearises at the pose reached;
//   a refused update: status = singular, every later launch returns at entry, the reported pose is aff0;
//   an accepted update with |rvec| < stop_rot and |tvec| < stop_trans finishes the CURRENT level: its remaining launches
//   return at entry, the next level starts from the pose reached.  Thresholds of 0 never stop the loop (the compare is
//   strict; a NaN norm does not stop it either).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DFA_HD __host__ __device__
#define DFA_UNROLL _Pragma("unroll")
#else
#define DFA_HD
#define DFA_UNROLL
#endif

#pragma GCC visibility push(hidden)  // internal to the library: nothing here joins its exported symbols
namespace dfa {

constexpr int RIGID_MAX_LEVELS = 4;   // = the length of dfa_rigid_align_report.iters_run
constexpr int RIGID_MAX_ITERS  = 64;  // iterations of one call, all levels together

// icp_solve6: pivoted LU of a 6x6 system in double -> determinant and solution; false (det = 0) at a zero pivot column.
// The same operations in the same order; every loop has constant bounds and every index is one, the row exchange a chain
// of guarded swaps, so that on the device the matrix lives in registers (a row picked by a computed index puts it in
// scratch memory, a round trip per access for the one lane that runs this).
DFA_HD inline bool rigid_solve6(const double A_in[36], const double b_in[6], double x[6], double& det) {
    double A[36], b[6];
    DFA_UNROLL for (int i = 0; i < 36; ++i) A[i] = A_in[i];
    DFA_UNROLL for (int i = 0; i < 6; ++i) b[i] = b_in[i];
    det = 1.0;
    DFA_UNROLL for (int c = 0; c < 6; ++c) {
        int piv     = c;
        double best = fabs(A[6 * c + c]);  // |A[piv][c]|
        DFA_UNROLL for (int r = c + 1; r < 6; ++r) {
            const double v = fabs(A[6 * r + c]);
            if (v > best) best = v, piv = r;
        }
        if (best == 0.0) {
            det = 0.0;
            return false;
        }
        DFA_UNROLL for (int r = c + 1; r < 6; ++r)
            if (piv == r) {
                DFA_UNROLL for (int j = 0; j < 6; ++j) {
                    const double t = A[6 * c + j];
                    A[6 * c + j] = A[6 * r + j], A[6 * r + j] = t;
                }
                const double t = b[c];
                b[c] = b[r], b[r] = t;
                det = -det;
            }
        det *= A[6 * c + c];
        DFA_UNROLL for (int r = c + 1; r < 6; ++r) {
            const double f = A[6 * r + c] / A[6 * c + c];
            DFA_UNROLL for (int j = c; j < 6; ++j) A[6 * r + j] -= f * A[6 * c + j];
            b[r] -= f * b[c];
        }
    }
    DFA_UNROLL for (int r = 5; r >= 0; --r) {
        double s = b[r];
        DFA_UNROLL for (int j = r + 1; j < 6; ++j) s -= A[6 * r + j] * x[j];
        x[r] = s / A[6 * r + r];
    }
    return true;
}

// icp_from_rvec: Rodrigues rotation vector -> matrix, formed in double and rounded to float (the identity below 2^-52)
DFA_HD inline void rigid_rodrigues(const double r[3], float R[9]) {
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    R[0] = 1.f, R[1] = 0.f, R[2] = 0.f, R[3] = 0.f, R[4] = 1.f, R[5] = 0.f, R[6] = 0.f, R[7] = 0.f, R[8] = 1.f;
    if (th > 2.220446049250313e-16) {
        const double c = cos(th), s = sin(th), c1 = 1.0 - c, k[3] = {r[0] / th, r[1] / th, r[2] / th};
        const double M[9] = {c + c1 * k[0] * k[0],        c1 * k[0] * k[1] - s * k[2], c1 * k[0] * k[2] + s * k[1],
                             c1 * k[0] * k[1] + s * k[2], c + c1 * k[1] * k[1],        c1 * k[1] * k[2] - s * k[0],
                             c1 * k[0] * k[2] - s * k[1], c1 * k[1] * k[2] + s * k[0], c + c1 * k[2] * k[2]};
        for (int i = 0; i < 9; ++i) R[i] = (float)M[i];
    }
}

struct RigidStep {
    bool ok;            // false: refused, the pose untouched
    double rot, trans;  // |rvec|, |tvec| of the twist (0 when refused)
};

// icp_update on 12 floats (R row-major, then t): aff <- exp(x) aff
DFA_HD inline RigidStep rigid_step(const float sums[27], float aff[12]) {
    double A[36], b[6], x[6], det;
    int shift = 0;
    DFA_UNROLL for (int i = 0; i < 6; ++i)
        DFA_UNROLL for (int j = i; j < 7; ++j) {
            const double v = sums[shift++];
            if (j == 6) b[i] = v;
            else A[6 * j + i] = A[6 * i + j] = v;
        }
    const bool solved = rigid_solve6(A, b, x, det);
    if (!solved || fabs(det) < 1e-15 || det != det) return RigidStep{false, 0.0, 0.0};
    float R[9], out[12];
    rigid_rodrigues(x, R);
    const float t[3] = {(float)x[3], (float)x[4], (float)x[5]};
    for (int i = 0; i < 3; ++i) {  // Affine3f::operator*, float, in its order
        for (int j = 0; j < 3; ++j) out[3 * i + j] = R[3 * i] * aff[j] + R[3 * i + 1] * aff[3 + j] + R[3 * i + 2] * aff[6 + j];
        out[9 + i] = R[3 * i] * aff[9] + R[3 * i + 1] * aff[10] + R[3 * i + 2] * aff[11] + t[i];
    }
    for (int i = 0; i < 12; ++i) aff[i] = out[i];
    return RigidStep{true, sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]), sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])};
}

// What a call of dfa_rigid_align_cloud keeps on the device between its launches: zeroed by ONE memset at the start of the
// call (so the pose starts as "aff0", not as twelve zeros: have_pose), then written by the step launches only — but for
// matched[], where the row launch of iteration g adds its workgroups' counts into slot g.
struct RigidLoopState {
    float aff[12];  // the pose reached, once have_pose
    int have_pose;  // 0: no update was accepted yet, the pose is the call's aff0
    int status;     // 0 ok, 1 singular system
    int finished[RIGID_MAX_LEVELS];   // the stopping rule ended this level
    int iters_run[RIGID_MAX_LEVELS];  // accepted or refused iterations per level
    int last_iter;                    // the last iteration that ran (index over all levels)
    float last_rot, last_trans;       // the last accepted twist's norms
    unsigned int matched[RIGID_MAX_ITERS];  // per iteration, over all levels
};

// does a launch of `level` still have work?  (both kernels return at entry when not)
DFA_HD inline bool rigid_loop_active(const RigidLoopState& st, int level) { return st.status == 0 && st.finished[level] == 0; }

// the pose iteration linearises at
DFA_HD inline void rigid_loop_pose(const RigidLoopState& st, const float aff0[12], float aff[12]) {
    for (int i = 0; i < 12; ++i) aff[i] = st.have_pose ? st.aff[i] : aff0[i];
}

// The step of iteration `iter` (of `level`) behind its 27 sums: the update and the rules above.  Only for an active launch.
DFA_HD inline void rigid_loop_advance(RigidLoopState& st, const float aff0[12], int level, int iter, const float sums[27],
                                      float stop_rot, float stop_trans) {
    float aff[12];
    rigid_loop_pose(st, aff0, aff);
    st.iters_run[level] += 1;
    st.last_iter = iter;
    const RigidStep r = rigid_step(sums, aff);
    if (!r.ok) {
        st.status = 1;
        return;
    }
    for (int i = 0; i < 12; ++i) st.aff[i] = aff[i];
    st.have_pose  = 1;
    st.last_rot   = (float)r.rot;
    st.last_trans = (float)r.trans;
    if (r.rot < (double)stop_rot && r.trans < (double)stop_trans) st.finished[level] = 1;
}

}  // namespace dfa
#pragma GCC visibility pop
