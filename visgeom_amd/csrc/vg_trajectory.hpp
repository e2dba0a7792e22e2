// vg_trajectory.hpp -- calibration trajectory planning: TrajectoryVisualQuality::EvaluateCost
// (src/calibration/trajectory_generation.cpp:146-281) with CircularTrajectory::compute (test/calibration/trajectory.cpp:27-82) on
// the SE(3) and camera functions of vg_geometry.hpp / vg_camera.hpp.  Three launches evaluate the cost at n parameter points,
// whatever n is:
//   trajectory_prepass_kernel   one lane per (point, trajectory): the serial part -- the poses xi_i = xi_{i-1} o dxi and the
//                               covariance recurrence cov <- L cov L^T + covIncr -- written once per pose;
//   trajectory_pose_kernel      one wave per (point, pose i >= 1): lanes run over the board's corners (looping when there are
//                               more than 64), the 21 + 21 sums of JtJ and JtCJ and the image-limit penalty are reduced by a
//                               butterfly of fixed order, lane 0 does the 6 x 6 algebra and writes J^T C^-1 J, the four
//                               penalties and the pose's validity;
//   trajectory_finish_kernel    one lane per point: H = prior + the contributions added trajectory-major and step-ascending,
//                               the penalties in the same order, -log det H from a Cholesky factor.
// No atomics; a point's result depends on nothing but its own parameters.  The same per-pose function serves
// trajectory_visual_cov_kernel (one wave per camera pose).  Evaluated in the order written (-ffp-contract=off);
// tests/trajectory_ref.py restates it.  DESIGN.md section 5.20, deviations section 9.
#pragma once

#include <cstdint>

#include "vg_camera.hpp"

namespace vgt {

constexpr int kP = 5;              // parameters of one trajectory: x0, y0, theta0, d, alpha
constexpr int kMaxTraj = 8;
constexpr int kMinSteps = 2, kMaxSteps = 256;
constexpr int kMaxCorners = 1024;
constexpr int kWave = 64;
constexpr int kTerms = 5;          // information, image limits, curvature, distance, normal
constexpr int kTri = 21;           // upper triangle of a 6 x 6
constexpr double kCovAbs = 1e-2, kCovVW = 1e-4;   // covAbs, covVW (trajectory.cpp:42, :51)
constexpr double kDiffEps = 1e-8;  // DIFF_EPS

struct Setup {
    int model;
    double cam[10];
    double width, height;
    double xi_cam[6], xi_board[6];
    double L_cam[36];              // xi_cam.screwTransfInv()
    double hess_prior[6];          // 1 / prior_variance
    double kappa_max, min_dist, margin, min_cell, stiffness, step;
    int nx, ny, T;
    int steps[kMaxTraj];
    int pose0[kMaxTraj + 1];       // first pose of trajectory t among all poses of a point (pose 0 included)
    int slot0[kMaxTraj + 1];       // first pose i >= 1 of trajectory t among the evaluated poses of a point
};

// ---- 6-vector transformations (transformation.h:80-99) and 6 x 6 helpers, row-major

VG_HD vg::Quat quat_of(const double *rot)
{
    const vg::RotTrig g = vg::rot_trig(rot, false, true);
    return vg::quat_from_rotvec(rot, g);
}

VG_HD void compose(const double *a, const double *b, double *out)
{
    const vg::Quat q1 = quat_of(a + 3), q2 = quat_of(b + 3);
    double rt[3];
    vg::quat_rotate(q1, b, rt);
    for (int i = 0; i < 3; i++) out[i] = rt[i] + a[i];
    vg::quat_to_rotvec(vg::quat_mul(q1, q2), out + 3);
}

VG_HD void inverse_compose(const double *a, const double *b, double *out)
{
    const vg::Quat q1 = quat_of(a + 3), q2 = quat_of(b + 3);
    const vg::Quat q1inv = {-q1.x, -q1.y, -q1.z, q1.w};
    const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    vg::quat_rotate(q1inv, d, out);
    vg::quat_to_rotvec(vg::quat_mul(q1inv, q2), out + 3);
}

VG_HD void rot_mat(const double *rot, double sign, double *R)
{
    const vg::RotTrig g = vg::rot_trig(rot, true, false);
    vg::rotation_matrix(rot, sign, g, R);
}

// Transformation::screwTransfInv (transformation.h:234-243): [R^-1, -R^-1 hat(t); 0, R^-1]
VG_HD void screw_transf_inv(const double *xi, double *L)
{
    double R[9], RH[9];
    rot_mat(xi + 3, -1., R);
    const double H[9] = {0, -xi[2], xi[1], xi[2], 0, -xi[0], -xi[1], xi[0], 0};
    vg::mat3_mul(R, H, RH);
#pragma unroll
    for (int k = 0; k < 36; k++) L[k] = 0.;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            L[6 * r + q] = R[3 * r + q];
            L[6 * r + 3 + q] = -RH[3 * r + q];
            L[6 * (3 + r) + 3 + q] = R[3 * r + q];
        }
}

VG_HD void mat6_mul(const double *A, const double *B, double *C)   // C = A B
{
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int q = 0; q < 6; q++) {
            double v = 0.;
#pragma unroll
            for (int k = 0; k < 6; k++) v += A[6 * r + k] * B[6 * k + q];
            C[6 * r + q] = v;
        }
}

VG_HD void mat6_mul_bt(const double *A, const double *B, double *C)   // C = A B^T
{
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int q = 0; q < 6; q++) {
            double v = 0.;
#pragma unroll
            for (int k = 0; k < 6; k++) v += A[6 * r + k] * B[6 * q + k];
            C[6 * r + q] = v;
        }
}

VG_HD void mat6_mul_at(const double *A, const double *B, double *C)   // C = A^T B
{
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int q = 0; q < 6; q++) {
            double v = 0.;
#pragma unroll
            for (int k = 0; k < 6; k++) v += A[6 * k + r] * B[6 * k + q];
            C[6 * r + q] = v;
        }
}

// the lower Cholesky factor of a symmetric 6 x 6 (its lower triangle is read); false when a pivot is not positive
VG_HD bool chol6(const double *A, double *L)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 36; k++) L[k] = 0.;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = A[6 * j + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[6 * j + k] * L[6 * j + k];
        ok = ok && d > 0.;   // false for a NaN
        const double l = sqrt(d);
        L[6 * j + j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = A[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = v / l;
        }
    }
    return ok;
}

VG_HD bool finite36(const double *A)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 36; k++) ok = ok && isfinite(A[k]);
    return ok;
}

// the inverse of a symmetric positive definite 6 x 6 from its Cholesky factor: A^-1 = L^-T L^-1, symmetric by construction.
// false when A has no factor or the inverse is not finite.
VG_HD bool spd6_inverse(const double *A, double *Ainv)
{
    double L[36], Li[36];
    bool ok = chol6(A, L);
#pragma unroll
    for (int k = 0; k < 36; k++) Li[k] = 0.;
#pragma unroll
    for (int j = 0; j < 6; j++) {   // column j of L^-1 by forward substitution
        Li[6 * j + j] = 1. / L[6 * j + j];
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = 0.;
#pragma unroll
            for (int k = j; k < i; k++) v -= L[6 * i + k] * Li[6 * k + j];
            Li[6 * i + j] = v / L[6 * i + i];
        }
    }
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int q = r; q < 6; q++) {
            double v = 0.;
#pragma unroll
            for (int k = q; k < 6; k++) v += Li[6 * k + r] * Li[6 * k + q];
            Ainv[6 * r + q] = v;
            Ainv[6 * q + r] = v;
        }
    return ok && finite36(Ainv);
}

// ---- CircularTrajectory::compute, one step at a time (the prepass kernel and vg_trajectory_poses run the same code)

struct TrajectoryWalk {
    double xi[6], dxi[6], L[36], cov_incr[36], cov_odom[36];
};

// pose 0 and what every step needs: xi0, dxi, L = dxi.screwTransfInv(), covIncr = dxidu covVW dxidu^T, covOdom = covIncr
VG_HD void walk_start(const double *p, TrajectoryWalk &w)
{
    const double dist = p[3], alpha = p[4];
    double sa, ca;
    vg::sincos_(alpha * 0.5, &sa, &ca);
    const double xi0[6] = {p[0], p[1], 0., 0., 0., p[2]};
    const double dxi[6] = {-dist * sa, dist * ca, 0., 0., 0., alpha};
    for (int k = 0; k < 6; k++) {
        w.xi[k] = xi0[k];
        w.dxi[k] = dxi[k];
    }
    const double J[12] = {-sa, -dist / 2 * ca, ca, -dist / 2 * sa, 0., 0., 0., 0., 0., 0., 0., 1.};   // dxidu, 6 x 2
    for (int r = 0; r < 6; r++)
        for (int q = 0; q < 6; q++) w.cov_incr[6 * r + q] = (J[2 * r] * kCovVW) * J[2 * q] + (J[2 * r + 1] * kCovVW) * J[2 * q + 1];
    for (int k = 0; k < 36; k++) w.cov_odom[k] = w.cov_incr[k];
    screw_transf_inv(w.dxi, w.L);
}

// the covariance of the pose the walk stands at: covAbs at pose 0, covOdom + covAbs afterwards
VG_HD void walk_cov(const TrajectoryWalk &w, bool first, double *cov)
{
    for (int k = 0; k < 36; k++) cov[k] = first ? (k % 7 == 0 ? kCovAbs : 0.) : w.cov_odom[k] + (k % 7 == 0 ? kCovAbs : 0.);
}

VG_HD void walk_step(TrajectoryWalk &w)
{
    double next[6], T1[36], T2[36];
    compose(w.xi, w.dxi, next);
    for (int k = 0; k < 6; k++) w.xi[k] = next[k];
    mat6_mul(w.L, w.cov_odom, T1);
    mat6_mul_bt(T1, w.L, T2);
    for (int k = 0; k < 36; k++) w.cov_odom[k] = T2[k] + w.cov_incr[k];
}

// ---- the penalties that do not need the corners

// curvatureCost (:274-281)
VG_HD double curvature_cost(const Setup &s, const double *xi1, const double *xi2)
{
    double zeta[6];
    inverse_compose(xi1, xi2, zeta);
    const double v = vg::norm3(zeta), w = vg::norm3(zeta + 3);
    const double kapa = w / v;
    const double e = fmax(0., kapa - s.kappa_max) * 10;
    return e * e;
}

// distanceCost (:208-212) on xiCamBoard
VG_HD double distance_cost(const Setup &s, const double *xcb)
{
    const double e = fmax(s.min_dist - vg::norm3(xcb), 0.);
    return e * e;
}

// normalCost (:214-223) on xiCamBoard and its rotation matrix; the norm of a cross product against pi / 6, as written
VG_HD double normal_cost(const double *xcb, const double *R)
{
    const double ez[3] = {R[2], R[5], R[8]};
    const double nrm = vg::norm3(xcb);
    const double d[3] = {xcb[0] / nrm, xcb[1] / nrm, xcb[2] / nrm};
    const double c[3] = {d[1] * ez[2] - d[2] * ez[1], d[2] * ez[0] - d[0] * ez[2], d[0] * ez[1] - d[1] * ez[0]};
    const double e = fmax(vg::norm3(c) - M_PI / 6, 0.) * 10;
    return e * e;
}

struct EvalArgs {
    Setup s;
    int64_t n;
    int PT, n_poses, n_slots;
    const double *params;          // DEVICE [n][PT]
    double *xi;                    // [n][n_poses][6]
    double *cov;                   // [n][n_poses][36]
    double *contrib;               // [n][n_slots][36]
    double *pen;                   // [n][n_slots][4]
    int32_t *bad;                  // [n][n_slots]
    double *cost;                  // [n]
    double *terms;                 // [n][kTerms]
    int32_t *invalid;              // [n]
};

struct CovArgs {
    Setup s;
    int64_t n;
    const double *poses;           // DEVICE [n][6]
    double *cov, *info;            // [n][36]
    int32_t *invalid;              // [n]
};

__global__ __launch_bounds__(kWave) void trajectory_prepass_kernel(EvalArgs a)
{
    const int64_t item = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (item >= a.n * a.s.T) return;
    const int64_t point = item / a.s.T;
    const int t = (int)(item % a.s.T);
    TrajectoryWalk w;
    walk_start(a.params + point * a.PT + kP * t, w);
    double *xi = a.xi + (point * a.n_poses + a.s.pose0[t]) * 6;
    double *cov = a.cov + (point * a.n_poses + a.s.pose0[t]) * 36;
    double c[36];
    for (int i = 0; i < a.s.steps[t]; i++) {
        if (i > 0) walk_step(w);
        walk_cov(w, i == 0, c);
        for (int k = 0; k < 6; k++) xi[6 * i + k] = w.xi[k];
        for (int k = 0; k < 36; k++) cov[36 * i + k] = c[k];
    }
}

// a sum over the wave in a fixed order, the same in every lane afterwards
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// What visualCov (:185-206) and imageLimitsCost (:226-272) take from the corners, for the camera pose cam_pose, by one wave.
// On return, in every lane: JtJ and JtCJ (6 x 6, mirrored from their upper triangles), the image-limit penalty, the number of
// corners that did not project; xcb = xiCamBoard and R its rotation matrix.  uv: LDS [2 N], the projections.
template <int MODEL>
__device__ __forceinline__ void corner_sums(const Setup &s, const double *cam_pose, double *uv, double *JtJ, double *JtCJ, double &limits,
                                            int &failed, double *xcb, double *R)
{
    const int lane = threadIdx.x;
    const int N = s.nx * s.ny;
    inverse_compose(cam_pose, s.xi_board, xcb);
    rot_mat(xcb + 3, 1., R);
    double a[kTri], c[kTri];
#pragma unroll
    for (int k = 0; k < kTri; k++) a[k] = c[k] = 0.;
    double lim = 0.;
    int bad = 0;
    const double cu = s.cam[vg::CameraTraits<MODEL>::kFocal + 2], cv = s.cam[vg::CameraTraits<MODEL>::kFocal + 3];
    const double radius = (cu + cv) / 2.;
    for (int k = lane; k < N; k += kWave) {
        const double bx = s.step * (k % s.nx), by = s.step * (k / s.nx);
        const double X0 = R[0] * bx + R[1] * by + xcb[0], X1 = R[3] * bx + R[4] * by + xcb[1], X2 = R[6] * bx + R[7] * by + xcb[2];
        vg::CornerEval<vg::CameraTraits<MODEL>::K> e;
        vg::eval_corner<MODEL, true, false>(s.cam, X0, X1, X2, e);
        uv[2 * k] = e.u;
        uv[2 * k + 1] = e.v;
        if (!e.ok) {
            bad++;
            continue;
        }
        // dpdxi = dpdx [-I | hat(X)]
        double r0[6], r1[6];
        const double *P = e.P;
        r0[0] = -P[0], r0[1] = -P[1], r0[2] = -P[2];
        r0[3] = P[1] * X2 - P[2] * X1, r0[4] = P[2] * X0 - P[0] * X2, r0[5] = P[0] * X1 - P[1] * X0;
        r1[0] = -P[3], r1[1] = -P[4], r1[2] = -P[5];
        r1[3] = P[4] * X2 - P[5] * X1, r1[4] = P[5] * X0 - P[3] * X2, r1[5] = P[3] * X1 - P[4] * X0;
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p; q < 6; q++, idx++) {
                a[idx] += r0[p] * r0[q] + r1[p] * r1[q];
                c[idx] += (r0[p] * s.stiffness) * r0[q] + (r1[p] * s.stiffness) * r1[q];
            }
        const double dx = fmax(s.margin - fmin(e.u, s.width - e.u), 0.), dy = fmax(s.margin - fmin(e.v, s.height - e.v), 0.);
        const double du = e.u - cu, dv = e.v - cv;
        const double dr = fmax(sqrt(du * du + dv * dv) - radius, 0.);
        const double m = fmax(dx, fmax(dy, dr)) / 10.;
        lim += m * m;
    }
    __syncthreads();   // one wave: the projections are in LDS for the neighbours' lanes
    const int nh = (s.nx - 1) * s.ny, nv = s.nx * (s.ny - 1);
    for (int k = lane; k < nh + nv; k += kWave) {
        int i0, i1;
        if (k < nh) {   // the horizontal cell size, i outer and j inner as in the reference
            const int i = k / s.ny, j = k % s.ny;
            i0 = s.nx * j + i, i1 = i0 + 1;
        } else {        // the vertical cell size
            const int kk = k - nh, i = kk / (s.ny - 1), j = kk % (s.ny - 1);
            i0 = s.nx * j + i, i1 = i0 + s.nx;
        }
        const double du = uv[2 * i0] - uv[2 * i1], dv = uv[2 * i0 + 1] - uv[2 * i1 + 1];
        const double m = fmax(s.min_cell - sqrt(du * du + dv * dv), 0.) / 10.;
        lim += m * m;
    }
    failed = (int)wave_sum((double)bad);
    limits = wave_sum(lim);
    int idx = 0;
#pragma unroll
    for (int p = 0; p < 6; p++)
#pragma unroll
        for (int q = p; q < 6; q++, idx++) {
            const double sa = wave_sum(a[idx]), sc = wave_sum(c[idx]);
            JtJ[6 * p + q] = JtJ[6 * q + p] = sa;
            JtCJ[6 * p + q] = JtCJ[6 * q + p] = sc;
        }
}

// visualCov's tail: JtCJ^-T JtJ JtCJ^-1; false when JtCJ has no finite inverse
__device__ __forceinline__ bool visual_cov(const double *JtJ, const double *JtCJ, double *V)
{
    double W[36], T[36];
    const bool ok = spd6_inverse(JtCJ, W);
    mat6_mul_at(W, JtJ, T);
    mat6_mul(T, W, V);
    return ok && finite36(V);
}

template <int MODEL>
__global__ __launch_bounds__(kWave) void trajectory_pose_kernel(EvalArgs a)
{
    extern __shared__ double uv[];
    const Setup &s = a.s;
    const int slot = blockIdx.x;
    const int64_t point = blockIdx.y;
    int t = 0;
    while (t + 1 < s.T && slot >= s.slot0[t + 1]) t++;
    const int i = slot - s.slot0[t] + 1;
    const double *xi0 = a.xi + (point * a.n_poses + s.pose0[t]) * 6, *xi = xi0 + 6 * i;
    double cam_pose[6], xcb[6], R[9], JtJ[36], JtCJ[36], limits;
    int failed;
    compose(xi, s.xi_cam, cam_pose);   // xiOrigCam
    corner_sums<MODEL>(s, cam_pose, uv, JtJ, JtCJ, limits, failed, xcb, R);
    if (threadIdx.x != 0) return;
    double V[36], C[36], Cinv[36], T1[36], T2[36];
    bool ok = failed == 0 && visual_cov(JtJ, JtCJ, V);
    const double *cov = a.cov + (point * a.n_poses + s.pose0[t] + i) * 36;
    mat6_mul(s.L_cam, cov, T1);
    mat6_mul_bt(T1, s.L_cam, T2);
    for (int k = 0; k < 36; k++) C[k] = V[k] + T2[k];
    ok = spd6_inverse(C, Cinv) && ok;
    double rel[6], vis[6], J[36];
    inverse_compose(xi0, cam_pose, rel);
    inverse_compose(s.xi_cam, rel, vis);   // xiVis
    screw_transf_inv(vis, J);
    for (int k = 0; k < 6; k++) J[7 * k] -= 1.;
    mat6_mul_at(J, Cinv, T1);
    mat6_mul(T1, J, T2);
    ok = ok && finite36(T2);
    const double four[4] = {limits, curvature_cost(s, xi - 6, xi), distance_cost(s, xcb), normal_cost(xcb, R)};
    for (int k = 0; k < 4; k++) ok = ok && isfinite(four[k]);
    const int64_t o = point * a.n_slots + slot;
    for (int k = 0; k < 36; k++) a.contrib[o * 36 + k] = ok ? T2[k] : 0.;
    for (int k = 0; k < 4; k++) a.pen[o * 4 + k] = ok ? four[k] : 0.;
    a.bad[o] = ok ? 0 : 1;
}

__global__ __launch_bounds__(kWave) void trajectory_finish_kernel(EvalArgs a)
{
    const int64_t point = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (point >= a.n) return;
    double H[36], L[36];
    for (int k = 0; k < 36; k++) H[k] = k % 7 == 0 ? a.s.hess_prior[k / 7] : 0.;
    double res = 0., pen[4] = {0., 0., 0., 0.};
    int invalid = 0;
    for (int slot = 0; slot < a.n_slots; slot++) {   // trajectory-major, step-ascending
        const int64_t o = point * a.n_slots + slot;
        if (a.bad[o]) {
            invalid++;
            continue;
        }
        for (int k = 0; k < 36; k++) H[k] += a.contrib[o * 36 + k];
        for (int k = 0; k < 4; k++) {
            res += a.pen[o * 4 + k];
            pen[k] += a.pen[o * 4 + k];
        }
    }
    double info = 0.;
    const bool ok = chol6(H, L) && invalid == 0;
    for (int k = 0; k < 6; k++) info -= 2. * log(L[7 * k]);   // -sum log sigma_k(H) = -log det H
    const double cost = res + info;
    const bool fin = ok && isfinite(cost);
    a.cost[point] = fin ? cost : HUGE_VAL;
    a.terms[point * kTerms] = fin ? info : HUGE_VAL;
    for (int k = 0; k < 4; k++) a.terms[point * kTerms + 1 + k] = pen[k];
    a.invalid[point] = invalid;
}

template <int MODEL>
__global__ __launch_bounds__(kWave) void trajectory_visual_cov_kernel(CovArgs a)
{
    extern __shared__ double uv[];
    const int64_t item = blockIdx.x;
    double xcb[6], R[9], JtJ[36], JtCJ[36], V[36], limits;
    int failed;
    corner_sums<MODEL>(a.s, a.poses + 6 * item, uv, JtJ, JtCJ, limits, failed, xcb, R);
    if (threadIdx.x != 0) return;
    const bool ok = failed == 0 && visual_cov(JtJ, JtCJ, V);
    for (int k = 0; k < 36; k++) {
        a.cov[item * 36 + k] = ok ? V[k] : HUGE_VAL;
        a.info[item * 36 + k] = ok ? JtJ[k] : HUGE_VAL;
    }
    a.invalid[item] = ok ? 0 : 1;
}

}  // namespace vgt
