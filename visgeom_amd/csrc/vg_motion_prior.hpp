// vg_motion_prior.hpp -- OdometryPrior(errV, errW, lambdaT, lambdaR, xiOdom) of the localization costs
// (local_cost_functions.cpp:393-493), shared by the photometric solve (host loop) and the sparse odometry solve (in the
// kernel): the weighting A and the constant Jacobian J, both row-major 6 x 6, built on the host, and the block's
// contribution to the 28 sums [J^T J (21) | J^T r (6) | cost] of a pose.  (vg_odometry.hpp holds the calibration's block of
// the same name, which couples two poses and clamps its variances; this one does neither.)
#pragma once

#include <cmath>
#include <cstring>

#include "vg_geometry.hpp"
#include "vg_pose_host.hpp"

namespace vgmp {

struct MotionPrior {
    double A[36], J[36];
    vgth::Array6d xi;
};

inline MotionPrior make_prior(const double *xi_odom, double errV, double errW, double lambdaT, double lambdaR)
{
    MotionPrior p;
    std::memcpy(p.xi.data(), xi_odom, sizeof(double) * 6);
    const double delta = xi_odom[5], l = vg::norm3(xi_odom);
    const double s = std::sin(delta / 2.), c = std::cos(delta / 2.), l2 = l / 2.;
    const double dfdu[3][2] = {{c, l2 * s}, {-s, l2 * c}, {0., 1.}};
    const double Cu[2] = {errV * errV * l * l, errW * errW * delta * delta};
    const double lam[3] = {lambdaT * lambdaT, lambdaT * lambdaT, lambdaR * lambdaR};
    double Cx[9];
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) Cx[3 * r + q] = dfdu[r][0] * Cu[0] * dfdu[q][0] + dfdu[r][1] * Cu[1] * dfdu[q][1] + (r == q ? lam[r] : 0.);
    const double c00 = Cx[4] * Cx[8] - Cx[5] * Cx[7], c01 = Cx[5] * Cx[6] - Cx[3] * Cx[8], c02 = Cx[3] * Cx[7] - Cx[4] * Cx[6];
    const double id = 1. / (Cx[0] * c00 + Cx[1] * c01 + Cx[2] * c02);
    const double Ci[9] = {c00 * id, (Cx[2] * Cx[7] - Cx[1] * Cx[8]) * id, (Cx[1] * Cx[5] - Cx[2] * Cx[4]) * id,
                          c01 * id, (Cx[0] * Cx[8] - Cx[2] * Cx[6]) * id, (Cx[2] * Cx[3] - Cx[0] * Cx[5]) * id,
                          c02 * id, (Cx[1] * Cx[6] - Cx[0] * Cx[7]) * id, (Cx[0] * Cx[4] - Cx[1] * Cx[3]) * id};
    double L[9] = {0.};   // CxInv = L L^T; LLT::matrixU is L^T: U(i, j) = L[3 j + i]
    for (int r = 0; r < 3; r++)
        for (int q = 0; q <= r; q++) {
            double v = Ci[3 * r + q];
            for (int k = 0; k < q; k++) v -= L[3 * r + k] * L[3 * q + k];
            L[3 * r + q] = r == q ? std::sqrt(v) : v / L[3 * q + q];
        }
    for (int k = 0; k < 36; k++) p.A[k] = p.J[k] = 0.;
    p.A[6 * 1 + 1] = L[0];        // U(0, 0)
    p.A[6 * 0 + 0] = -L[4];       // -U(1, 1)
    p.A[6 * 0 + 1] = -L[3];       // -U(0, 1)
    p.A[6 * 0 + 5] = -L[7];       // -U(1, 2)
    p.A[6 * 1 + 5] = L[6];        // U(0, 2)
    p.A[6 * 2 + 2] = 1. / lambdaT;
    p.A[6 * 3 + 3] = 1. / lambdaR;
    p.A[6 * 4 + 4] = 1. / lambdaR;
    p.A[6 * 5 + 5] = L[8];        // U(2, 2)
    double R[9], M[9], RM[9], blk[9], out[9];
    const vg::RotTrig rt = vg::rot_trig(xi_odom + 3, true, true);
    vg::rotation_matrix(xi_odom + 3, -1., rt, R);
    vg::inter_omega_rot(xi_odom + 3, rt, M);
    vg::mat3_mul(R, M, RM);
    const int r0[3] = {0, 0, 3}, c0[3] = {0, 3, 3};   // J's blocks: top left A R, top right A R M, bottom right A R M
    for (int b = 0; b < 3; b++) {
        for (int r = 0; r < 3; r++)
            for (int q = 0; q < 3; q++) blk[3 * r + q] = p.A[6 * (r0[b] + r) + c0[b] + q];
        vg::mat3_mul(blk, b == 0 ? R : RM, out);
        for (int r = 0; r < 3; r++)
            for (int q = 0; q < 3; q++) p.J[6 * (r0[b] + r) + c0[b] + q] = out[3 * r + q];
    }
    return p;
}

// OdometryPrior::Evaluate (:472-493) added to the 28 sums of a pose; d = xiOdom^-1 o x
VG_HD void accumulate(const double *A, const double *J, const double *d, double *G)
{
    double r[6];
    for (int i = 0; i < 6; i++) {
        r[i] = 0.;
        for (int k = 0; k < 6; k++) r[i] += A[6 * i + k] * d[k];
    }
    int q = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++, q++)
            for (int k = 0; k < 6; k++) G[q] += J[6 * k + i] * J[6 * k + j];
    for (int i = 0; i < 6; i++)
        for (int k = 0; k < 6; k++) G[21 + i] += J[6 * k + i] * r[k];
    for (int k = 0; k < 6; k++) G[27] += 0.5 * (r[k] * r[k]);
}

inline void add_prior(const MotionPrior &p, const double *x, double *G)
{
    double d[6];
    vgth::inverse_compose(p.xi.data(), x, d);
    accumulate(p.A, p.J, d, G);
}

}  // namespace vgmp
