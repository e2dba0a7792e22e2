// vg_photometric_row.hpp -- what the photometric costs share per (pose, point): the pose row of an image gradient
// (CameraJacobian::dfdxi) and the 28 products of [J | r]^T [J | r] that the ordered reduction of vg_image_device.hpp sums.
// Included by vg_photometric.hpp (the photometric and the mutual-information cost) and vg_dense_ba.hpp; kept apart from
// vg_image_device.hpp so that the pipelines without a camera Jacobian do not reach the camera models.
#pragma once

#include "vg_camera.hpp"
#include "vg_image_device.hpp"

namespace vgs {

constexpr int kSums = 28;   // J^T J upper triangle row-major (21) | J^T r (6) | 1/2 sum r^2

// CameraJacobian::dfdxi (jacobian.h:98-115) for the point X in the camera frame, its projection Jacobian P (2 x 3 row-major)
// and the image gradient (g0, g1) = (d/du, d/dv): d = g0 P[0..2] + g1 P[3..5], row = (-d^T L11 | d^T (H L22 - L12)) with H the
// cross-product matrix of X.  The sums are returned unscaled: a caller with a factor (the loss derivative, 1 / sigma) applies it
// to the finished sums, never inside them.
VGS_HD void dfdxi_row(const double *X, const double *P, double g0, double g1, const double *L11, const double *L12, const double *L22, double *d,
                      double *row)
{
    const double H[9] = {0, -X[2], X[1], X[2], 0, -X[0], -X[1], X[0], 0};
    double B[9];
    vg::mat3_mul(H, L22, B);
    for (int k = 0; k < 9; k++) B[k] = B[k] - L12[k];
    for (int j = 0; j < 3; j++) d[j] = g0 * P[j] + g1 * P[3 + j];
    for (int j = 0; j < 3; j++) {
        row[j] = (-d[0]) * L11[0 + j] + (-d[1]) * L11[3 + j] + (-d[2]) * L11[6 + j];
        row[3 + j] = d[0] * B[0 + j] + d[1] * B[3 + j] + d[2] * B[6 + j];
    }
}

// the kSums products of one residual r and its pose row
__device__ __forceinline__ void row_products(const double *row, double r, double (&s)[kSums])
{
    int q = 0;
#pragma unroll
    for (int rr = 0; rr < 6; rr++)
#pragma unroll
        for (int c = rr; c < 6; c++) s[q++] = row[rr] * row[c];
#pragma unroll
    for (int k = 0; k < 6; k++) s[21 + k] = row[k] * r;
    s[27] = 0.5 * (r * r);
}

}  // namespace vgs
