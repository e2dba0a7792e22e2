// vg_bicubic.hpp -- ceres::BiCubicInterpolator over the reference's clamping Grid2D (include/ceres.h), for any sample type that
// converts to double: the float pyramids of photometric localization (vg_photometric.hpp) and the 8-bit textures of the scene
// renderer (vg_render.hpp) share this one restatement.
#pragma once

#include "vg_stereo_device.hpp"

namespace vgs {

VGS_HD int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }   // Grid2D::GetValue (include/ceres.h:55-64)

// ceres::CubicHermiteSpline<1>
VGS_HD void cubic(double p0, double p1, double p2, double p3, double x, double &f, double &dfdx)
{
    const double a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3);
    const double b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3);
    const double c = 0.5 * (-p0 + p2);
    const double d = p1;
    f = d + x * (c + x * (b + x * a));
    dfdx = c + x * (2.0 * b + 3.0 * a * x);
}

// ceres::BiCubicInterpolator<Grid2D<T>>::Evaluate(r, c): the four rows row - 1 .. row + 2 along the columns, then those
// four values and their column derivatives along r; the grid clamps its indices (include/ceres.h:55-64)
template <class T>
VGS_HD void bicubic(const T *img, int w, int h, double r, double c, double &f, double &dfdr, double &dfdc)
{
    const int row = (int)floor(r), col = (int)floor(c);
    double fk[4], dk[4];
    int cc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) cc[j] = clamp_index(col - 1 + j, w);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const T *p = img + (int64_t)clamp_index(row - 1 + k, h) * w;
        cubic((double)p[cc[0]], (double)p[cc[1]], (double)p[cc[2]], (double)p[cc[3]], c - col, fk[k], dk[k]);
    }
    double unused;
    cubic(fk[0], fk[1], fk[2], fk[3], r - row, f, dfdr);
    cubic(dk[0], dk[1], dk[2], dk[3], r - row, dfdc, unused);
}

}  // namespace vgs
