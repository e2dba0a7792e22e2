// vg_unproject.hpp -- pixel -> viewing ray of ONE pixel for the five camera models, host and device: the inverse of eval_corner
// (vg_camera.hpp).  Used by the conversion between camera models (vg_convert.hpp).
//
// Self-contained like vg_lm6.hpp: <cmath> and the model list, so a plain host compiler takes it (tests/host/unproject_check.cpp).
// Every statement keeps one shape for both builds; tests/convert_ref.py restates the order below in numpy.
//
//   unproject<MODEL>(intr, u, v, X)        the ray X through pixel (u, v), NOT normalised; false (X untouched or unspecified) where
//                                          the pixel is outside the model's domain
//   unproject_unit<MODEL>(intr, u, v, X)   X / sqrt(x^2 + y^2 + z^2), summed in that order; (0, 0, 0) and false where it fails
//
// Order of operations.  A NaN or infinite pixel fails in every model, before anything is computed; a ray with a component that is
// not finite fails, after everything is computed.  Below (mx, my) = ((u - u0) / fu, (v - v0) / fv) and r2 = mx mx + my my.
//
// EUCM [alpha, beta, fu, fv, u0, v0] (the reference's reconstructPoint, eucm.h:85-106):
//   gamma = 1 - alpha;  num = 1 - r2 alpha alpha beta;  det = 1 - (alpha - gamma) beta r2;  fails when det < 0
//   X = (mx, my, num / (gamma + alpha sqrt(det)))
// UCM [xi, fu, fv, u0, v0] (ucm.h:81-103):
//   disc = 1 + r2 (1 - xi xi);  fails when disc < 0 (the reference returns true and a NaN ray there: DESIGN.md section 9)
//   g = sqrt(disc);  en = -g - xi r2;  ed = xi xi r2 - 1;  X = (mx, my, ed / (ed + xi en))
// Mei [xi, k1, k2, k3, k4, k5, fu, fv, u0, v0]: with k1 = ... = k5 = 0 exactly UCM's statements on (mx, my) (the reference's
//   reconstructPoint, mei.h:90-112, which ignores the distortion whatever its values: DESIGN.md section 9).  Otherwise (mx, my) is
//   the DISTORTED normalised point and distort(m) = (mx, my) is solved first, by Newton in two dimensions from m = (mx, my):
//     xx = x x, xy = x y, yy = y y, q = xx + yy;  D = 1 + k1 q + k2 q q + k3 q q q;  dD = k1 + 2 k2 q + 3 k3 q q
//     f = (x D + 2 k4 xy + k5 (q + 2 xx) - mx,  y D + 2 k5 xy + k4 (q + 2 yy) - my)          (eval_corner's expressions)
//     a0 = D + 2 xx dD + 2 k4 y + 6 k5 x;  a1 = 2 xy dD + 2 k4 x + 2 k5 y;  b1 = D + 2 yy dD + 2 k5 x + 6 k4 y   (b0 = a1)
//     det = a0 b1 - a1 a1;  fails when !(det > 0): the distortion has folded over
//     dx = (b1 f0 - a1 f1) / det;  dy = (a0 f1 - a1 f0) / det;  x -= dx;  y -= dy;  fails when x or y is not finite
//     settled when max(|dx|, |dy|) <= 1e-12 max(|x|, |y|);  at most 20 steps, fails when none settles
//   then UCM's statements on the settled (x, y).
// Kannala-Brandt [k1, k2, k3, k4, fu, fv, u0, v0] (vgcal::reconstruct_point, vg_calibration.hpp):
//   rd = hypot(mx, my);  rd = 0 gives (0, 0, 1);  theta from rd by Newton on d(theta) = rd, at most 20 steps, fails when d' <= 0 on
//   the way or at the root, when theta leaves [0, pi] or when no step satisfies |step| <= 1e-12 theta
//   X = (sin(theta) / rd mx, sin(theta) / rd my, cos(theta))
// double sphere [xi, alpha, fu, fv, u0, v0] (vgcal::reconstruct_point):
//   fails when alpha > 0.5 and r2 > 1 / (2 alpha - 1)
//   mz = (1 - alpha alpha r2) / (alpha sqrt(1 - (2 alpha - 1) r2) + 1 - alpha)
//   sc = (mz xi + sqrt(mz mz + (1 - xi xi) r2)) / (mz mz + r2);  X = (sc mx, sc my, sc mz - xi)
#pragma once

#include <cmath>
#include <type_traits>

#include "vg_model_list.hpp"

#if defined(__HIPCC__)
#define VG_UNPROJECT_FN __host__ __device__ __forceinline__
#else
#define VG_UNPROJECT_FN inline
#endif

namespace vg {

constexpr int kUnprojectNewtonSteps = 20;
constexpr double kUnprojectSettled = 1e-12;
constexpr double kUnprojectPi = 3.14159265358979323846;

// the unified model's ray through the undistorted normalised point (x, y)
VG_UNPROJECT_FN bool unproject_unified(double xi, double x, double y, double X[3])
{
    const double u2 = x * x + y * y;
    const double disc = 1. + u2 * (1 - xi * xi);
    if (disc < 0) return false;
    const double gamma = std::sqrt(disc);
    const double etanum = -gamma - xi * u2;
    const double etadenom = xi * xi * u2 - 1;
    X[0] = x;
    X[1] = y;
    X[2] = etadenom / (etadenom + xi * etanum);
    return true;
}

VG_UNPROJECT_FN bool unproject_model(const double *p, double u, double v, double X[3], std::integral_constant<int, kEUCM>)
{
    const double alpha = p[0], beta = p[1], fu = p[2], fv = p[3], u0 = p[4], v0 = p[5];
    const double xn = (u - u0) / fu, yn = (v - v0) / fv;
    const double u2 = xn * xn + yn * yn;
    const double gamma = 1. - alpha;
    const double num = 1. - u2 * alpha * alpha * beta;
    const double det = 1 - (alpha - gamma) * beta * u2;
    if (det < 0) return false;
    const double denom = gamma + alpha * std::sqrt(det);
    X[0] = xn;
    X[1] = yn;
    X[2] = num / denom;
    return true;
}

VG_UNPROJECT_FN bool unproject_model(const double *p, double u, double v, double X[3], std::integral_constant<int, kUCM>)
{
    const double xi = p[0], fu = p[1], fv = p[2], u0 = p[3], v0 = p[4];
    return unproject_unified(xi, (u - u0) / fu, (v - v0) / fv, X);
}

VG_UNPROJECT_FN bool unproject_model(const double *p, double u, double v, double X[3], std::integral_constant<int, kMEI>)
{
    const double xi = p[0], k1 = p[1], k2 = p[2], k3 = p[3], k4 = p[4], k5 = p[5];
    const double fu = p[6], fv = p[7], u0 = p[8], v0 = p[9];
    const double mx = (u - u0) / fu, my = (v - v0) / fv;
    if (k1 == 0. && k2 == 0. && k3 == 0. && k4 == 0. && k5 == 0.) return unproject_unified(xi, mx, my, X);
    double x = mx, y = my;
    bool settled = false;
    for (int it = 0; it < kUnprojectNewtonSteps && !settled; it++) {
        const double xx = x * x, xy = x * y, yy = y * y;
        const double r2 = xx + yy;
        const double D = 1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
        const double dDdr2 = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2;
        const double deltax = 2. * k4 * xy + k5 * (r2 + 2. * xx);
        const double deltay = 2. * k5 * xy + k4 * (r2 + 2. * yy);
        const double f0 = x * D + deltax - mx, f1 = y * D + deltay - my;
        const double a0 = D + 2 * xx * dDdr2 + 2 * k4 * y + 6 * k5 * x;
        const double a1 = 2 * xy * dDdr2 + 2 * k4 * x + 2 * k5 * y;
        const double b1 = D + 2 * yy * dDdr2 + 2 * k5 * x + 6 * k4 * y;
        const double det = a0 * b1 - a1 * a1;
        if (!(det > 0.)) return false;
        const double dx = (b1 * f0 - a1 * f1) / det, dy = (a0 * f1 - a1 * f0) / det;
        x -= dx;
        y -= dy;
        if (!(std::isfinite(x) && std::isfinite(y))) return false;
        settled = std::fmax(std::fabs(dx), std::fabs(dy)) <= kUnprojectSettled * std::fmax(std::fabs(x), std::fabs(y));
    }
    if (!settled) return false;
    return unproject_unified(xi, x, y, X);
}

VG_UNPROJECT_FN bool unproject_model(const double *p, double u, double v, double X[3], std::integral_constant<int, kKB>)
{
    const double k1 = p[0], k2 = p[1], k3 = p[2], k4 = p[3], fu = p[4], fv = p[5], u0 = p[6], v0 = p[7];
    const double mx = (u - u0) / fu, my = (v - v0) / fv;
    const double rd = std::hypot(mx, my);
    if (rd == 0.) {
        X[0] = 0.;
        X[1] = 0.;
        X[2] = 1.;
        return true;
    }
    double theta = rd;
    bool settled = false;
    for (int it = 0; it < kUnprojectNewtonSteps && !settled; it++) {
        const double t2 = theta * theta;
        const double d = theta * (1. + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
        const double dp = 1. + t2 * (3. * k1 + t2 * (5. * k2 + t2 * (7. * k3 + t2 * (9. * k4))));
        if (!(dp > 0.)) return false;
        const double step = (d - rd) / dp;
        theta -= step;
        if (!(theta >= 0. && theta <= kUnprojectPi)) return false;
        settled = std::fabs(step) <= kUnprojectSettled * theta;
    }
    if (!settled) return false;
    {   // the polynomial must not have folded over at the root either
        const double t2 = theta * theta;
        if (!(1. + t2 * (3. * k1 + t2 * (5. * k2 + t2 * (7. * k3 + t2 * (9. * k4)))) > 0.)) return false;
    }
    const double sc = std::sin(theta) / rd;
    X[0] = sc * mx;
    X[1] = sc * my;
    X[2] = std::cos(theta);
    return true;
}

VG_UNPROJECT_FN bool unproject_model(const double *p, double u, double v, double X[3], std::integral_constant<int, kDS>)
{
    const double xi = p[0], alpha = p[1], fu = p[2], fv = p[3], u0 = p[4], v0 = p[5];
    const double mx = (u - u0) / fu, my = (v - v0) / fv;
    const double r2 = mx * mx + my * my;
    if (alpha > 0.5 && r2 > 1. / (2. * alpha - 1.)) return false;
    const double mz = (1. - alpha * alpha * r2) / (alpha * std::sqrt(1. - (2. * alpha - 1.) * r2) + 1. - alpha);
    const double sc = (mz * xi + std::sqrt(mz * mz + (1. - xi * xi) * r2)) / (mz * mz + r2);
    X[0] = sc * mx;
    X[1] = sc * my;
    X[2] = sc * mz - xi;
    return true;
}

template <int MODEL>
VG_UNPROJECT_FN bool unproject(const double *intr, double u, double v, double X[3])
{
    if (!(std::isfinite(u) && std::isfinite(v))) return false;
    double Y[3];
    if (!unproject_model(intr, u, v, Y, std::integral_constant<int, MODEL>{})) return false;
    if (!(std::isfinite(Y[0]) && std::isfinite(Y[1]) && std::isfinite(Y[2]))) return false;
    X[0] = Y[0];
    X[1] = Y[1];
    X[2] = Y[2];
    return true;
}

template <int MODEL>
VG_UNPROJECT_FN bool unproject_unit(const double *intr, double u, double v, double X[3])
{
    double Y[3];
    bool ok = unproject<MODEL>(intr, u, v, Y);
    const double n = ok ? std::sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]) : 0.;
    ok = ok && n > 0. && std::isfinite(n);
    X[0] = ok ? Y[0] / n : 0.;
    X[1] = ok ? Y[1] / n : 0.;
    X[2] = ok ? Y[2] / n : 0.;
    return ok;
}

}  // namespace vg
