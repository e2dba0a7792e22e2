// vg_stereo_host.hpp -- the host half of the stereo handles (vg_stereo, vg_motion_stereo): the parameter, camera and pose checks and
// setTransformation in FP64 -- R12 / R21 / t12, StereoEpipoles and the 2 x (planes + 1) curve tables.  vg_stereo builds them
// once at creation, vg_motion_stereo for every item of every call; both go through build_geometry, in one arithmetic order.
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "vg_geometry.hpp"
#include "vg_internal.hpp"
#include "vg_stereo_device.hpp"

namespace vgsh {

using vgi::fail;

inline void limit_vector(double *x)   // limitVector (epipoles.cpp:27-35)
{
    const double M = 1e6;
    for (int i = 0; i < 2; i++) {
        if (x[i] > M) x[i] = M;
        if (x[i] < -M) x[i] = -M;
    }
}

// EnhancedEpipolar::computePolynomial (eucm_epipolar.cpp:129-169) for the camera `p` with epipole `ep`
inline vgs::Poly2 compute_polynomial(const double *p, const double *ep, const double *plane)
{
    const double alpha = p[0], beta = p[1], fu = p[2], fv = p[3], u0 = p[4], v0 = p[5];
    const double gamma = 1 - alpha, ag = alpha - gamma, a2b = alpha * alpha * beta;
    const double fufv = fu * fv, fufu = fu * fu, fvfv = fv * fv;
    const double A = plane[0], B = plane[1], C = plane[2];
    const double AA = A * A, BB = B * B, CC = C * C;
    const double CCfufv = CC * fufv;
    const double dd = CCfufv / (AA + BB);
    vgs::Poly2 s;
    if ((AA + BB) > 0 && dd < 1.) {
        s.kuu = s.kuv = s.kvv = 0;
        s.ku = A / fu;
        s.kv = B / fv;
        const double normABinv = 1. / std::sqrt(AA + BB);
        const double Cnorm = C / std::sqrt(AA + BB + CC);
        const double du = -A * Cnorm * normABinv * fu;
        const double dv = -B * Cnorm * normABinv * fv;
        s.k1 = -(u0 + du) * A / fu - (v0 + dv) * B / fv;
    } else {
        s.kuu = (AA * ag + CC * a2b) / (CC * fufu);
        s.kuv = 2 * A * B * ag / (CCfufv);
        s.kvv = (BB * ag + CC * a2b) / (CC * fvfv);
        s.ku = 2 * (-(AA * fv * u0 + A * B * fu * v0) * ag - A * C * fufv * gamma - CC * a2b * fv * u0) / (CCfufv * fu);
        s.kv = 2 * (-(BB * fu * v0 + A * B * fv * u0) * ag - B * C * fufv * gamma - CC * a2b * fu * v0) / (CCfufv * fv);
        s.k1 = -(s.kuu * ep[0] * ep[0] + s.kuv * ep[0] * ep[1] + s.kvv * ep[1] * ep[1] + s.ku * ep[0] + s.kv * ep[1]);
    }
    return s;
}

inline void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// The ScaleParameters fields of p, the only ones the handles on a depth grid read: their ranges and the grid's size.  uMax / vMax
// are checked where they are read: always by a handle that also takes them for the image size (image_size_always), under
// equal_margins by the others.
inline int scaled_grid(const vg_stereo_params &p, bool image_size_always, int &x_max, int &y_max)
{
    if (p.scale < 1 || p.scale > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "scale must be in [1, 16384]");
    if ((image_size_always || p.equal_margins) && (p.u_max < 1 || p.u_max > 16384 || p.v_max < 1 || p.v_max > 16384))
        return fail(VG_ERR_INVALID_ARGUMENT, "uMax / vMax must be in [1, 16384]");
    if (std::abs(p.u0) > 16384 || std::abs(p.v0) > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "|u0|, |v0| must be at most 16384");
    x_max = p.x_max;
    y_max = p.y_max;
    if (p.equal_margins) {   // ScaleParameters::setEqualMargin (scale_parameters.cpp:44-52)
        x_max = (p.u_max - 2 * p.u0) / p.scale + 1;
        y_max = (p.v_max - 2 * p.v0) / p.scale + 1;
    }
    if (x_max < 1 || y_max < 1) return fail(VG_ERR_INVALID_ARGUMENT, "the scaled image is empty: xMax < 1 or yMax < 1");
    if (x_max > 16384 || y_max > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "xMax / yMax must be at most 16384");
    return VG_OK;
}

inline int check_params(const vg_stereo_params &p, int &x_max, int &y_max)
{
    if (p.hypotheses != 1) return fail(VG_ERR_INVALID_ARGUMENT, "hypotheses must be 1 (reconstructDisparityMH is not provided)");
    if (p.disp_max < 4 || p.disp_max > 256 || p.disp_max % 2) return fail(VG_ERR_INVALID_ARGUMENT, "disparity_max must be even in [4, 256]");
    if (p.desc_length < 3 || p.desc_length > vgs::kMaxDesc || p.desc_length % 2 == 0)
        return fail(VG_ERR_INVALID_ARGUMENT, "descriptor_size must be odd in [3, 31]");
    if (p.n_scales < 1 || p.n_scales > vgs::kMaxScales) return fail(VG_ERR_INVALID_ARGUMENT, "1 to 8 descriptor scales");
    for (int i = 0; i < p.n_scales; i++)
        if (p.scales[i] < 1 || p.scales[i] > 16) return fail(VG_ERR_INVALID_ARGUMENT, "every descriptor scale must be in [1, 16]");
    if (const int rc = scaled_grid(p, true, x_max, y_max)) return rc;
    if (p.num_epipolar_planes < 2 || p.num_epipolar_planes > (1 << 20) || p.num_epipolar_planes % 2)
        return fail(VG_ERR_INVALID_ARGUMENT, "num_epipolar_planes must be even in [2, 2^20]");
    if (p.epipole_margin < 0) return fail(VG_ERR_INVALID_ARGUMENT, "epipole_margin must be >= 0");
    if (p.flaw_cost < 0 || p.flaw_cost > 10000 || p.step_cost < 0 || p.step_cost > 10000 || p.jump_cost < 0 || p.jump_cost > 10000)
        return fail(VG_ERR_INVALID_ARGUMENT, "flaw_cost, step_cost and jump_cost must be in [0, 10000]");
    if (std::abs(p.desc_resp_thresh) > 1000000) return fail(VG_ERR_INVALID_ARGUMENT, "descriptor_response_thresh out of range");
    return VG_OK;
}

inline bool finite_n(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// what both handles ask of a camera pair and of a pose [t, rotvec] besides finite_n
inline bool focal_nonzero(const double *c1, const double *c2) { return c1[2] != 0. && c1[3] != 0. && c2[2] != 0. && c2[3] != 0.; }
// one camera: six finite values, fu and fv non-zero.  what: the camera's name in a handle that has more than one
inline int check_camera(const double *eucm, const char *what = nullptr)
{
    if (!finite_n(eucm, 6)) return fail(VG_ERR_INVALID_ARGUMENT, std::string(what ? what : "camera") + " parameters must be finite");
    if (!focal_nonzero(eucm, eucm)) return fail(VG_ERR_INVALID_ARGUMENT, (what ? std::string(what) + ": " : std::string()) + "fu, fv must be non-zero");
    return VG_OK;
}
inline bool has_baseline(const double *xi) { return xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2] > 1e-10; }   // false for NaN

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// the host half of the handle: transform, epipoles (StereoEpipoles ctor, epipoles.cpp:37-57), curve bases and tables
// (EnhancedEpipolar::initialize, eucm_epipolar.cpp:33-107); `table` holds 2 x (num_epipolar_planes + 1) entries
inline int build_geometry(vgs::StereoGeom &g, const vg_stereo_params &p, const double *c1, const double *c2, const double *xi, vgs::Poly2 *table)
{
    for (int i = 0; i < 6; i++) {
        g.c1[i] = c1[i];
        g.c2[i] = c2[i];
    }
    const vg::RotTrig rt = vg::rot_trig(xi + 3, true, false);
    vg::rotation_matrix(xi + 3, 1., rt, g.R);
    vg::rotation_matrix(xi + 3, -1., rt, g.Rinv);
    for (int i = 0; i < 3; i++) g.t[i] = xi[i];

    double ep[2][2][2];
    const double mt[3] = {-g.t[0], -g.t[1], -g.t[2]};
    double ti[3], mti[3];
    vgs::mat_vec(g.Rinv, g.t, ti);
    for (int i = 0; i < 3; i++) {
        ti[i] = -ti[i];   // transInv = -rotMatInv t
        mti[i] = -ti[i];
    }
    g.epi_ok[0][0] = vgs::eucm_project(c1, g.t, ep[0][0]);
    g.epi_ok[0][1] = vgs::eucm_project(c1, mt, ep[0][1]);
    g.epi_ok[1][0] = vgs::eucm_project(c2, ti, ep[1][0]);
    g.epi_ok[1][1] = vgs::eucm_project(c2, mti, ep[1][1]);
    for (int c = 0; c < 2; c++) {
        if (!g.epi_ok[c][0] && !g.epi_ok[c][1])
            return fail(VG_ERR_INVALID_ARGUMENT, std::string("neither the epipole nor the anti-epipole projects into camera ") +
                                                     (c == 0 ? "1" : "2"));
        for (int k = 0; k < 2; k++) {
            if (!g.epi_ok[c][k]) {
                ep[c][k][0] = ep[c][k][1] = 0.;
                g.epi_px[c][k][0] = g.epi_px[c][k][1] = 0;
                continue;
            }
            limit_vector(ep[c][k]);
            g.epi_px[c][k][0] = (int)std::round(ep[c][k][0]);
            g.epi_px[c][k][1] = (int)std::round(ep[c][k][1]);
        }
    }

    // the epipolar basis
    const int n = p.num_epipolar_planes;
    g.n_planes = n;
    g.plane_step = 4. / n;
    const double tn = std::sqrt(g.t[0] * g.t[0] + g.t[1] * g.t[1] + g.t[2] * g.t[2]);
    double z[3];
    for (int i = 0; i < 3; i++) z[i] = -(g.t[i] / tn);
    const int axis = (z[2] * z[2] > z[0] * z[0] + z[1] * z[1]) ? 0 : 2;
    double xb[3];
    for (int i = 0; i < 3; i++) xb[i] = (i == axis ? 1. : 0.) - z[i] * z[axis];
    const double xn = std::sqrt(xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2]);
    for (int i = 0; i < 3; i++) g.xBase[i] = xb[i] / xn;
    cross3(z, g.xBase, g.yBase);

    double z2[3];
    vgs::mat_vec(g.Rinv, z, z2);   // t21n
    for (int c = 0; c < 2; c++) {
        const double *cam = c == 0 ? c1 : c2;
        const int k = g.epi_ok[c][0] ? 0 : 1;   // StereoEpipoles::get(idx)
        for (int idx = 0; idx < n; idx++) {
            double dir[3];
            if (idx < n / 2) {
                const double sv = g.plane_step * idx - 1;
                for (int i = 0; i < 3; i++) dir[i] = g.xBase[i] + sv * g.yBase[i];
            } else {
                const double cv = g.plane_step * (-idx + n / 2) + 1;
                for (int i = 0; i < 3; i++) dir[i] = cv * g.xBase[i] + g.yBase[i];
            }
            double plane[3];
            if (c == 0) {
                cross3(dir, z, plane);
            } else {
                double dir2[3];
                vgs::mat_vec(g.Rinv, dir, dir2);
                cross3(dir2, z2, plane);
            }
            table[(size_t)c * (n + 1) + idx] = compute_polynomial(cam, ep[c][k], plane);
        }
        table[(size_t)c * (n + 1) + n] = table[(size_t)c * (n + 1)];
    }

    g.scale = p.scale;
    g.u0 = p.u0;
    g.v0 = p.v0;
    g.u_max = p.u_max;
    g.v_max = p.v_max;
    g.epipole_margin = p.epipole_margin;
    g.disp_max = p.disp_max;
    g.error_max = p.error_max;
    g.flaw_cost = p.flaw_cost;
    g.desc_length = p.desc_length;
    g.n_scales = p.n_scales;
    for (int i = 0; i < vgs::kMaxScales; i++) g.scales[i] = i < p.n_scales ? p.scales[i] : 1;
    g.desc_resp_thresh = p.desc_resp_thresh;
    g.step_cost = p.step_cost;
    g.jump_cost = p.jump_cost;
    g.image_based_cost = p.image_based_cost != 0;
    g.salient_points_only = p.salient_points_only != 0;
    g.use_uv_cache = p.use_uv_cache != 0;
    return VG_OK;
}

}  // namespace vgsh
