// vg_stereo_device.hpp -- the FP64 pieces the host and the kernels of both stereo translation units share (vg_stereo_tu.hip:
// EnhancedSgm, vg_motion_tu.hip: MotionStereo): EUCM reconstruct / project, the epipolar-curve rasteriser, the curve index,
// the epipole choice, the regular triangulation of two point pairs; and, for the kernels alone, the descriptor matching of
// stereo_curve_cost_kernel and motion_stereo_kernel (EpipolarDescriptor::compute, the thresholds and the DP of
// compareDescriptor, the block's LDS).  Everything is evaluated in the order written (the library is built with
// -ffp-contract=off), so the host walk, the kernels and the restatements in tests/ agree bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace vgs {

#define VGS_HD __host__ __device__ __forceinline__

enum : int { kEpipoleInverted = 1, kEpipoleTooClose = 2 };      // EpipoleResult (epipoles.h:33)
enum : int { kGeomMask = 1, kGeomPinf = 2 };                    // status bits of a geometry entry
constexpr int kDisparityMargin = 20;                            // DISPARITY_MARGIN (eucm_sgm.h:162)
constexpr int kMaxDesc = 31, kMaxHalf = 15, kMaxScales = 8;
constexpr int kMoveLimit = 1 << 20;                             // largest single rasteriser move (see rnd_move)
constexpr int kInf = 1 << 28;                                   // "no path" in the descriptor DP; kInf + cost stays < 2^31
constexpr double kTriangulateDistMax = 100.;                    // TRIANGULATE_DIST_MAX (eucm_stereo.cpp:250)
constexpr double kTriEps = 1e-3;                                // Triangulator(1e-3)

// one depth pixel's geometry, written once per handle
struct GeomEntry {
    int status;        // kGeomMask: camera 1 reconstructs the pixel; kGeomPinf: its point at infinity projects into camera 2
    int pinf_u, pinf_v;  // round(pinf)
    int index;         // EnhancedEpipolar::index of the reconstructed ray
    int flags1, flags2;  // chooseEpipole for camera 1 at the pixel, for camera 2 at pinf
    int pad0, pad1;
};

struct Poly2 {
    double kuu, kuv, kvv, ku, kv, k1;
};

VGS_HD double poly_val(const Poly2 &s, int u, int v)
{
    return (s.kuu * u + s.kuv * v + s.ku) * u + (s.kvv * v + s.kv) * v + s.k1;
}
VGS_HD double poly_gu(const Poly2 &s, int u, int v) { return 2 * s.kuu * u + s.kuv * v + s.ku; }
VGS_HD double poly_gv(const Poly2 &s, int u, int v) { return s.kuv * u + 2 * s.kvv * v + s.kv; }

VGS_HD int sgn(double x) { return 2 * int(x > 0) - 1; }   // sign (std.h:74): sign(0) = -1

// -round(x) as the int a move takes.  The reference converts without a bound (undefined past INT_MAX, e.g. 0/0 where both
// gradients vanish); here NaN moves 0 and the move is clamped to +-2^20, so every walk stays far inside int range.
VGS_HD int rnd_move(double x)
{
    double r = round(x);
    if (!(r == r)) return 0;
    r = r < -kMoveLimit ? -kMoveLimit : (r > kMoveLimit ? kMoveLimit : r);
    return -(int)r;
}

// CurveRasterizer<int, Polynomial2> (curve_rasterizer.h, the second definition)
struct Raster {
    double delta, fu, fv;
    int eps, u, v;
    Poly2 surf;

    VGS_HD void init(int u_, int v_, int eu, int ev, const Poly2 &s)
    {
        u = u_;
        v = v_;
        surf = s;
        fu = poly_gu(surf, u, v);
        fv = poly_gv(surf, u, v);
        delta = poly_val(surf, u, v);
        eps = (fu * (ev - v) - fv * (eu - u) > 0) ? 1 : -1;
    }
    VGS_HD void move_u(int du)
    {
        if (du == 0) return;
        u += du;
        const double fu2 = poly_gu(surf, u, v);
        delta += 0.5 * du * (fu + fu2);
        fu = fu2;
        fv = poly_gv(surf, u, v);
    }
    VGS_HD void move_v(int dv)
    {
        if (dv == 0) return;
        v += dv;
        const double fv2 = poly_gv(surf, u, v);
        delta += 0.5 * dv * (fv + fv2);
        fv = fv2;
        fu = poly_gu(surf, u, v);
    }
    VGS_HD void step()
    {
        if (fabs(fu) > fabs(fv)) {
            move_v(eps * sgn(fu));
            move_u(rnd_move(delta / fu));
        } else {
            move_u(-eps * sgn(fv));
            move_v(rnd_move(delta / fv));
        }
    }
    VGS_HD void unstep()
    {
        if (fabs(fu) > fabs(fv)) {
            move_v(-eps * sgn(fu));
            move_u(rnd_move(delta / fu));
        } else {
            move_u(eps * sgn(fv));
            move_v(rnd_move(delta / fv));
        }
    }
    VGS_HD void steps(int n)
    {
        if (n > 0)
            for (int i = 0; i < n; i++) step();
        else
            for (int i = 0; i > n; i--) unstep();
    }
};

// EnhancedCamera::reconstructPoint (eucm.h:85-104)
VGS_HD bool eucm_reconstruct(const double *p, double u, double v, double *X)
{
    const double alpha = p[0], beta = p[1], fu = p[2], fv = p[3], u0 = p[4], v0 = p[5];
    const double xn = (u - u0) / fu;
    const double yn = (v - v0) / fv;
    const double u2 = xn * xn + yn * yn;
    const double gamma = 1. - alpha;
    const double num = 1. - u2 * alpha * alpha * beta;
    const double det = 1 - (alpha - gamma) * beta * u2;
    if (det < 0) return false;
    const double denom = gamma + alpha * sqrt(det);
    X[0] = xn;
    X[1] = yn;
    X[2] = num / denom;
    return true;
}

// EnhancedProjector (eucm.h:30-63)
VGS_HD bool eucm_project(const double *p, const double *X, double *uv)
{
    const double alpha = p[0], beta = p[1], fu = p[2], fv = p[3], u0 = p[4], v0 = p[5];
    const double x = X[0], y = X[1], z = X[2];
    const double denom = alpha * sqrt(z * z + beta * (x * x + y * y)) + (1. - alpha) * z;
    if (denom < 1e-3) return false;
    if (alpha > 0.5) {
        const double zn = z / denom;
        const double C = (alpha - 1.) / (alpha + alpha - 1.);
        if (zn < C) return false;
    }
    uv[0] = fu * (x / denom) + u0;
    uv[1] = fv * (y / denom) + v0;
    return true;
}

VGS_HD double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
VGS_HD void mat_vec(const double *M, const double *x, double *y)   // y = M x, M row-major
{
    for (int i = 0; i < 3; i++) y[i] = M[3 * i] * x[0] + M[3 * i + 1] * x[1] + M[3 * i + 2] * x[2];
}
VGS_HD int round_int(double x) { return (int)round(x); }

// Triangulator::regDiv (triangulator.cpp:114-129)
VGS_HD double reg_div(double num, double denom)
{
    if (denom > kTriEps * num) return num / denom;
    if (num == 0) return 2. / kTriEps;
    return 2. / kTriEps - denom / (num * kTriEps * kTriEps);
}

// Triangulator::computeRegular, the first root only (triangulator.cpp:145-175); R, t: Transf T12 (rotMat, trans)
VGS_HD double triangulate_lambda(const double *R, const double *t, const double *p, const double *q0)
{
    double q[3], r[3];
    mat_vec(R, q0, q);
    for (int i = 0; i < 3; i++) r[i] = p[i] + q[i];
    const double tp = dot3(t, p), tq = dot3(t, q), tr = dot3(t, r), tt = dot3(t, t);
    const double rp = dot3(r, p), rq = dot3(r, q);
    const double delta = tp * rq - tq * rp;
    const double delta1 = tt * rq - tr * tq;
    return reg_div(delta1, delta);
}

// everything the kernels read about one handle (host-built, passed by value)
struct StereoGeom {
    double c1[6], c2[6];
    double R[9], Rinv[9], t[3];       // Transf T12: rotMat, rotMatInv, trans
    double xBase[3], yBase[3];
    double plane_step;                // 4 / num_epipolar_planes
    int n_planes;
    int epi_px[2][2][2];              // [camera][0 epipole, 1 anti-epipole][u, v]
    int epi_ok[2][2];                 // projected?
    const Poly2 *table;               // DEVICE [2][n_planes + 1]
    int scale, u0, v0, u_max, v_max, x_max, y_max;
    int epipole_margin;               // squared
    int disp_max, error_max, flaw_cost, desc_length, n_scales, scales[kMaxScales], desc_resp_thresh;
    int step_cost, jump_cost, image_based_cost, salient_points_only, use_uv_cache;
};

// EnhancedEpipolar::index (eucm_epipolar.cpp:110-127)
VGS_HD int curve_index(const StereoGeom &g, const double *X)
{
    const double c = dot3(X, g.xBase), ac = fabs(c);
    const double s = dot3(X, g.yBase), as = fabs(s);
    if (ac + as < 1e-4) return 0;
    const int i = ac > as ? round_int((s / c + 1) / g.plane_step) : round_int((1 - c / s) / g.plane_step) + g.n_planes / 2;
    return i < 0 ? 0 : (i > g.n_planes ? g.n_planes : i);   // in range already; the clamp only guards the table read
}

// StereoEpipoles::chooseEpipole (epipoles.cpp:59-93); squared distances in double (the reference's int squaredNorm can
// overflow for an epipole near the +-1e6 limit).  Neither epipole projected is refused by vg_stereo_create.
VGS_HD int choose_epipole(const StereoGeom &g, int cam, int u, int v)
{
    int res = 0;
    const double du = (double)u - g.epi_px[cam][0][0], dv = (double)v - g.epi_px[cam][0][1];
    const double au = (double)u - g.epi_px[cam][1][0], av = (double)v - g.epi_px[cam][1][1];
    const double dist = du * du + dv * dv, anti = au * au + av * av;
    const double th = g.epipole_margin;
    if (g.epi_ok[cam][0] && g.epi_ok[cam][1]) {
        if (anti < dist) {
            res |= kEpipoleInverted;
            if (anti < th) res |= kEpipoleTooClose;
        } else if (dist < th) res |= kEpipoleTooClose;
    } else if (g.epi_ok[cam][0]) {
        if (dist < th) res |= kEpipoleTooClose;
    } else {
        res |= kEpipoleInverted;
        if (anti < th) res |= kEpipoleTooClose;
    }
    return res;
}

// EnhancedSgm::getCurveRasteriser (eucm_sgm.cpp:33-46)
VGS_HD void make_raster(const StereoGeom &g, int cam, int u, int v, int index, int flags, Raster &r)
{
    const int inv = (flags & kEpipoleInverted) ? 1 : 0;
    r.init(u, v, g.epi_px[cam][inv][0], g.epi_px[cam][inv][1], g.table[cam * (g.n_planes + 1) + index]);
    if (inv) r.eps *= -1;
}

VGS_HD bool inside(const StereoGeom &g, int u, int v) { return !(v < 0 || v >= g.v_max || u < 0 || u >= g.u_max); }

VGS_HD int compute_error(int v, int th)   // computeError (eucm_stereo.cpp:73-76); th = thMin | thMax << 8
{
    const int lo = th & 255, hi = th >> 8;
    const int a = lo - v, b = v - hi;
    return 0 > (a > b ? a : b) ? 0 : (a > b ? a : b);
}

VGS_HD int imin(int a, int b) { return a < b ? a : b; }

// the four-point triangulate (eucm_stereo.cpp:250-296): a pixel of camera 1 and its successor on the curve, (a, b) against
// (c, d) in camera 2.  Distance of the first pair, and as its uncertainty the difference to the second pair's (both along
// the first ray).  False when one of the four does not reconstruct.
VGS_HD bool triangulate_pairs(const StereoGeom &g, int ua, int va, int ub, int vb, int uc, int vc, int ud, int vd, double &dist, double &sigma)
{
    double p1[3], p2[3], q1[3], q2[3];
    if (!eucm_reconstruct(g.c1, (double)ua, (double)va, p1) || !eucm_reconstruct(g.c1, (double)ub, (double)vb, p2) ||
        !eucm_reconstruct(g.c2, (double)uc, (double)vc, q1) || !eucm_reconstruct(g.c2, (double)ud, (double)vd, q2))
        return false;
    const double pn = sqrt(dot3(p1, p1));
    dist = triangulate_lambda(g.R, g.t, p1, q1) * pn;
    sigma = fabs(triangulate_lambda(g.R, g.t, p2, q2) * pn - dist);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// EpipolarDescriptor::compute and compareDescriptor for one depth pixel per lane: the one implementation behind
// stereo_curve_cost_kernel and motion_stereo_kernel.  The kernels keep what differs: where a sample comes from, what leaving
// the image does, and what becomes of a final column.

constexpr int kRing = 32;          // > 2 HALF_LENGTH: the lag of the second half of compareDescriptor
constexpr int kMatchLanes = 256;   // lanes per block of both kernels

struct MatchLds {   // one block's LDS, 56 576 bytes: two blocks per CU
    int ring[kRing][kMatchLanes];          // (V_H[j] << 8) | sample[j] at slot j % kRing
    uint16_t thr[kMaxDesc][kMatchLanes];   // thMin | thMax << 8
    uint8_t desc[kMaxDesc][kMatchLanes];
};

// EpipolarDescriptor::compute: the descriptor around `ref` at the first scale whose response passes (else the last one) goes
// to lds.desc; returns that scale, or -1 when a descriptor leaves the image
__device__ __forceinline__ int compute_descriptor(const StereoGeom &g, const Raster &ref, const uint8_t *im1, MatchLds &lds, int lane, int &resp)
{
    const int L = g.desc_length, H = L / 2;
    const int wave_thresh = g.desc_resp_thresh * L;
    int step = -1;
    resp = 0;
    for (int si = 0; si < g.n_scales; si++) {
        const int sc = g.scales[si];
        Raster r = ref;
        r.eps *= -sc;
        r.steps(-H);
        for (int i = 0; i < L; i++, r.step()) {
            if (!inside(g, r.u, r.v)) return -1;
            lds.desc[i][lane] = im1[(int64_t)r.v * g.u_max + r.u];
        }
        int tv = 0;
        for (int i = 1; i < L; i++) tv += abs((int)lds.desc[i - 1][lane] - (int)lds.desc[i][lane]);
        resp = (tv * 100) / ((int)lds.desc[H][lane] + 30);
        step = sc;
        if (abs(resp) > wave_thresh) break;
    }
    return step;
}

// the thresholds of lds.desc (compareDescriptor, eucm_stereo.cpp:81-113)
__device__ __forceinline__ void descriptor_thresholds(MatchLds &lds, int L, int lane)
{
    for (int i = 0; i < L; i++) {
        const int di = lds.desc[i][lane];
        int lo, hi;
        if (i == 0 || i == L - 1) {
            const int dn = lds.desc[i == 0 ? 1 : L - 2][lane];
            const int m = (di + dn) / 2;
            if (di > dn) {
                lo = m;
                hi = di;
            } else {
                hi = m;
                lo = di;
            }
        } else {
            const int d1 = (di + lds.desc[i - 1][lane]) / 2, d2 = (di + lds.desc[i + 1][lane]) / 2;
            lo = imin(di, imin(d1, d2));
            hi = di > d1 ? (di > d2 ? di : d2) : (d1 > d2 ? d1 : d2);
        }
        lds.thr[i][lane] = (uint16_t)(lo | hi << 8);
    }
}

// compareDescriptor's two row DPs as one stream over the N samples of a lane.  The first half (descriptor rows 0 .. H, columns
// left to right) keeps two columns of history per row; the second half (rows L-1 .. H+1, whose recurrence looks two columns to
// the right) runs row k lagged by 2k columns, so at time t the cost of column t - 2H is final.  The samples and the first-half
// results of the last kRing columns live in lds.ring.  Per time step t = 0 .. N + 2H - 1: push (while t < N), then advance.
struct MatchDp {
    int v1[kMaxHalf], v2[kMaxHalf];                 // first half: rows 0 .. H-1, columns t-1 and t-2
    int w0[kMaxHalf], w1[kMaxHalf], w2[kMaxHalf];   // second half, level k = row L-1-k: its last three columns

    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int i = 0; i < kMaxHalf; i++) {
            v1[i] = v2[i] = kInf;
            w0[i] = w1[i] = w2[i] = kInf;
        }
    }
    // first half, column t, and the ring write
    __device__ __forceinline__ void push(MatchLds &lds, int lane, int H, int f, int t, int s)
    {
        int cur = compute_error(s, lds.thr[0][lane]);
#pragma unroll
        for (int i = 1; i <= kMaxHalf; i++) {
            if (i <= H) {
                const int nv = imin(cur + f, imin(v1[i - 1], v2[i - 1] + f)) + compute_error(s, lds.thr[i][lane]);
                v2[i - 1] = v1[i - 1];
                v1[i - 1] = cur;
                cur = nv;
            }
        }
        lds.ring[t % kRing][lane] = cur << 8 | s;
    }
    // second half: level k at column t - 2k.  True once column j = t - 2H has all its rows (j >= H), its cost in `total`.
    __device__ __forceinline__ bool advance(MatchLds &lds, int lane, int L, int f, int t, int N, int &total)
    {
        const int H = L / 2;
#pragma unroll
        for (int k = 0; k < kMaxHalf; k++) {
            if (k < H) {
                const int c = t - 2 * k;
                int val = kInf;
                if (c >= 0 && c < N) {
                    const int sc = lds.ring[c % kRing][lane] & 255;
                    const int ev = compute_error(sc, lds.thr[L - 1 - k][lane]);
                    if (k == 0) val = ev;
                    else val = imin(w2[k - 1] + f, imin(w1[k - 1], w0[k - 1] + f)) + ev;
                }
                w2[k] = w1[k];
                w1[k] = w0[k];
                w0[k] = val;
            }
        }
        const int j = t - 2 * H;
        if (j < H) return false;
        int fw2 = kInf, fw1 = kInf, fw0 = kInf;
#pragma unroll
        for (int k = 0; k < kMaxHalf; k++)
            if (k == H - 1) {
                fw2 = w2[k];
                fw1 = w1[k];
                fw0 = w0[k];
            }
        total = (lds.ring[j % kRing][lane] >> 8) + imin(fw2 + f, imin(fw1, fw0 + f));
        return true;
    }
};

// ---- what motion stereo (vg_motion.hpp) and the depth map operations (vg_depth.hpp) share
constexpr double kMinDepth = 0.25;          // MIN_DEPTH (stereo_misc.h:24)
constexpr double kCoordLimit = 16777216.;   // a projected point beyond +-2^24 px is refused

VGS_HD double dmax(double a, double b) { return a < b ? b : a; }   // std::max

VGS_HD bool coord_ok(const double *pt) { return fabs(pt[0]) <= kCoordLimit && fabs(pt[1]) <= kCoordLimit; }   // false for NaN

// filter (depth_map.cpp:32-37)
VGS_HD void fuse(double &v1, double &s1, double v2, double s2)
{
    const double K = 1. / (s1 + s2);
    v1 = (v1 * s2 + v2 * s1) * K;
    s1 = dmax(s1 * s2 * K, 0.05 * v1);
}

}  // namespace vgs
