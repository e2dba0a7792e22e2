// vg_motion.hpp -- motion stereo: the reference's MotionStereo (src/reconstruction/eucm_motion_stereo.cpp) on the device
// functions of vg_stereo.hpp (Poly2, Raster, EUCM reconstruct / project, curve index, epipole choice, regular triangulation).
// Two kernels: the gradient mask of the key frames (computeMask) and one lane per (item, depth pixel) through selectPoint,
// computeUncertainty, sampleImage and reconstruct.  Every item has its own StereoGeom in device memory (the pose changes with
// every call).  Evaluated in the order written (-ffp-contract=off), so tests/motion_ref.py agrees bit for bit.
#pragma once

#include "vg_stereo_device.hpp"

namespace vgm {

using namespace vgs;

// status of a depth pixel: the stage that rejected it, or what reconstruct did
enum : int { kRejSelect = 1, kRejUncertainty = 2, kTooCertain = 3, kRejSample = 4, kNotUpdated = 5, kUpdated = 6 };
constexpr double kMinDepth = 0.25;          // MIN_DEPTH (stereo_misc.h:24)
constexpr double kCoordLimit = 16777216.;   // a projected search end beyond +-2^24 px is refused

struct Rec {   // the record of vg_motion_stereo_select, 16 x int32
    int status, gstep, gu2, gv2, su, sv, fu, fv, disp_max, inverted, best, best_cost, index2, pad0, pad1, pad2;
};

// ---------------------------------------------------------------------------------------------------------------------
// computeMask (eucm_motion_stereo.h:109-119): Sobel(ksize 1) in x and y, |gx| + |gy|, GaussianBlur 7 x 7 with sigma 0,
// convertTo u8, threshold to 0 / 128.  Borders BORDER_REFLECT_101 at both stages.  For ksize 7 and sigma 0 OpenCV's
// getGaussianKernel returns a fixed table (1, 3.5, 7, 9, 7, 3.5, 1) / 32; the taps are exact in float and so is every sum
// (inputs <= 510), whatever the order.  The blurred value is rounded half to even.
constexpr int kMaskW = 32, kMaskH = 8, kMaskR = 3;

VGS_HD int reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

__global__ __launch_bounds__(kMaskW *kMaskH) void motion_mask_kernel(const uint8_t *img, uint8_t *mask, int w, int h, int thresh)
{
    __shared__ int grad[kMaskH + 2 * kMaskR][kMaskW + 2 * kMaskR];
    __shared__ float rows[kMaskH + 2 * kMaskR][kMaskW];
    const float wt[7] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    const uint8_t *im = img + (int64_t)blockIdx.z * w * h;
    const int x0 = blockIdx.x * kMaskW, y0 = blockIdx.y * kMaskH;
    const int tid = threadIdx.y * kMaskW + threadIdx.x;
    constexpr int GW = kMaskW + 2 * kMaskR, GH = kMaskH + 2 * kMaskR;
    for (int i = tid; i < GW * GH; i += kMaskW * kMaskH) {
        const int gx_ = i % GW, gy_ = i / GW;
        const int x = reflect101(x0 + gx_ - kMaskR, w), y = reflect101(y0 + gy_ - kMaskR, h);
        const int64_t row = (int64_t)y * w;
        const int gx = (int)im[row + reflect101(x + 1, w)] - (int)im[row + reflect101(x - 1, w)];
        const int gy = (int)im[(int64_t)reflect101(y + 1, h) * w + x] - (int)im[(int64_t)reflect101(y - 1, h) * w + x];
        grad[gy_][gx_] = abs(gx) + abs(gy);
    }
    __syncthreads();
    for (int i = tid; i < kMaskW * GH; i += kMaskW * kMaskH) {
        const int cx = i % kMaskW, cy = i / kMaskW;
        float s = 0.f;
        for (int k = 0; k < 7; k++) s += wt[k] * (float)grad[cy][cx + k];
        rows[cy][cx] = s;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x < w && y < h) {
        float s = 0.f;
        for (int k = 0; k < 7; k++) s += wt[k] * rows[threadIdx.y + k][threadIdx.x];
        int v = (int)rintf(s);
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        mask[(int64_t)blockIdx.z * w * h + (int64_t)y * w + x] = v > thresh ? 128 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
struct MotionArgs {
    const StereoGeom *geom;                        // DEVICE [n]: the geometry of every item
    const uint8_t *img1, *mask, *img2;             // [n][v_max][u_max]
    const double *depth_in, *sigma_in, *cost_in;   // [n][P], all NULL without a prior
    double *depth, *sigma, *cost;                  // [n][P], all NULL for the stage entry
    Rec *rec;                                      // [n][P] or NULL
    unsigned long long *counts;                    // [n][6] or NULL
    int64_t P;
    int gradient_thresh;
};

constexpr int kMotionLanes = 256;

VGS_HD double dmax(double a, double b) { return a < b ? b : a; }   // std::max

VGS_HD bool coord_ok(const double *pt) { return fabs(pt[0]) <= kCoordLimit && fabs(pt[1]) <= kCoordLimit; }   // false for NaN

// filter (depth_map.cpp:32-37)
VGS_HD void fuse(double &v1, double &s1, double v2, double s2)
{
    const double K = 1. / (s1 + s2);
    v1 = (v1 * s2 + v2 * s1) * K;
    s1 = dmax(s1 * s2 * K, 0.05 * v1);
}

// MotionStereo::compute (eucm_motion_stereo.cpp:258-358) for one depth pixel per lane.  compareDescriptor runs as the one
// stream over the samples that stereo_curve_cost_kernel uses (first half: two columns of history per row; second half: row k
// lagged by 2 k columns; samples and first-half results of the last 32 columns in an LDS ring), at step 1 and with the running
// minimum instead of an error volume.  The positions of the best sample and its successor come from a second walk.
__global__ __launch_bounds__(kMotionLanes) void motion_stereo_kernel(MotionArgs a)
{
    __shared__ int ring[kRing][kMotionLanes];
    __shared__ uint16_t thr[kMaxDesc][kMotionLanes];
    __shared__ uint8_t desc[kMaxDesc][kMotionLanes];
    const int lane = threadIdx.x;
    const int64_t item = blockIdx.y;
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const StereoGeom &g = a.geom[item];
    const int L = g.desc_length, H = L / 2, f = g.flaw_cost;
    const bool live = pix < a.P;
    const int64_t gi = item * a.P + (live ? pix : 0);
    const int64_t img = (int64_t)g.u_max * g.v_max;
    const bool prior = a.depth_in != nullptr;
    Rec r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double dist = 0., sig = 0., cst = (double)g.error_max;
    if (live && prior) {
        dist = a.depth_in[gi];
        sig = a.sigma_in[gi];
        cst = a.cost_in[gi];
    }
    int status = 0;
    const int x = (int)(pix % g.x_max), y = (int)(pix / g.x_max);
    const int gu = x * g.scale + g.u0, gv = y * g.scale + g.v0;
    double X[3];

    // ---- selectPoint
    if (live) {
        status = kRejSelect;
        do {
            if (!inside(g, gu, gv)) break;
            if (a.mask[item * img + (int64_t)gv * g.u_max + gu] < a.gradient_thresh) break;
            if (!eucm_reconstruct(g.c1, (double)gu, (double)gv, X)) break;
            const int flags1 = choose_epipole(g, 0, gu, gv);
            if (flags1 & kEpipoleTooClose) break;
            Raster ref;
            make_raster(g, 0, gu, gv, curve_index(g, X), flags1, ref);
            const uint8_t *im1 = a.img1 + item * img;
            int step = -1, resp = 0;
            const int wave_thresh = g.desc_resp_thresh * L;
            for (int si = 0; si < g.n_scales; si++) {   // EpipolarDescriptor::compute
                const int sc = g.scales[si];
                Raster rr = ref;
                rr.eps *= -sc;
                rr.steps(-H);
                bool border = false;
                for (int i = 0; i < L; i++, rr.step()) {
                    if (!inside(g, rr.u, rr.v)) {
                        border = true;
                        break;
                    }
                    desc[i][lane] = im1[(int64_t)rr.v * g.u_max + rr.u];
                }
                if (border) {
                    step = -1;
                    break;
                }
                int tv = 0;
                for (int i = 1; i < L; i++) tv += abs((int)desc[i - 1][lane] - (int)desc[i][lane]);
                resp = (tv * 100) / ((int)desc[H][lane] + 30);
                step = sc;
                if (abs(resp) > wave_thresh) break;
            }
            r.gstep = step;
            ref.eps *= step;   // descRasterUncert
            ref.step();
            r.gu2 = ref.u;
            r.gv2 = ref.v;
            if (step != 1 || !(abs(resp) > wave_thresh)) break;
            status = 0;
        } while (false);
    }

    // ---- computeUncertainty
    if (live && status == 0) {
        status = kRejUncertainty;
        do {
            double Xr[3], ps[2], pf[2];
            if (dist == 0.) {   // no prior: just rotate
                mat_vec(g.Rinv, X, Xr);
                if (!eucm_project(g.c2, Xr, ps) || !coord_ok(ps)) break;
                r.su = round_int(ps[0]);
                r.sv = round_int(ps[1]);
                const int fl = choose_epipole(g, 1, r.su, r.sv);
                if (fl & kEpipoleTooClose) break;
                const int inv = (fl & kEpipoleInverted) ? 1 : 0;
                r.fu = g.epi_px[1][inv][0];
                r.fv = g.epi_px[1][inv][1];
                if (inv) {
                    r.disp_max = g.disp_max;
                    r.inverted = 1;
                } else {
                    const int du = abs(r.su - r.fu), dv = abs(r.sv - r.fv);
                    r.disp_max = imin(g.disp_max, du > dv ? du : dv);
                }
            } else {
                const double nrm = sqrt(dot3(X, X));
                for (int i = 0; i < 3; i++) X[i] = X[i] / nrm;
                const double d_far = dist + 3 * sig, d_near = dmax(dist - 3 * sig, kMinDepth);
                double Xa[3], Xb[3];
                for (int i = 0; i < 3; i++) {
                    Xa[i] = X[i] * d_far - g.t[i];
                    Xb[i] = X[i] * d_near - g.t[i];
                }
                mat_vec(g.Rinv, Xa, Xr);
                if (!eucm_project(g.c2, Xr, ps) || !coord_ok(ps)) break;
                mat_vec(g.Rinv, Xb, Xr);
                if (!eucm_project(g.c2, Xr, pf) || !coord_ok(pf)) break;
                const int delta = round_int(dmax(fabs(pf[0] - ps[0]), fabs(pf[1] - ps[1])));
                r.disp_max = imin(g.disp_max, delta);
                r.su = round_int(ps[0]);
                r.sv = round_int(ps[1]);
                r.fu = round_int(pf[0]);
                r.fv = round_int(pf[1]);
            }
            r.index2 = curve_index(g, X);   // the curve of camera 2 is looked up by the ray of camera 1 (normalised with a prior)
            status = 0;
        } while (false);
    }
    if (live && status == 0 && r.disp_max < (prior ? 2 : 1)) status = kTooCertain;

    // ---- sampleImage + compareDescriptor + the minimum over [HALF_LENGTH, size - HALF_LENGTH)
    if (live && status == 0) {
        for (int i = 0; i < L; i++) {   // thresholds (compareDescriptor, eucm_stereo.cpp:81-113)
            const int di = desc[i][lane];
            int lo, hi;
            if (i == 0 || i == L - 1) {
                const int dn = desc[i == 0 ? 1 : L - 2][lane];
                const int m = (di + dn) / 2;
                if (di > dn) {
                    lo = m;
                    hi = di;
                } else {
                    hi = m;
                    lo = di;
                }
            } else {
                const int d1 = (di + desc[i - 1][lane]) / 2, d2 = (di + desc[i + 1][lane]) / 2;
                lo = imin(di, imin(d1, d2));
                hi = di > d1 ? (di > d2 ? di : d2) : (d1 > d2 ? d1 : d2);
            }
            thr[i][lane] = (uint16_t)(lo | hi << 8);
        }
        const uint8_t *im2 = a.img2 + item * img;
        const Poly2 &curve = g.table[(int64_t)(g.n_planes + 1) + r.index2];
        const int nSteps = r.disp_max, N = nSteps + L - 1;
        Raster r2;
        r2.init(r.su, r.sv, r.fu, r.fv, curve);
        if (r.inverted) r2.eps *= -1;
        r2.steps(-H);
        int v1[kMaxHalf], v2[kMaxHalf];
        int w0[kMaxHalf], w1[kMaxHalf], w2[kMaxHalf];
#pragma unroll
        for (int i = 0; i < kMaxHalf; i++) {
            v1[i] = v2[i] = kInf;
            w0[i] = w1[i] = w2[i] = kInf;
        }
        int best = -1, best_cost = 0x7fffffff;
        const int t_end = nSteps + 3 * H;
        for (int t = 0; t < t_end; t++) {
            if (t < N) {
                if (t > 0) r2.step();
                if (!inside(g, r2.u, r2.v)) {
                    status = kRejSample;
                    break;
                }
                const int s = im2[(int64_t)r2.v * g.u_max + r2.u];
                int cur = compute_error(s, thr[0][lane]);
#pragma unroll
                for (int i = 1; i <= kMaxHalf; i++) {
                    if (i <= H) {
                        const int nv = imin(cur + f, imin(v1[i - 1], v2[i - 1] + f)) + compute_error(s, thr[i][lane]);
                        v2[i - 1] = v1[i - 1];
                        v1[i - 1] = cur;
                        cur = nv;
                    }
                }
                ring[t % kRing][lane] = cur << 8 | s;
            }
#pragma unroll
            for (int k = 0; k < kMaxHalf; k++) {
                if (k < H) {
                    const int c = t - 2 * k;
                    int val = kInf;
                    if (c >= 0 && c < N) {
                        const int sc = ring[c % kRing][lane] & 255;
                        const int ev = compute_error(sc, thr[L - 1 - k][lane]);
                        if (k == 0) val = ev;
                        else val = imin(w2[k - 1] + f, imin(w1[k - 1], w0[k - 1] + f)) + ev;
                    }
                    w2[k] = w1[k];
                    w1[k] = w0[k];
                    w0[k] = val;
                }
            }
            const int j = t - 2 * H;
            if (j >= H) {
                int fw2 = kInf, fw1 = kInf, fw0 = kInf;
#pragma unroll
                for (int k = 0; k < kMaxHalf; k++)
                    if (k == H - 1) {
                        fw2 = w2[k];
                        fw1 = w1[k];
                        fw0 = w0[k];
                    }
                const int total = (ring[j % kRing][lane] >> 8) + imin(fw2 + f, imin(fw1, fw0 + f));
                if (total < best_cost) {   // min_element: the first minimum
                    best_cost = total;
                    best = j;
                }
            }
        }
        if (status == 0) {
            r.best = best;
            r.best_cost = best_cost;
            status = kNotUpdated;
            // ---- reconstruct
            if (best_cost < g.error_max && (double)best_cost < 2 * cst) {
                Raster r3;
                r3.init(r.su, r.sv, r.fu, r.fv, curve);
                if (r.inverted) r3.eps *= -1;
                r3.steps(-H);
                r3.steps(best);
                const int u21 = r3.u, v21 = r3.v;
                r3.step();
                double p1[3], p2[3], q1[3], q2[3];
                if (eucm_reconstruct(g.c1, (double)gu, (double)gv, p1) && eucm_reconstruct(g.c1, (double)r.gu2, (double)r.gv2, p2) &&
                    eucm_reconstruct(g.c2, (double)u21, (double)v21, q1) && eucm_reconstruct(g.c2, (double)r3.u, (double)r3.v, q2)) {
                    const double pn = sqrt(dot3(p1, p1));
                    const double l1 = triangulate_lambda(g.R, g.t, p1, q1) * pn;
                    const double l2 = triangulate_lambda(g.R, g.t, p2, q2) * pn;
                    const double sigma_new = fabs(l2 - l1);
                    if (dist != 0.) {
                        fuse(dist, sig, l1, sigma_new);
                        cst = cst * 0.7 + best_cost * 0.3;
                    } else {
                        dist = l1;
                        sig = sigma_new;
                        cst = (double)best_cost;
                    }
                    status = kUpdated;
                }
            }
        }
    }

    if (live) {
        if (a.depth) {
            a.depth[gi] = dist;
            a.sigma[gi] = sig;
            a.cost[gi] = cst;
        }
        if (a.rec) {
            r.status = status;
            a.rec[gi] = r;
        }
    }
    if (a.counts) {   // every lane of the block arrives here: one atomic per wave and counter
        for (int k = 1; k <= 6; k++) {
            const bool hit = live && (k == 5 ? status >= kNotUpdated : (k == 6 ? status == kUpdated : status == k));
            const int c = __popcll(__ballot(hit));
            if ((lane & 63) == 0 && c) atomicAdd(a.counts + item * 6 + (k - 1), (unsigned long long)c);
        }
    }
}

}  // namespace vgm
