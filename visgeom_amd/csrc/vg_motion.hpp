// vg_motion.hpp -- motion stereo: the reference's MotionStereo (src/reconstruction/eucm_motion_stereo.cpp) on the device
// functions of vg_stereo_device.hpp (Poly2, Raster, EUCM reconstruct / project, curve index, epipole choice, the four-point
// triangulation, the descriptor and its matching; MIN_DEPTH, the coordinate limit and DepthMap's filter, shared with vg_depth.hpp).
// Two kernels: the gradient mask of the key frames (computeMask) and one lane per (item, depth pixel) through selectPoint,
// computeUncertainty, sampleImage and reconstruct.  Every item has its own StereoGeom in device memory (the pose changes with
// every call).  Evaluated in the order written (-ffp-contract=off), so tests/motion_ref.py agrees bit for bit.
#pragma once

#include "vg_stereo_device.hpp"

namespace vgm {

using namespace vgs;

// status of a depth pixel: the stage that rejected it, or what reconstruct did
enum : int { kRejSelect = 1, kRejUncertainty = 2, kTooCertain = 3, kRejSample = 4, kNotUpdated = 5, kUpdated = 6 };

struct Rec {   // the record of vg_motion_stereo_select, 16 x int32
    int status, gstep, gu2, gv2, su, sv, fu, fv, disp_max, inverted, best, best_cost, index2, pad0, pad1, pad2;
};

// ---------------------------------------------------------------------------------------------------------------------
// computeMask (eucm_motion_stereo.h:109-119): Sobel(ksize 1) in x and y, |gx| + |gy|, GaussianBlur 7 x 7 with sigma 0,
// convertTo u8, threshold to 0 / 128.  Borders BORDER_REFLECT_101 at both stages.  For ksize 7 and sigma 0 OpenCV's
// getGaussianKernel returns a fixed table (1, 3.5, 7, 9, 7, 3.5, 1) / 32; the taps are exact in float and so is every sum
// (inputs <= 510), whatever the order.  The blurred value is rounded half to even.
constexpr int kMaskW = 32, kMaskH = 8, kMaskR = 3;

// Not vgs::reflect101 (vg_image_device.hpp): the mask's halo is fed coordinates up to a whole tile beyond the image, which may be
// several times a small image's side, so the reflection is repeated until it lands inside where the shared form would clamp.
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

// MotionStereo::compute (eucm_motion_stereo.cpp:258-358) for one depth pixel per lane.  The descriptor, its thresholds and
// compareDescriptor's DP are vg_stereo_device.hpp's, as in stereo_curve_cost_kernel; here the samples are the prior's segment
// at step 1, leaving the image rejects the pixel, and a final column goes into the running first minimum.  The positions of
// the best sample and its successor come from a second walk.
__global__ __launch_bounds__(kMatchLanes) void motion_stereo_kernel(MotionArgs a)
{
    __shared__ MatchLds lds;
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
            int resp;
            const int step = compute_descriptor(g, ref, a.img1 + item * img, lds, lane, resp);
            r.gstep = step;
            ref.eps *= step;   // descRasterUncert
            ref.step();
            r.gu2 = ref.u;
            r.gv2 = ref.v;
            if (step != 1 || !(abs(resp) > g.desc_resp_thresh * L)) break;
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
        descriptor_thresholds(lds, L, lane);
        const uint8_t *im2 = a.img2 + item * img;
        const Poly2 &curve = g.table[(int64_t)(g.n_planes + 1) + r.index2];
        const int nSteps = r.disp_max, N = nSteps + L - 1;
        Raster r2;
        r2.init(r.su, r.sv, r.fu, r.fv, curve);
        if (r.inverted) r2.eps *= -1;
        r2.steps(-H);
        MatchDp dp;
        dp.init();
        int best = -1, best_cost = 0x7fffffff;
        const int t_end = nSteps + 3 * H;   // column j = t - 2H is final at time t
        for (int t = 0; t < t_end; t++) {
            if (t < N) {
                if (t > 0) r2.step();
                if (!inside(g, r2.u, r2.v)) {
                    status = kRejSample;
                    break;
                }
                dp.push(lds, lane, H, f, t, im2[(int64_t)r2.v * g.u_max + r2.u]);
            }
            int total;
            if (dp.advance(lds, lane, L, f, t, N, total) && total < best_cost) {   // min_element: the first minimum
                best_cost = total;
                best = t - 2 * H;
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
                double l1, sigma_new;
                if (triangulate_pairs(g, gu, gv, r.gu2, r.gv2, u21, v21, r3.u, r3.v, l1, sigma_new)) {
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
