// vg_photometric.hpp -- photometric pose estimation against a depth key frame: BinaryScalSpace with gradients
// (include/localization/scale_space.h), ScalePhotometric::initPhotometricData (src/localization/photometric.cpp:46-93) and
// PhotometricCostFunction::Evaluate with lossFunction / getUMapgin / getVMapgin (src/localization/local_cost_functions.cpp:35-210)
// on the EUCM device functions of vg_camera.hpp and vg_stereo_device.hpp.  A pyramid level is a gather (every output pixel sums
// its own sources in the reference's raster order), the data pack is compacted in raster order with a prefix sum, and the cost
// kernel fuses residual, Jacobian row and the 28 sums of [J | r]^T [J | r] per (pose, point): FP64 wave butterflies, per-workgroup
// partials, a second pass that adds the partials in index order -- no floating-point atomics, the same bits on every run.
// DESIGN.md section 5.13.
#pragma once

#include "vg_bicubic.hpp"
#include "vg_compact.hpp"
#include "vg_photometric_row.hpp"

namespace vgp {

using namespace vgs;

constexpr int kLanes = 256, kWaves = kLanes / 64;
constexpr int kMaxLevels = 8;            // levels 0 .. 7: the sums of a level stay exact in float
constexpr double kGradThresh = 250.;     // GRAD_THRESH (photometric.h:100)
constexpr double kDistMax = 50.;         // DIST_MAX (:102)
constexpr double kGreyMax = 240.;        // photometric.cpp:74
constexpr double kLossFactor = 3.;       // LOSS_FACTOR (local_cost_functions.h:78)
constexpr double kMarginPixels = 50.;    // MARGIN_SIZE = 50 / scale (local_cost_functions.cpp:43)

// ---- pyramid (level 0 of n images: u8_to_float_kernel) ----------------------------------------------------------------

// BinaryScalSpace::propagate (scale_space.h:121-132) for one level of n images, as a gather: source row v goes to
// min(round(v / 2.), h - 1) (round half away: rows 2 vs - 1 and 2 vs, row 0 alone, the last row takes the rest), source column
// u to min(u / 2, w - 1).  The sources are added in the reference's order (v ascending, u ascending), then * 0.25.
__global__ __launch_bounds__(kLanes) void photo_down_kernel(float *pyr, int64_t item_stride, int64_t off_prev, int wp, int hp, int64_t off,
                                                           int w, int h)
{
    const int64_t pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= (int64_t)w * h) return;
    const int us = (int)(pix % w), vs = (int)(pix / w);
    const int v_lo = vs == 0 ? 0 : 2 * vs - 1, v_hi = vs == h - 1 ? hp - 1 : 2 * vs;
    const int u_lo = 2 * us, u_hi = us == w - 1 ? wp - 1 : 2 * us + 1;
    const float *src = pyr + blockIdx.y * item_stride + off_prev;
    float acc = 0.f;
    for (int v = v_lo; v <= v_hi; v++)
        for (int u = u_lo; u <= u_hi; u++) acc += src[(int64_t)v * wp + u];
    pyr[blockIdx.y * item_stride + off + pix] = acc * 0.25f;
}

// the Sobel / 8 pair (sobel8_at) of every pixel of one level of n images
__global__ __launch_bounds__(kLanes) void photo_sobel_kernel(const float *img, float *gu, float *gv, int64_t item_stride, int w, int h)
{
    const int64_t pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= (int64_t)w * h) return;
    float fu, fv;
    sobel8_at(img + blockIdx.y * item_stride, w, h, (int)(pix % w), (int)(pix / w), fu, fv);
    gu[blockIdx.y * item_stride + pix] = fu;
    gv[blockIdx.y * item_stride + pix] = fv;
}

// ---- the data pack ---------------------------------------------------------------------------------------------------

struct SelectArgs {
    const float *img, *gu, *gv;   // the base level
    int w, h, level_scale;        // level_scale = 1 << scale_idx (BinaryScalSpace::uConv)
    double cam[6];
    Grid g;
    const double *depth;          // [y_max][x_max]
    double Rb[9], tb[3];          // xi_base_cam: rotMat, trans
    unsigned *block_counts;       // [blocks]
    const unsigned *block_offsets;
    int32_t *idx;                 // the pack, filled by the second pass
    double *val, *cloud;
};

// initPhotometricData's tests in its order, then DepthMap::reconstruct (depth_map.cpp:486-505) and _xiBaseCam.transform
VGS_HD bool select_point(const SelectArgs &a, int64_t pix, double &value, double *X)
{
    const double gu = a.gu[pix], gv = a.gv[pix];
    if (gu * gu + gv * gv < kGradThresh) return false;
    const int us = (int)(pix % a.w), vs = (int)(pix / a.w);
    const int ub = us * a.level_scale, vb = vs * a.level_scale;
    const int xd = round_int(((double)ub - a.g.u0) / a.g.scale), yd = round_int(((double)vb - a.g.v0) / a.g.scale);   // DepthMap::nearest
    const bool valid = xd >= 0 && xd < a.g.x_max && yd >= 0 && yd < a.g.y_max;
    const double d = valid ? a.depth[(int64_t)yd * a.g.x_max + xd] : 0.;
    if (d > kDistMax || d == 0.) return false;
    value = a.img[pix];
    if (value > kGreyMax) return false;
    double Xr[3], Xd[3];
    if (!eucm_reconstruct(a.cam, (double)ub, (double)vb, Xr)) return false;
    if (d < kMinDepth) return false;
    const double nrm = sqrt(dot3(Xr, Xr));
    for (int i = 0; i < 3; i++) Xd[i] = Xr[i] / nrm * d;
    mat_vec(a.Rb, Xd, X);
    for (int i = 0; i < 3; i++) X[i] = X[i] + a.tb[i];
    return true;
}

// pass 1 (WRITE = false): the survivors of every block of 256 pixels; pass 2: their raster-ordered places from the scanned
// block counts (vgc::block_place)
template <bool WRITE>
__global__ __launch_bounds__(kLanes) void photo_select_kernel(SelectArgs a)
{
    const int64_t pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double value = 0., X[3] = {0., 0., 0.};
    const bool keep = pix < (int64_t)a.w * a.h && select_point(a, pix, value, X);
    const unsigned pos = vgc::block_place<WRITE, kLanes>(keep, blockIdx.x, a.block_counts, a.block_offsets);
    if (!WRITE || !keep) return;
    a.idx[pos] = (int32_t)pix;
    a.val[pos] = value;
    for (int i = 0; i < 3; i++) a.cloud[3 * (int64_t)pos + i] = X[i];
}

// ---- the cost --------------------------------------------------------------------------------------------------------

// what one pose brings: xiCam = xi o xi_base_cam (rotMatInv, trans) and CameraJacobian(camera, xi, xi_base_cam)'s L11 | L12 | L22
struct PoseFrame {
    double Rinv[9], t[3], L11[9], L12[9], L22[9];
    int target, active;
};

struct EvalArgs {
    const PoseFrame *frames;   // DEVICE [n]
    const float *targets;      // the target pyramids
    int64_t target_stride, level_off;
    int w, h;                  // the level
    double inv_scale, margin;  // 1. / scale, 50. / scale
    double cam[6];
    const double *val, *cloud; // the pack of the level
    int m, blocks;
    double *res, *jac;         // [n][m], [n][m][6] or NULL
    double *partials;          // [n][blocks][kSums]
};

// getUMapgin / getVMapgin (local_cost_functions.cpp:66-92)
VGS_HD double margin_of(double x, double inv_scale, double margin, int size)
{
    const double xs = x * inv_scale;
    if (xs < margin) return xs - margin;
    if (xs > size - margin - 1) return xs - size + margin + 1;
    return 0.;
}

// lossFunction (:50-59); sign(0) = -1 (std.h:74), rho(0) = 0 either way
VGS_HD void loss(double x, double &rho, double &drhodx)
{
    const double s = 0.1 * sgn(x);
    const double arg = -fabs(x) / kLossFactor;
    const double e = arg > -5 ? exp(-fabs(x) / kLossFactor) : 0;
    rho = s * kLossFactor * (1. - e);
    drhodx = 0.1 * e;
}

// PhotometricCostFunction::Evaluate for point i under one pose: the residual and its row.  A point that does not project, or
// projects into the margin (the reference multiplies residual and row by 0 there), gives a zero residual and a zero row.
VGS_HD void eval_point(const EvalArgs &a, const PoseFrame &fr, int64_t i, double &r, double *row)
{
    r = 0.;
    for (int k = 0; k < 6; k++) row[k] = 0.;
    double Xd[3], X[3];
    for (int k = 0; k < 3; k++) Xd[k] = a.cloud[3 * i + k] - fr.t[k];   // xiCam.inverseTransform
    mat_vec(fr.Rinv, Xd, X);
    vg::CornerEval<6> e;
    vg::eval_corner<vg::kEUCM, true, false>(a.cam, X[0], X[1], X[2], e);
    const double pt[2] = {e.u, e.v};
    // a projection that is not finite or lies beyond +-2^24 px counts as failed: the reference would convert it to int
    if (!(e.ok && coord_ok(pt) && margin_of(pt[0], a.inv_scale, a.margin, a.w) == 0. && margin_of(pt[1], a.inv_scale, a.margin, a.h) == 0.)) return;
    double f, dfdr, dfdc;
    bicubic(a.targets + fr.target * a.target_stride + a.level_off, a.w, a.h, pt[1] * a.inv_scale, pt[0] * a.inv_scale, f, dfdr, dfdc);
    const double g0 = dfdc * a.inv_scale, g1 = dfdr * a.inv_scale;   // grad = (d/du, d/dv), normalised by the scale
    double drho;
    loss(f - a.val[i], r, drho);
    double d[3];
    dfdxi_row(X, e.P, g0, g1, fr.L11, fr.L12, fr.L22, d, row);
    for (int k = 0; k < 6; k++) row[k] = row[k] * drho;   // times drhoderr, on the finished sums
}

// one lane per (pose, point): blockIdx.y the pose, blockIdx.x * 256 + threadIdx.x the point
__global__ __launch_bounds__(kLanes) void photo_eval_kernel(EvalArgs a)
{
    const int pose = blockIdx.y;
    const PoseFrame &fr = a.frames[pose];
    if (!fr.active) return;   // uniform over the workgroup: a converged pose of compute_pose
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double r = 0., row[6] = {0., 0., 0., 0., 0., 0.};
    if (i < a.m) {
        eval_point(a, fr, i, r, row);
        if (a.res) a.res[(int64_t)pose * a.m + i] = r;
        if (a.jac)
#pragma unroll
            for (int k = 0; k < 6; k++) a.jac[((int64_t)pose * a.m + i) * 6 + k] = row[k];
    }
    if (!a.partials) return;
    double s[kSums];
    row_products(row, r, s);
    block_sums<kSums, kLanes>(s, a.partials + ((int64_t)pose * a.blocks + blockIdx.x) * kSums);
}

// the second pass: the partials of a pose in index order, one lane per sum
__global__ __launch_bounds__(64) void photo_reduce_kernel(const PoseFrame *frames, const double *partials, int blocks, double *sums)
{
    const int pose = blockIdx.x, k = threadIdx.x;
    if (k >= kSums || !frames[pose].active) return;
    double s = 0.;
    for (int b = 0; b < blocks; b++) s += partials[((int64_t)pose * blocks + b) * kSums + k];
    sums[(int64_t)pose * kSums + k] = s;
}

}  // namespace vgp
