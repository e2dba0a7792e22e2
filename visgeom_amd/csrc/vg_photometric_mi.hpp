// vg_photometric_mi.hpp -- the mutual-information cost of photometric localization: MutualInformation::Evaluate with
// computeShares / computeShareDerivative / computeHist / computeHist2d / reduceHist (src/localization/cost_function_mi.cpp:35-289)
// at the settings of ScalePhotometric::computePoseMI (src/localization/photometric.cpp:260-321: 8 bins, valMax 255), on the data
// packs, pose frames, EUCM projection and bicubic sampler of vg_photometric.hpp.  The gradient of a point needs the finished
// histogram of its pose, so one evaluation is four launches on the handle's stream: sample + histogram (a wave walks its 64
// points in point order, lane b owns bin b), a per-pose kernel that adds the workgroups' histograms in workgroup order and forms
// hist2, logVec12 and the cost, the gradient (the point is recomputed, not stored: DESIGN.md section 5.14), and the ordered sum
// of the gradient partials.  No floating-point atomics: the same bits on every run and in every batch.  The second half of the
// file is the host side of computePoseMI: the odometry term of MutualInformationOdom and a BFGS with a strong-Wolfe line search
// written as a state machine, so that every pose of a batch proposes one trial per launch.
#pragma once

#include <cmath>
#include <cstring>

#include "../../include/visgeom_amd.h"
#include "vg_photometric.hpp"

namespace vgp {

constexpr int kMiBins = 8, kMiCells = kMiBins * kMiBins;   // computePoseMI: numBins 8
constexpr double kMiValMax = 255.;                        // valMax
constexpr double kMiHistStep = kMiValMax / (kMiBins - 1); // _histStep
constexpr int kMiOut = 72;                                // per pose: hist12 [64] | cost | gradient [6] | unused
static_assert(kMiCells == 64, "lane b owns bin b: the joint histogram has to fill exactly one wave");

// computeShares and computeShareDerivative (cost_function_mi.cpp:146-216) in one: idx1 = round(val / histStep) half away from
// zero, share = 1 - 2 tail^2, der = -+4 tail / histStep, the neighbour by the sign of the remainder (none at bins 0 and 7 on
// their outer side); below bin 0 and from bin 8 on the index is clamped, share = der = 0 and there is no neighbour (i2 = -1)
VGS_HD void mi_shares(double val, int &i1, int &i2, double &share, double &der)
{
    const double sv = val / kMiHistStep;
    const double r = round(sv);
    const double tail = fabs(r - sv);
    i2 = -1;
    share = der = 0.;
    if (r < 0.) {
        i1 = 0;
    } else if (r >= (double)kMiBins) {
        i1 = kMiBins - 1;
    } else {
        i1 = (int)r;
        share = 1. - 2 * tail * tail;
        if (sv > r && i1 < kMiBins - 1) {
            i2 = i1 + 1;
            der = -(4 * tail / kMiHistStep);
        } else if (sv < r && i1 > 0) {
            i2 = i1 - 1;
            der = 4 * tail / kMiHistStep;
        }
    }
}

// what a point puts on one axis of a histogram: weight a0 on bin i1 and 1 - a0 on bin i2; without a neighbour the whole
// increment goes to i1 whatever the share is (the last branches of computeHist and computeHist2d)
VGS_HD double mi_axis_weight(int i2, double share) { return i2 < 0 ? 1. : share; }

// a lane value read by every lane of the wave; j is uniform (an unrolled loop counter), all 64 lanes are active
__device__ inline int mi_lane_read(int v, int j) { return __builtin_amdgcn_readlane(v, j); }
__device__ inline double mi_lane_read(double v, int j)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// the weight lane bin `b` receives from a point with bins (i1, i2 + 1 packed as pk & 15, pk >> 4) and first weight a0
__device__ inline double mi_bin_weight(int b, int pk, double a0)
{
    const int i1 = pk & 15, i2 = ((pk >> 4) & 15) - 1;
    return b == i1 ? a0 : (b == i2 ? 1. - a0 : 0.);
}

// ---- _hist1: the key frame's histogram, once per set_base and scale -------------------------------------------------------

// computeHist over the pack in point order: lane b (mod 8) owns bin b, a wave walks its 64 points, the waves of a workgroup
// are added in wave order.  count (DEVICE): the pack's size, known on the device only while set_base runs; the grid covers
// the level's pixels, workgroups past the pack write zeros.
__global__ __launch_bounds__(kLanes) void mi_hist1_kernel(const double *val, const unsigned *count, double *partials)
{
    __shared__ double wave_hist[kWaves][kMiBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = *count, i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    const double inc = m > 0 ? 1. / (double)m : 0.;
    int pk = 0;
    double a0 = 0.;
    if (i < m) {
        int i1, i2;
        double share, der;
        mi_shares(val[i], i1, i2, share, der);
        pk = i1 | (i2 + 1) << 4;
        a0 = mi_axis_weight(i2, share);
    } else {
        pk = 15;   // no bin
    }
    double acc = 0.;
#pragma unroll
    for (int j = 0; j < 64; j++) acc += inc * mi_bin_weight(lane & 7, mi_lane_read(pk, j), mi_lane_read(a0, j));
    if (lane < kMiBins) wave_hist[wave][lane] = acc;
    __syncthreads();
    if (threadIdx.x < kMiBins) {
        const int k = threadIdx.x;
        partials[(int64_t)blockIdx.x * kMiBins + k] = ((wave_hist[0][k] + wave_hist[1][k]) + wave_hist[2][k]) + wave_hist[3][k];
    }
}

// the workgroups' histograms in workgroup order
__global__ __launch_bounds__(64) void mi_hist1_reduce_kernel(const double *partials, int blocks, double *hist1)
{
    const int k = threadIdx.x;
    if (k >= kMiBins) return;
    double s = 0.;
    for (int b = 0; b < blocks; b++) s += partials[(int64_t)b * kMiBins + k];
    hist1[k] = s;
}

// ---- the cost --------------------------------------------------------------------------------------------------------

struct MiArgs {
    const PoseFrame *frames;   // DEVICE [n]
    const float *targets;      // the target pyramids
    int64_t target_stride, level_off;
    int w, h;                  // the level
    double inv_scale;          // 1. / scale
    double cam[6];
    const double *val, *cloud; // the pack of the level
    const double *hist1;       // DEVICE [8]: _hist1 of the level
    int m, blocks;
    double increment;          // 1. / m
    double *values;            // DEVICE [n][m] or NULL: valVec2
    double *hist_partials;     // DEVICE [n][blocks][64]
    double *grad_partials;     // DEVICE [n][blocks][6]
    double *logv;              // DEVICE [n][64]: logVec12
    double *out;               // DEVICE [n][kMiOut]
};

// the loop body of MutualInformation::Evaluate for point i under one pose: the sampled grey f (0 when projectPoint fails: the
// point is still counted, in bin 0 of the second axis) and, with ROW, CameraJacobian::dfdxi of the image gradient / scale
// (zero for a failed point).  There is no margin test: a point that projects is sampled through the clamping grid wherever
// it lands.  A projection that is not finite or lies beyond +-2^24 px counts as failed, as in eval_point.
template <bool ROW>
VGS_HD void mi_point(const MiArgs &a, const PoseFrame &fr, int64_t i, double &f, double *row)
{
    f = 0.;
    if (ROW)
        for (int k = 0; k < 6; k++) row[k] = 0.;
    double Xd[3], X[3];
    for (int k = 0; k < 3; k++) Xd[k] = a.cloud[3 * i + k] - fr.t[k];   // xiCam.inverseTransform
    mat_vec(fr.Rinv, Xd, X);
    vg::CornerEval<6> e;
    vg::eval_corner<vg::kEUCM, true, false>(a.cam, X[0], X[1], X[2], e);
    const double pt[2] = {e.u, e.v};
    if (!(e.ok && coord_ok(pt))) return;
    double dfdr, dfdc;
    bicubic(a.targets + fr.target * a.target_stride + a.level_off, a.w, a.h, pt[1] * a.inv_scale, pt[0] * a.inv_scale, f, dfdr, dfdc);
    if (!ROW) return;
    const double g0 = dfdc * a.inv_scale, g1 = dfdr * a.inv_scale;   // grad = (d/du, d/dv), normalised by the scale
    double d[3];
    dfdxi_row(X, e.P, g0, g1, fr.L11, fr.L12, fr.L22, d, row);
}

// launch 1, one lane per (pose, point): valVec2 and computeHist2d.  Lane b of a wave owns bin b = idx2 * 8 + idx1 and the wave
// walks its 64 points in point order -- the reference's summation order inside a wave; a point's (<= 2) x (<= 2) bins and two
// weights reach the lanes as three lane reads.  The product is (increment * w1) * w2 in every case.
__global__ __launch_bounds__(kLanes) void mi_hist_kernel(MiArgs a)
{
    __shared__ double wave_hist[kWaves][kMiCells];
    const int pose = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PoseFrame &fr = a.frames[pose];
    if (!fr.active) return;   // uniform over the workgroup: a finished pose of compute_pose_mi
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    int pk = 0xffff;          // past the pack: no bin on either axis
    double a0 = 0., b0 = 0.;
    if (i < a.m) {
        double f, der, s1, s2;
        int i11, i12, i21, i22;
        mi_point<false>(a, fr, i, f, nullptr);
        if (a.values) a.values[(int64_t)pose * a.m + i] = f;
        mi_shares(a.val[i], i11, i12, s1, der);
        mi_shares(f, i21, i22, s2, der);
        pk = i11 | (i12 + 1) << 4 | i21 << 8 | (i22 + 1) << 12;
        a0 = mi_axis_weight(i12, s1);
        b0 = mi_axis_weight(i22, s2);
    }
    const int b1 = lane & 7, b2 = lane >> 3;
    double acc = 0.;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const int pj = mi_lane_read(pk, j);
        acc += (a.increment * mi_bin_weight(b1, pj, mi_lane_read(a0, j))) * mi_bin_weight(b2, pj >> 8, mi_lane_read(b0, j));
    }
    wave_hist[wave][lane] = acc;
    __syncthreads();
    if (threadIdx.x < kMiCells) {
        const int k = threadIdx.x;
        a.hist_partials[((int64_t)pose * a.blocks + blockIdx.x) * kMiCells + k] =
            ((wave_hist[0][k] + wave_hist[1][k]) + wave_hist[2][k]) + wave_hist[3][k];
    }
}

// launch 2, one wave per pose: the workgroups' histograms in workgroup order, reduceHist (a row's eight entries from the
// left), logVec12 (0 where p12 == 0) and the cost, subtracted bin after bin like the reference's double loop
__global__ __launch_bounds__(64) void mi_finish_kernel(MiArgs a)
{
    __shared__ double terms[kMiCells];
    const int pose = blockIdx.x, b = threadIdx.x;
    if (!a.frames[pose].active) return;
    double p = 0.;
    for (int k = 0; k < a.blocks; k++) p += a.hist_partials[((int64_t)pose * a.blocks + k) * kMiCells + b];
    double h2 = 0.;
#pragma unroll
    for (int k = 0; k < kMiBins; k++) h2 += __shfl(p, (b & ~7) + k, 64);
    const double l = p > 0. ? log(p / (h2 * a.hist1[b & 7])) : 0.;
    a.logv[(int64_t)pose * kMiCells + b] = l;
    a.out[(int64_t)pose * kMiOut + b] = p;
    terms[b] = p > 0. ? p * l : 0.;
    __syncthreads();
    if (b == 0) {
        double c = 0.;
        for (int k = 0; k < kMiCells; k++) c -= terms[k];
        a.out[(int64_t)pose * kMiOut + kMiCells] = c;
    }
}

// launch 3, one lane per (pose, point): dMIdf * dfdxi of the point, the six sums by the ordered reduction of
// photo_eval_kernel (vgs::block_sums).  The point is projected and sampled again.
__global__ __launch_bounds__(kLanes) void mi_grad_kernel(MiArgs a)
{
    __shared__ double logv[kMiCells];
    const int pose = blockIdx.y;
    const PoseFrame &fr = a.frames[pose];
    if (!fr.active) return;   // uniform over the workgroup, in front of both barriers
    if (threadIdx.x < kMiCells) logv[threadIdx.x] = a.logv[(int64_t)pose * kMiCells + threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double s[6] = {0., 0., 0., 0., 0., 0.};
    if (i < a.m) {
        double f, row[6], dPdf, share1, unused;
        int i11, i12, i21, i22;
        mi_point<true>(a, fr, i, f, row);
        mi_shares(f, i21, i22, unused, dPdf);
        mi_shares(a.val[i], i11, i12, share1, unused);
        double dMIdP = 0.;
        if (i22 != -1) {
            if (i12 != -1)
                dMIdP = logv[i21 * kMiBins + i11] * share1 + logv[i21 * kMiBins + i12] * (1 - share1) - logv[i22 * kMiBins + i11] * share1 -
                        logv[i22 * kMiBins + i12] * (1 - share1);
            else
                dMIdP = logv[i21 * kMiBins + i11] - logv[i22 * kMiBins + i11];
        }
        const double dMIdf = dMIdP * a.increment * dPdf;
#pragma unroll
        for (int k = 0; k < 6; k++) s[k] = dMIdf * row[k];
    }
    block_sums<6, kLanes>(s, a.grad_partials + ((int64_t)pose * a.blocks + blockIdx.x) * 6);
}

// launch 4: the gradient partials of a pose in workgroup order; dMIdxi -= ... makes the sum negative
__global__ __launch_bounds__(64) void mi_grad_reduce_kernel(MiArgs a)
{
    const int pose = blockIdx.x, k = threadIdx.x;
    if (k >= 6 || !a.frames[pose].active) return;
    double s = 0.;
    for (int b = 0; b < a.blocks; b++) s += a.grad_partials[((int64_t)pose * a.blocks + b) * 6 + k];
    a.out[(int64_t)pose * kMiOut + kMiCells + 1 + k] = -s;
}

// ---- host: the odometry term and the quasi-Newton solve ------------------------------------------------------------------

// MutualInformationOdom (cost_function_mi.cpp:292-368): DAMPING err (C / 2) err^T on the cost and DAMPING err J on the
// gradient, err = xiPrior^-1 o xi as a row.  C and J row-major 6 x 6, C already halved.
struct MiOdometry {
    double C[36], J[36], prior[6];
};
constexpr double kMiDamping = 0.0002;

// the constructor; R = xiPrior.rotMatInv(), M = interOmegaRot(xiPrior.rot()), both row-major 3 x 3
inline void mi_odometry_init(MiOdometry &o, const double *xi_odom, const double *xi_prior, const double *R, const double *M)
{
    const double errV = 0.1, errW = 0.01, lambdaT = 0.01, lambdaR = 0.01;   // the defaults of cost_function_mi.h:104-107
    const double delta = xi_odom[5], l = std::sqrt(xi_odom[0] * xi_odom[0] + xi_odom[1] * xi_odom[1] + xi_odom[2] * xi_odom[2]);
    const double s = std::sin(delta / 2.), c = std::cos(delta / 2.), l2 = l / 2.;
    const double dfdu[3][2] = {{s, -l2 * c}, {c, l2 * s}, {0., 1.}};
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
    double C[36] = {0.};
    for (int r = 0; r < 2; r++) {
        for (int q = 0; q < 2; q++) C[6 * r + q] = Ci[3 * r + q];
        C[6 * r + 5] = Ci[3 * r + 2];
        C[6 * 5 + r] = Ci[3 * 2 + r];
    }
    C[6 * 5 + 5] = Ci[8];
    C[6 * 2 + 2] = 1 / (lambdaT * lambdaT);
    C[6 * 3 + 3] = C[6 * 4 + 4] = 1 / (lambdaR * lambdaR);
    double RM[9];
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) RM[3 * r + q] = R[3 * r] * M[q] + R[3 * r + 1] * M[3 + q] + R[3 * r + 2] * M[6 + q];
    for (int br = 0; br < 2; br++)       // every 3 x 3 block of C times R (left column) or R M (right column)
        for (int bc = 0; bc < 2; bc++) {
            const double *T = bc ? RM : R;
            for (int r = 0; r < 3; r++)
                for (int q = 0; q < 3; q++) {
                    double v = 0.;
                    for (int k = 0; k < 3; k++) v += C[6 * (3 * br + r) + 3 * bc + k] * T[3 * k + q];
                    o.J[6 * (3 * br + r) + 3 * bc + q] = v;
                }
        }
    for (int k = 0; k < 36; k++) o.C[k] = 0.5 * C[k];
    std::memcpy(o.prior, xi_prior, sizeof o.prior);
}

// err = xiPrior^-1 o xi (HOST [6], from the caller's inverse_compose); gradient may be NULL: the reference writes to it
// untested, here the gradient term is added only when a gradient is asked for
inline void mi_odometry_add(const MiOdometry &o, const double *err, double *cost, double *gradient)
{
    double q = 0.;
    for (int r = 0; r < 6; r++) {
        double v = 0.;
        for (int k = 0; k < 6; k++) v += o.C[6 * r + k] * err[k];
        q += err[r] * v;
    }
    *cost += kMiDamping * q;
    for (int i = 0; gradient && i < 6; i++) {
        double v = 0.;
        for (int k = 0; k < 6; k++) v += err[k] * o.J[6 * k + i];
        gradient[i] += v * kMiDamping;
    }
}

// BFGS with a strong-Wolfe line search (Nocedal & Wright, algorithms 3.5 and 3.6, cubic interpolation 3.59) for one pose, as a
// state machine: trial() is the pose to evaluate next, consume() takes cost and gradient there.  The inverse Hessian starts at
// the identity, the first step length is min(1, 1 / max|g|) and 1 afterwards, a search spends at most 20 evaluations, the
// update is skipped when s^T y <= 0.
struct MiBfgs {
    static constexpr double kC1 = 1e-4, kC2 = 0.9;
    static constexpr int kMaxSearchEvals = 20;
    double ftol = 1e-2, gtol = 1e-3;
    int max_iterations = 50;
    double x[6], f = 0., g[6], H[36], d[6];
    double phi0 = 0., dphi0 = 0.;                        // the search: phi(alpha) = f(x + alpha d)
    double alpha = 0., a_prev = 0., phi_prev = 0., dphi_prev = 0.;
    double a_lo = 0., phi_lo = 0., dphi_lo = 0., a_hi = 0., phi_hi = 0., dphi_hi = 0.;
    double xt[6];
    int evals = 0, iterations = 0, term = VG_TERM_NO_CONVERGENCE;
    bool zoom = false, done = false, started = false;
    double initial_cost = 0.;

    static double max_abs(const double *v)
    {
        double m = 0.;
        for (int k = 0; k < 6; k++) m = std::fmax(m, std::fabs(v[k]));
        return m;
    }
    void start(const double *x0)
    {
        std::memcpy(x, x0, sizeof x);
        std::memcpy(xt, x0, sizeof xt);
        for (int k = 0; k < 36; k++) H[k] = k % 7 == 0 ? 1. : 0.;
        done = started = zoom = false;
        iterations = evals = 0;
        term = VG_TERM_NO_CONVERGENCE;
    }
    const double *trial() const { return xt; }
    bool trial_finite() const
    {
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(xt[k])) return false;
        return true;
    }
    void finish(int t)
    {
        term = t;
        done = true;
    }
    void set_trial(double a)
    {
        alpha = a;
        for (int k = 0; k < 6; k++) xt[k] = x[k] + a * d[k];
    }
    // a new search from x along -H g (steepest descent when that is no descent direction)
    void begin_search()
    {
        if (iterations >= max_iterations) return finish(VG_TERM_NO_CONVERGENCE);
        double gd = 0.;
        for (int r = 0; r < 6; r++) {
            d[r] = 0.;
            for (int k = 0; k < 6; k++) d[r] -= H[6 * r + k] * g[k];
            gd += g[r] * d[r];
        }
        if (!(gd < 0.)) {
            for (int k = 0; k < 36; k++) H[k] = k % 7 == 0 ? 1. : 0.;
            gd = 0.;
            for (int k = 0; k < 6; k++) {
                d[k] = -g[k];
                gd -= g[k] * g[k];
            }
        }
        phi0 = f;
        dphi0 = gd;
        a_prev = 0.;
        phi_prev = phi0;
        dphi_prev = dphi0;
        evals = 0;
        zoom = false;
        set_trial(iterations == 0 ? std::fmin(1., 1. / max_abs(g)) : 1.);
    }
    // the minimiser of the cubic through (a, fa, da) and (b, fb, db), kept a tenth of the interval away from both ends; the
    // midpoint when the cubic has none there or a value is not finite
    static double interpolate(double a, double fa, double da, double b, double fb, double db)
    {
        const double mid = 0.5 * (a + b), lo = std::fmin(a, b), hi = std::fmax(a, b), w = hi - lo;
        const double d1 = da + db - 3. * (fa - fb) / (a - b);
        const double rad = d1 * d1 - da * db;
        if (!(rad >= 0.) || !std::isfinite(rad)) return mid;
        const double d2 = (b > a ? 1. : -1.) * std::sqrt(rad);
        const double t = b - (b - a) * (db + d2 - d1) / (db - da + 2. * d2);
        if (!std::isfinite(t) || t < lo + 0.1 * w || t > hi - 0.1 * w) return mid;
        return t;
    }
    void zoom_trial()
    {
        zoom = true;
        if (evals >= kMaxSearchEvals) return finish(VG_TERM_FAILURE);
        set_trial(interpolate(a_lo, phi_lo, dphi_lo, a_hi, phi_hi, dphi_hi));
    }
    // the step to x + alpha d is taken: the update, the tests, the next search
    void accept(double fn, const double *gn)
    {
        double s[6], y[6], sy = 0.;
        for (int k = 0; k < 6; k++) {
            s[k] = xt[k] - x[k];
            y[k] = gn[k] - g[k];
            sy += s[k] * y[k];
        }
        if (sy > 0.) {   // H = (I - rho s y^T) H (I - rho y s^T) + rho s s^T
            const double rho = 1. / sy;
            double Hy[6], yHy = 0.;
            for (int r = 0; r < 6; r++) {
                Hy[r] = 0.;
                for (int k = 0; k < 6; k++) Hy[r] += H[6 * r + k] * y[k];
            }
            for (int k = 0; k < 6; k++) yHy += y[k] * Hy[k];
            for (int r = 0; r < 6; r++)
                for (int q = 0; q < 6; q++) H[6 * r + q] += -rho * (s[r] * Hy[q] + Hy[r] * s[q]) + (rho * rho * yHy + rho) * s[r] * s[q];
        }
        const double f_old = f;
        std::memcpy(x, xt, sizeof x);
        std::memcpy(g, gn, sizeof g);
        f = fn;
        iterations++;
        if (max_abs(g) <= gtol) return finish(VG_TERM_CONVERGENCE_GRADIENT);
        if (std::fabs(f - f_old) <= ftol * std::fabs(f_old)) return finish(VG_TERM_CONVERGENCE_FUNCTION);
        begin_search();
    }
    // cost and gradient at trial(); ok = false: the trial pose was not finite (nothing was evaluated) or its cost is not
    void consume(double ft, const double *gt, bool ok)
    {
        if (!started) {
            started = true;
            if (!ok || !std::isfinite(ft)) return finish(VG_TERM_FAILURE);
            f = initial_cost = ft;
            std::memcpy(g, gt, sizeof g);
            if (max_abs(g) <= gtol) return finish(VG_TERM_CONVERGENCE_GRADIENT);
            return begin_search();
        }
        evals++;
        double dphi = 0.;
        ok = ok && std::isfinite(ft);
        for (int k = 0; ok && k < 6; k++) {
            dphi += gt[k] * d[k];
            ok = std::isfinite(gt[k]);
        }
        const double phi = ok ? ft : HUGE_VAL;   // a failed trial: too far
        if (!ok) dphi = 0.;
        const bool armijo = phi <= phi0 + kC1 * alpha * dphi0, wolfe = std::fabs(dphi) <= -kC2 * dphi0;
        if (!zoom) {
            if (!armijo || (evals > 1 && phi >= phi_prev)) {
                a_lo = a_prev, phi_lo = phi_prev, dphi_lo = dphi_prev;
                a_hi = alpha, phi_hi = phi, dphi_hi = dphi;
                return zoom_trial();
            }
            if (wolfe) return accept(ft, gt);
            if (dphi >= 0.) {
                a_lo = alpha, phi_lo = phi, dphi_lo = dphi;
                a_hi = a_prev, phi_hi = phi_prev, dphi_hi = dphi_prev;
                return zoom_trial();
            }
            if (evals >= kMaxSearchEvals) return finish(VG_TERM_FAILURE);
            a_prev = alpha, phi_prev = phi, dphi_prev = dphi;
            return set_trial(2. * alpha);
        }
        if (!armijo || phi >= phi_lo) {
            a_hi = alpha, phi_hi = phi, dphi_hi = dphi;
        } else {
            if (wolfe) return accept(ft, gt);
            if (dphi * (a_hi - a_lo) >= 0.) a_hi = a_lo, phi_hi = phi_lo, dphi_hi = dphi_lo;
            a_lo = alpha, phi_lo = phi, dphi_lo = dphi;
        }
        zoom_trial();
    }
};

}  // namespace vgp
