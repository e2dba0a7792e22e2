// vg_mapping.hpp -- photometric mapping (section 16 of the C ABI): the host arithmetic of the reference's PhotometricMapping state
// machine (src/localization/mapping.cpp: checkDistance :322-332, selectMapFrame :275-300, the scale normalisation of localizePhoto
// :420-459) and the one kernel the loop adds to the pipelines it calls: wrapImage + computeErr (test/localization/map_test.cpp
// :17-32) + the sums of the error in one launch.  The warped value comes from vg_warp_image.hpp's device function, which
// vg_mono_odom_warp_image launches too; the host side of the handle that both sections share is vg_frame_loop.hpp.
#pragma once

#include "vg_warp_image.hpp"

namespace vgmap {

using vgmo::Array6d;
using vgmo::norm3;

enum : int { kBegin = 0, kInit = 1, kLocalize = 2, kSlam = 3 };
enum : int { kWarnNone = 0, kWarnScale = 1, kWarnRotation = 2 };
enum : int {
    kFirst = 0, kWaiting, kInitSlam, kInitLocalize, kLocalizeRefined, kLocalizeInterFrame, kLocalizeMapFrameChanged, kLocalizeMapFrameKept,
    kLocalizeLeftMap, kSlamRefined, kSlamInterFrame, kSlamEnteredMap
};
constexpr double kSelectK = 4.;   // the default K of selectMapFrame; checkDistance's is 1
constexpr int kLanes = vgmo::kLanes;

// checkDistance(xi, K): the thresholds are squares; the angular one is not scaled by K
inline bool check_distance(const vg_mapping_params &p, const Array6d &xi, double K)
{
    const double r = xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5];
    const double d = xi[0] * xi[0] / 5 + xi[1] * xi[1] + xi[2] * xi[2];
    return r < p.new_kf_angular_thresh && d < p.new_kf_distance_thresh * K;
}

// selectMapFrame: among the frames that pass checkDistance(xi^-1 o frame, K), the smallest r + d with the isotropic d; the
// first index wins a tie; -1 when none passes
inline int select_frame(const vg_mapping_params &p, int64_t n, const Array6d *poses, const Array6d &xi, double K)
{
    int res = -1;
    double best = 1e15;   // DOUBLE_MAX (include/std.h)
    for (int64_t i = 0; i < n; i++) {
        const Array6d delta = vgth::inverse_compose(xi, poses[i]);
        const double r = delta[3] * delta[3] + delta[4] * delta[4] + delta[5] * delta[5];
        const double d = delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2];
        if (!check_distance(p, delta, K)) continue;
        if (r + d < best) {
            best = r + d;
            res = (int)i;
        }
    }
    return res;
}

struct Scale {
    Array6d xi;   // the new xi_local
    double K, length, length_prior, rot_diff;
    int warning;
};

// the tail of localizePhoto: prior = xi_local in front of the photometric solve, vo = behind it.  Without normalize_scale the
// solve's pose passes through and the numbers are zero (the caller then leaves xi_local_old alone).
inline Scale normalize_scale(const vg_mapping_params &p, const Array6d &old, const Array6d &prior, const Array6d &vo)
{
    Scale s;
    s.xi = vo;
    s.K = s.length = s.length_prior = s.rot_diff = 0.;
    s.warning = kWarnNone;
    if (!p.normalize_scale) return s;
    const Array6d zeta_prior = vgth::inverse_compose(old, prior);
    Array6d zeta = vgth::inverse_compose(old, vo);
    s.length_prior = norm3(zeta_prior.data());
    s.length = norm3(zeta.data());
    s.rot_diff = std::abs(zeta[5] - zeta_prior[5]);
    s.K = s.length_prior / s.length;
    if (s.rot_diff > p.rotation_tolerance) {   // discard the VO result, rotation error
        s.xi = vgth::compose(old, zeta_prior);
        s.warning = kWarnRotation;
    } else if (s.length > p.min_scale_length) {
        if (s.K < p.min_scale_ratio || s.K > p.max_scale_ratio) {   // too much divergence between WO and VO
            s.xi = vgth::compose(old, zeta_prior);
            s.warning = kWarnScale;
        } else {
            for (int i = 0; i < 3; i++) zeta[i] *= s.K;
            s.xi = vgth::compose(old, zeta);
        }
    }
    return s;
}

// wrapImage of w.src into the key frame, computeErr against base, and the sums, one lane per key frame pixel.  err (may be
// NULL): 0 where either pixel is 0, else 127 + base - warped, saturated.  sums[3] (zeroed by the caller): compared pixels,
// sum |base - warped|, sum (base - warped)^2 -- integers, so the order of the adds does not show in the result.  A wave
// reduces by shuffles (at most 64 * 255^2 per wave fits an int), the workgroup's four waves through LDS, then one atomic per
// sum and workgroup.
struct AlignArgs {
    vgmo::WarpImageArgs w;
    const uint8_t *base;
    uint8_t *err;
    unsigned long long *sums;
};

__global__ __launch_bounds__(kLanes) void mapping_alignment_kernel(AlignArgs a)
{
    __shared__ int part[kLanes / 64][3];
    const int64_t pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    int v[3] = {0, 0, 0};
    if (pix < (int64_t)a.w.v.width * a.w.v.height) {
        const int warped = vgmo::warp_image_value(a.w, pix), b = a.base[pix];
        uint8_t e = 0;
        if (warped != 0 && b != 0) {
            const int d = b - warped, s = 127 + d;
            e = (uint8_t)(s < 0 ? 0 : s > 255 ? 255 : s);
            v[0] = 1;
            v[1] = d < 0 ? -d : d;
            v[2] = d * d;
        }
        if (a.err) a.err[pix] = e;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < 3; k++) v[k] += __shfl_down(v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) part[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long sum = 0;
        for (int w = 0; w < kLanes / 64; w++) sum += (unsigned long long)part[w][threadIdx.x];
        if (sum) atomicAdd(a.sums + threadIdx.x, sum);
    }
}

}  // namespace vgmap
