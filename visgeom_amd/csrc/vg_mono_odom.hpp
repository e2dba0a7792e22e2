// vg_mono_odom.hpp -- monocular visual odometry (section 15 of the C ABI): the host arithmetic of the reference's MonoOdometry
// state machine (src/localization/mono_odom.cpp: feedWheelOdometry, the scale normalisation of feedImage, isNewKeyframeNeeded,
// getCameraMotion) and the two kernels the loop adds to the pipelines it calls: MonoOdometry::setDepth (:63-79) and
// ScalePhotometric::wrapImage (src/localization/photometric.cpp:387-415), both one lane per output element and pure gathers.
// Evaluated in the order written (-ffp-contract=off), so tests/mono_odom_ref.py agrees bit for bit on the kernels.  The pose
// integration, getCameraMotion and wrapImage's device function live in vg_warp_image.hpp, the host side of the handle in
// vg_frame_loop.hpp, both shared with section 16.
#pragma once

#include "vg_warp_image.hpp"

namespace vgmo {

enum : int { kBegin = 0, kSparseInit = 1, kReady = 2 };
enum : int { kFirst = 0, kWaiting = 1, kSparseInitKeyframe = 2, kRefined = 3, kKeyframe = 4, kDiscarded = 5 };
constexpr double kSetDepthSigma = 0.1;
constexpr double kDefaultCost = 5.;   // DEFAULT_COST_DEPTH (stereo_misc.h)

struct Scale {
    Array6d xi;   // the new xi_local
    double K, length, length_prior;
    bool discarded;
};

// the scale normalisation of feedImage (:120-139): prior = xi_local in front of the photometric solve, vo = behind it
inline Scale normalize_scale(const vg_mono_odom_params &p, const Array6d &old, const Array6d &prior, const Array6d &vo)
{
    Scale s;
    const Array6d zeta_prior = vgth::inverse_compose(old, prior);
    Array6d zeta = vgth::inverse_compose(old, vo);
    s.length_prior = norm3(zeta_prior.data());
    s.length = norm3(zeta.data());
    s.K = s.length_prior / s.length;
    s.discarded = false;
    if (s.length > p.min_scale_length) {
        if (s.K > p.max_scale_ratio) {   // too much divergence between wheel and visual odometry
            s.xi = vgth::compose(old, zeta_prior);
            s.discarded = true;
            return s;
        }
        for (int i = 0; i < 3; i++) zeta[i] *= s.K;
    }
    s.xi = vgth::compose(old, zeta);
    return s;
}

// isNewKeyframeNeeded
inline bool needs_keyframe(const vg_mono_odom_params &p, const Array6d &xi_local)
{
    return norm3(xi_local.data()) > p.max_dist || norm3(xi_local.data() + 3) > p.max_angle;
}

// setDepth: cell (x, y) takes the depth image at (uConv(x), vConv(y)); cost (may be NULL) is set to DEFAULT_COST_DEPTH
__global__ __launch_bounds__(kLanes) void mono_odom_set_depth_kernel(View v, const float *image, double *depth, double *sigma, double *cost)
{
    const int64_t pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= (int64_t)v.g.x_max * v.g.y_max) return;
    const int x = (int)(pix % v.g.x_max), y = (int)(pix / v.g.x_max);
    const int u = x * v.g.scale + v.g.u0, w = y * v.g.scale + v.g.v0;
    const bool inside = u >= 0 && u < v.width && w >= 0 && w < v.height;
    depth[pix] = inside ? (double)image[(int64_t)w * v.width + u] : 0.;
    sigma[pix] = kSetDepthSigma;
    if (cost) cost[pix] = kDefaultCost;
}

// wrapImage, one lane per key frame pixel (WarpImageArgs, warp_image_value: vg_warp_image.hpp)
__global__ __launch_bounds__(kLanes) void mono_odom_warp_image_kernel(WarpImageArgs a)
{
    const int64_t pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= (int64_t)a.v.width * a.v.height) return;
    a.dst[pix] = warp_image_value(a, pix);
}

}  // namespace vgmo
