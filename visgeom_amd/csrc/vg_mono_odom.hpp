// vg_mono_odom.hpp -- monocular visual odometry (section 15 of the C ABI): the host arithmetic of the reference's MonoOdometry
// state machine (src/localization/mono_odom.cpp: feedWheelOdometry, the scale normalisation of feedImage, isNewKeyframeNeeded,
// getCameraMotion) and the two kernels the loop adds to the pipelines it calls: MonoOdometry::setDepth (:63-79) and
// ScalePhotometric::wrapImage (src/localization/photometric.cpp:387-415), both one lane per output element and pure gathers.
// Evaluated in the order written (-ffp-contract=off), so tests/mono_odom_ref.py agrees bit for bit on the kernels.
#pragma once

#include "vg_stereo_device.hpp"
#include "vg_internal.hpp"
#include "vg_transf_host.hpp"

namespace vgmo {

using vgth::Array6d;

enum : int { kBegin = 0, kSparseInit = 1, kReady = 2 };
enum : int { kFirst = 0, kWaiting = 1, kSparseInitKeyframe = 2, kRefined = 3, kKeyframe = 4, kDiscarded = 5 };
constexpr double kSetDepthSigma = 0.1;
constexpr double kDefaultCost = 5.;   // DEFAULT_COST_DEPTH (stereo_misc.h)
constexpr int kLanes = 256;

inline double norm3(const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// feedWheelOdometry: xi_local.composeInverse(xi_odom).compose(xi_odom_new)
inline Array6d integrate(const Array6d &xi_local, const Array6d &xi_odom, const Array6d &xi_odom_new)
{
    return vgth::compose(vgth::compose_inverse(xi_local, xi_odom), xi_odom_new);
}

// getCameraMotion: xi_base_cam.inverseCompose(xi).compose(xi_base_cam)
inline Array6d camera_motion(const Array6d &xi_base_cam, const Array6d &xi)
{
    return vgth::compose(vgth::inverse_compose(xi_base_cam, xi), xi_base_cam);
}

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

using namespace vgs;

struct Grid {   // ScaleParameters (vgd::Grid's fields; vg_depth.hpp defines kernels and belongs to its own translation unit)
    int scale, u0, v0, x_max, y_max;
};

struct View {   // what both kernels read about the handle
    double cam[6];
    Grid g;
    int width, height;
};

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

// wrapImage: Rinv, t = the camera motion of the pose (rotMatInv, trans); one lane per key frame pixel
struct WarpImageArgs {
    View v;
    double Rinv[9], t[3];
    const double *depth;   // [y_max][x_max]
    const uint8_t *src;
    uint8_t *dst;
};

__global__ __launch_bounds__(kLanes) void mono_odom_warp_image_kernel(WarpImageArgs a)
{
    const int64_t pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= (int64_t)a.v.width * a.v.height) return;
    const int j = (int)(pix % a.v.width), i = (int)(pix / a.v.width);
    const Grid &g = a.v.g;
    uint8_t out = 0;
    const int xd = round_int((double)(j - g.u0) / g.scale), yd = round_int((double)(i - g.v0) / g.scale);   // xConv, yConv
    if (xd >= 0 && xd < g.x_max && yd >= 0 && yd < g.y_max) {
        const double d = a.depth[(int64_t)yd * g.x_max + xd];
        double X[3], X1[3], X2[3], q[2];
        if (d >= kMinDepth && eucm_reconstruct(a.v.cam, (double)j, (double)i, X)) {   // false for NaN
            const double nrm = sqrt(dot3(X, X));
            for (int k = 0; k < 3; k++) X1[k] = X[k] / nrm * d - a.t[k];   // normalized() * depth, then inverseTransform
            mat_vec(a.Rinv, X1, X2);
            if (eucm_project(a.v.cam, X2, q) && coord_ok(q)) {
                const int u = round_int(q[0]), w = round_int(q[1]);
                if (u >= 0 && u < a.v.width && w >= 0 && w < a.v.height) out = a.src[(int64_t)w * a.v.width + u];
            }
        }
    }
    a.dst[pix] = out;
}

}  // namespace vgmo
