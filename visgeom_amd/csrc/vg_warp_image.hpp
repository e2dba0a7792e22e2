// vg_warp_image.hpp -- what monocular odometry (section 15) and photometric mapping (section 16) share: the host pose arithmetic
// of both state machines (feedOdometry's integration, getCameraMotion) and the device function of ScalePhotometric::wrapImage
// (src/localization/photometric.cpp:387-415), one key frame pixel per call and a pure gather.  No kernel is defined here, so
// both translation units include it.  Evaluated in the order written (-ffp-contract=off): tests/mono_odom_ref.py agrees bit for bit.
// The handle the two sections share -- members, create, stage steps, small entries -- is vg_frame_loop.hpp, built on this.
#pragma once

#include "vg_image_device.hpp"
#include "vg_internal.hpp"
#include "vg_pose_host.hpp"

namespace vgmo {

using vgth::Array6d;

constexpr int kLanes = 256;

inline double norm3(const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// feedWheelOdometry / feedOdometry: xi_local.composeInverse(xi_odom).compose(xi_odom_new)
inline Array6d integrate(const Array6d &xi_local, const Array6d &xi_odom, const Array6d &xi_odom_new)
{
    return vgth::compose(vgth::compose_inverse(xi_local, xi_odom), xi_odom_new);
}

// getCameraMotion: xi_base_cam.inverseCompose(xi).compose(xi_base_cam)
inline Array6d camera_motion(const Array6d &xi_base_cam, const Array6d &xi)
{
    return vgth::compose(vgth::inverse_compose(xi_base_cam, xi), xi_base_cam);
}

using namespace vgs;

struct View {   // what the kernels read about the handle
    double cam[6];
    Grid g;
    int width, height;
};

// wrapImage: Rinv, t = the camera motion of the pose (rotMatInv, trans); one lane per key frame pixel
struct WarpImageArgs {
    View v;
    double Rinv[9], t[3];
    const double *depth;   // [y_max][x_max]
    const uint8_t *src;
    uint8_t *dst;
};

// the value wrapImage writes at key frame pixel pix (< width * height): src at the rounded projection of the pixel's point, 0
// where nothing lands
__device__ inline uint8_t warp_image_value(const WarpImageArgs &a, int64_t pix)
{
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
    return out;
}

// the host half of a warp: the camera motion of the base-frame pose xi into the launch arguments (depth, src, dst left to the caller)
inline void warp_image_pose(const Array6d &xi_base_cam, const Array6d &xi, WarpImageArgs &args)
{
    const Array6d motion = camera_motion(xi_base_cam, xi);
    vgth::inverse_frame(motion.data(), args.Rinv, args.t);   // rotMatInv, trans
}

}  // namespace vgmo
