// vg_frame_loop.hpp -- the frame-loop core of monocular odometry (section 15) and photometric mapping (section 16): the four
// pipelines and three map triples such a handle owns, the odometry integration, the tail of create, the stage steps of a frame
// and the bodies of the entries both sections have.  A stage step returns a status and writes only into the scratch triples, so
// the caller's frame still commits last.  The two state machines, their Frame / commit, normalize_scale, parameters and key /
// inter image stay in their translation units: they restate different reference code.  Host only, no kernel.
#pragma once

#include <cstring>

#include "vg_handle.hpp"
#include "vg_stereo_host.hpp"
#include "vg_warp_image.hpp"

namespace vgmo {
namespace {   // internal linkage: each of the two translation units has its own copy, and the library exports none of it

using vgi::fail;

constexpr int kMaxPyramid = 8;   // vg_photometric_create refuses more pyramid levels

using vgth::load6;
using vgth::store6;

struct FrameLoop : vgi::HandleBase {
    vg_stereo_params stereo;   // of the per-key-frame SGM objects: equal_margins resolved once into x_max, y_max
    int num_scales = 0;
    double cam[6];
    Array6d xi_base_cam;
    View view;
    int64_t P = 0, img = 0;
    vg_sparse_odom *sparse = nullptr;
    vg_motion_stereo *motion = nullptr;
    vg_depth_fusion *fusion = nullptr;
    vg_photometric *photo = nullptr;
    bool have_odom = false, have_map = false;
    Array6d xi_local{}, xi_local_old{}, xi_odom{};
    vgi::Grow<double> d_maps;   // [3 triples][3][P]
    int map_slot = 0;           // which triple is the map; the other two are scratch
    double *triple(int k) const { return d_maps.get() + (size_t)((map_slot + k) % 3) * 3 * (size_t)P; }   // 0: the map
    ~FrameLoop()
    {
        vg_sparse_odom_destroy(sparse);
        vg_motion_stereo_destroy(motion);
        vg_depth_fusion_destroy(fusion);
        vg_photometric_destroy(photo);
    }
};

// the tail of create behind the caller's own threshold check; what: "<what> has no CPU fallback"
inline int open_loop(FrameLoop *s, int device, void *hip_stream, const double *eucm, const double *xi_base_cam, int width, int height,
                     const vg_motion_stereo_params &motion, const vg_sparse_odom_params &sparse, int num_scales, const char *what)
{
    const vg_stereo_params &sp = motion.stereo;
    if (width != sp.u_max || height != sp.v_max) return fail(VG_ERR_INVALID_ARGUMENT, "the image size must be uMax x vMax of the stereo parameters");
    if (!vgsh::finite_n(xi_base_cam, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "xi_base_cam must be finite");
    // every pipeline checks its own arguments before it asks for the device: a missing device is reported only when all
    // four have accepted theirs
    int rcs[4];
    rcs[0] = vg_motion_stereo_create(&s->motion, device, hip_stream, eucm, eucm, &motion);
    if (rcs[0] == VG_ERR_INVALID_ARGUMENT) return rcs[0];
    rcs[1] = vg_depth_fusion_create(&s->fusion, device, hip_stream, eucm, &sp);
    if (rcs[1] == VG_ERR_INVALID_ARGUMENT) return rcs[1];
    rcs[2] = vg_photometric_create(&s->photo, device, hip_stream, eucm, &sp, xi_base_cam, width, height, num_scales);
    if (rcs[2] == VG_ERR_INVALID_ARGUMENT) return rcs[2];
    rcs[3] = vg_sparse_odom_create(&s->sparse, device, hip_stream, eucm, xi_base_cam, width, height, &sparse);
    if (rcs[3] == VG_ERR_INVALID_ARGUMENT) return rcs[3];
    for (int i = 0; i < 4; i++)
        if (rcs[i]) return rcs[i];
    int x_max = 0, y_max = 0;
    if (const int rc = vg_motion_stereo_size(s->motion, &x_max, &y_max)) return rc;
    s->stereo = sp;
    s->stereo.x_max = x_max;
    s->stereo.y_max = y_max;
    s->stereo.equal_margins = 0;
    s->num_scales = num_scales;
    for (int i = 0; i < 6; i++) s->cam[i] = s->view.cam[i] = eucm[i];
    s->xi_base_cam = load6(xi_base_cam);
    s->view.g = Grid{sp.scale, sp.u0, sp.v0, x_max, y_max};
    s->view.width = width;
    s->view.height = height;
    s->P = (int64_t)x_max * y_max;
    s->img = (int64_t)width * height;
    if (const int rc = s->open(device, hip_stream, what)) return rc;
    VG_HIP(hipSetDevice(device));
    return s->d_maps.grow(9 * (size_t)s->P, "the depth maps");
}

// ---- the stage steps of a frame.  One image of the handle's size, device to device:
inline int copy_image(const FrameLoop *s, uint8_t *dst, const uint8_t *src)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    VG_HIP(hipMemcpyAsync(dst, src, (size_t)s->img, hipMemcpyDeviceToDevice, s->stream));
    return call.finish();
}

// the photometric solve of img from xi_local, which is its prior too, against the key frame the caller has set (set_base or
// vg_photo_set_depth): the solve's pose and report[3] = iterations over the scales, final cost and termination of the finest
inline int solve_photo(FrameLoop *s, const uint8_t *img, const Array6d &xi_local, Array6d &vo, double *report)
{
    if (const int rc = vg_photometric_set_targets(s->photo, 1, img)) return rc;
    const int32_t target = 0;
    double rep[4 * kMaxPyramid];
    if (const int rc = vg_photometric_compute_pose(s->photo, 1, xi_local.data(), &target, xi_local.data(), vo.data(), rep)) return rc;
    report[0] = 0.;
    for (int i = 0; i < s->num_scales; i++) report[0] += rep[4 * (size_t)i];
    report[1] = rep[2];
    report[2] = rep[3];
    return VG_OK;
}

// motion stereo of img at the camera motion `motion` with the map as the prior, then the noise filter: into triple(1)
inline int refine_map(FrameLoop *s, const Array6d &motion, const uint8_t *img, double *counts6)
{
    const double *map = s->triple(0);
    double *m = s->triple(1);
    const size_t P = (size_t)s->P;
    int64_t mc[6];
    if (const int rc = vg_motion_stereo_compute(s->motion, 1, motion.data(), img, map, map + P, map + 2 * P, m, m + P, m + 2 * P, mc)) return rc;
    if (const int rc = vg_depth_filter_noise(s->fusion, 1, m, m + P, m, m + P, nullptr)) return rc;
    for (int i = 0; i < 6; i++) counts6[i] = (double)mc[i];
    return VG_OK;
}

// EnhancedSgm(motion.inverse(), ...): computeStereo(img, key) into triple(1), noise-filtered when `filter`
inline int sgm_map(FrameLoop *s, const Array6d &motion, const uint8_t *img, const uint8_t *key, bool filter)
{
    const Array6d inv = vgth::inverse(motion);
    double *sgm = s->triple(1);
    const size_t P = (size_t)s->P;
    vg_stereo *st = nullptr;
    if (const int rc = vg_stereo_create(&st, s->device, s->stream, s->cam, s->cam, inv.data(), &s->stereo)) return rc;
    const int rc = vg_stereo_compute(st, 1, img, key, sgm, sgm + P, sgm + 2 * P, nullptr);
    vg_stereo_destroy(st);
    if (rc || !filter) return rc;
    return vg_depth_filter_noise(s->fusion, 1, sgm, sgm + P, sgm, sgm + P, nullptr);
}

// the map carried into the frame at `motion`: into triple(2)
inline int warp_map(FrameLoop *s, const Array6d &motion)
{
    const double *map = s->triple(0);
    double *warp = s->triple(2);
    const size_t P = (size_t)s->P;
    return vg_depth_warp(s->fusion, 1, motion.data(), map, map + P, map + 2 * P, warp, warp + P, warp + 2 * P, nullptr);
}

// the SGM map of triple(1) merged into the warped map of triple(2)
inline int merge_maps(FrameLoop *s, double *counts5)
{
    double *sgm = s->triple(1), *warp = s->triple(2);
    const size_t P = (size_t)s->P;
    int64_t mc[5];
    if (const int rc = vg_depth_merge(s->fusion, 1, warp, warp + P, sgm, sgm + P, mc)) return rc;
    for (int i = 0; i < 5; i++) counts5[i] = (double)mc[i];
    return VG_OK;
}

// ---- the bodies of the entries both sections have
inline int size(const FrameLoop *s, int *width, int *height, int *x_max, int *y_max)
{
    if (!s || !width || !height || !x_max || !y_max) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *width = s->view.width;
    *height = s->view.height;
    *x_max = s->view.g.x_max;
    *y_max = s->view.g.y_max;
    return VG_OK;
}

inline int feed_odometry(FrameLoop *s, const double *xi_odom_new)
{
    if (!s || !xi_odom_new) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_odom_new, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the odometry pose must be finite");
    const Array6d xi_new = load6(xi_odom_new);
    if (s->have_odom) s->xi_local = integrate(s->xi_local, s->xi_odom, xi_new);
    s->xi_odom = xi_new;
    s->have_odom = true;
    return VG_OK;
}

// which: 0 xi_local, 1 the frame's pose (H::*frame: xi_global / xi_inter), 2 frame o xi_local
template <class H>
int get_pose(const H *s, Array6d H::*frame, double *xi6, int which)
{
    if (!s || !xi6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    store6(which == 0 ? s->xi_local : which == 1 ? s->*frame : vgth::compose(s->*frame, s->xi_local), xi6);
    return VG_OK;
}

inline int get_map(FrameLoop *s, double *depth, double *sigma, double *cost, const char *null_handle)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, null_handle);
    if (!s->have_map) return fail(VG_ERR_STATE, "no depth map yet");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    double *const out[3] = {depth, sigma, cost};
    for (int i = 0; i < 3; i++)
        if (out[i]) VG_HIP(hipMemcpyAsync(out[i], s->triple(0) + (size_t)i * (size_t)s->P, (size_t)s->P * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    return call.finish();
}

inline int map(const FrameLoop *s, const double **depth, const double **sigma, const double **cost)
{
    if (!s || !depth || !sigma || !cost) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!s->have_map) return fail(VG_ERR_STATE, "no depth map yet");
    *depth = s->triple(0);
    *sigma = s->triple(0) + s->P;
    *cost = s->triple(0) + 2 * s->P;
    return VG_OK;
}

}  // namespace
}  // namespace vgmo
